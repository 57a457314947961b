// parallel-gcn_amd/csrc/host/data.hpp -- host-side graph data and the kept hpdga loader.
//
// SparseIndex / GCNData mirror include/sparse.cuh:11-17 and include/gcn.cuh:51-58 (and
// hpdga-spring23/include/sparse.h:12-17, gcn.h:18-24). Parser keeps the hpdga loader's API
// and semantics (hpdga-spring23/include/parser.h:10-24, src/parser.cpp:6-140): implicit
// self loop first, neighbours in file order, duplicates kept, an unterminated last line
// dropped, empty svmlight lines give label -1, input_dim = max feature id + 1,
// output_dim = max label + 1.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace pgcn {

struct SparseIndex {
  std::vector<int> indices;
  std::vector<int> indptr;
};

struct GCNData {
  SparseIndex feature_index, graph;
  std::vector<int> split;
  std::vector<int> label;
  std::vector<float> feature_value;
  int num_nodes = 0, input_dim = 0, output_dim = 0;
  // multi-label data (empty / 0: single-label): [num_nodes][label_words] bits, bit j % 32 of
  // word j / 32 = node i has class j; a node is labelled iff label[i] >= 0
  std::vector<uint32_t> label_bits;
  int label_words = 0;
  // graph-level data (0 / empty: none): graph g owns rows [graph_ptr[g], graph_ptr[g + 1]);
  // graph_label in [0, output_dim) or -1, graph_split 0..3 (GCNParams::readout)
  int num_graphs = 0;
  std::vector<int> graph_ptr, graph_label, graph_split;
  // pair-level data for link prediction (empty: none): pair e = (pair_src[e], pair_dst[e]),
  // pair_label 1 / 0 / -1 (unlabelled), pair_split 0..3 (GCNParams::link_decoder)
  std::vector<int> pair_src, pair_dst, pair_label, pair_split;
};

class Parser {
 public:
  // Opens <root>/data/<name>.{graph,split,svmlight} (the reference opens data/<name>.*
  // relative to the working directory; root "." reproduces that).
  Parser(GCNData *data, const std::string &name, const std::string &root = ".");
  bool parse();

 private:
  GCNData *data_;
  std::string graph_path_, split_path_, svm_path_;
};

// Seeded reddit-shaped synthetic dataset: Chung-Lu power-law graph
// (Pareto alpha 1.8 weights capped at 40x mean, no self loops before the loader's implicit
// ones, neighbours sorted), dense N(0,1) features quantised to 4 decimals, uniform labels,
// split sizes scaled from reddit's 153,431 / 23,831 / 55,703.
void make_synthetic(GCNData *d, int n, int f, int c, long long undirected_edges,
                    uint64_t seed);

// Binary dataset cache: the parsed arrays of GCNData as one file
// ("PGCNDS01" header, sizes, the source files' size + mtime stamps, raw little-endian arrays,
// FNV-1a 64 checksum of the payload).  load_binary fails (returns false) on a missing file,
// another version, stamps that differ from `stamps` (when given), a short file or a checksum
// mismatch; the caller then parses the text.
// FNV-1a 64 over n bytes, continued from h (kFnvBasis to start): the checksum of the binary
// files this library writes (the dataset cache here, training checkpoints in checkpoint.cpp)
constexpr uint64_t kFnvBasis = 14695981039346656037ull;
uint64_t fnv1a(uint64_t h, const void *p, size_t n);
struct FileStamp {
  long long size = -1, mtime_ns = -1;
};
bool stamp_file(const std::string &path, FileStamp *st);
bool save_binary(const GCNData &d, const std::string &path, const FileStamp stamps[3]);
bool load_binary(GCNData *d, const std::string &path, const FileStamp *stamps);
// Parser + cache: <root>/data/<name>.pgcnbin is read when its stamps match the three text
// files, else the text is parsed and the cache (re)written (best effort).  *from_cache tells
// which happened.
bool load_dataset_cached(GCNData *d, const std::string &root, const std::string &name,
                         bool *from_cache);

// Multi-label sidecar file: line i = the class ids of node i separated by blanks (an empty line:
// no class).  Fills bits [num_nodes][words] and *classes (num_classes, or max id + 1 when 0);
// false (with *why) for a missing file, a line count other than num_nodes, a token that is not
// a number or an id outside [0, min(num_classes or 128, 128)).
bool read_labels_file(const std::string &path, int num_nodes, int num_classes,
                      std::vector<uint32_t> *bits, int *words, int *classes, std::string *why);

// Graph-level sidecar file: line g = `<rows> <label> <split>`.  Fills ptr [G + 1], label, split and
// *classes (num_classes, or max label + 1 when 0); false (with *why) for a missing file, a line
// that is not three integers, negative rows, rows that do not sum to num_nodes, a label below -1
// or >= min(num_classes or 128, 128), a split outside 0..3.
bool read_graphs_file(const std::string &path, int num_nodes, int num_classes,
                      std::vector<int> *ptr, std::vector<int> *label, std::vector<int> *split,
                      int *classes, std::string *why);
// graph arrays as GCNData holds them: ptr [G + 1] from 0 to num_nodes, non-decreasing, labels in
// [-1, classes), splits in 0..3
bool graphs_valid(int num_nodes, int G, const int *ptr, const int *label, const int *split,
                  int classes);

// Link-prediction sidecar file: line e = `<src> <dst> <label> <split>`.  Fills the four arrays;
// false (with *why) for a missing file, a line that is not four integers, an endpoint outside
// [0, num_nodes), a label outside {-1, 0, 1}, a split outside 0..3, no pair at all.
bool read_links_file(const std::string &path, int num_nodes, std::vector<int> *src,
                     std::vector<int> *dst, std::vector<int> *label, std::vector<int> *split,
                     std::string *why);
// pair arrays as GCNData holds them: E >= 1 pairs within an int, endpoints in [0, num_nodes),
// labels in {-1, 0, 1}, splits in 0..3
bool links_valid(int num_nodes, long long E, const int *src, const int *dst, const int *label,
                 const int *split);

// True when every row lists all features 0..F-1 in order (a dense matrix in CSR form).
bool features_dense(const GCNData &d);

}  // namespace pgcn
