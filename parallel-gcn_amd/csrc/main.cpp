// parallel-gcn_amd/csrc/main.cpp -- `gcn-par <dataset> [file=<params>] [root=<dir>] [cache=1]
//   [epochs=<n>] [residual=1] [layer_norm=1] [attention=1] [heads=<K>] [attn_dropout=<p>] [aggregator=mean|max] [root_weight=1] [multilabel=1] [readout=sum|mean|max] [link=dot embed=<D> [rank=1|<file>] [recommend=<file> [topk=<K>]]] [load=<checkpoint>] [save=<checkpoint>] [predict=<file>]`
// The reference's entry point (src/main.cpp:9-61): parse the dataset with the kept loader,
// build the GCN, run the epochs printing the reference's epoch lines.  Parameters come from
// a key=value file with the reference's keys (parameters/parameters_<ds>.txt layout:
// n_layers, hidden_dims, dropouts, epochs, early_stopping, learning_rate, weight_decay,
// beta1, beta2, eps, seed (srand seed of the xorshift state); the CUDA launch knobs
// num_blocks_factor/num_threads are accepted and ignored) -- our own tiny parser, GetPot is
// not vendored; residual=1, in the file or on the command line, adds the reference's
// ResidualConnection to the middle layers of equal width, pgcn_params.residual; layer_norm=1
// likewise puts a LayerNorm between every hidden layer's GraphSum and ReLU, pgcn_params.layer_norm).  no_feature=1 is the PART2 NO_FEATURE build (feature values 1.0).
// New with the engine: load= resumes from a checkpoint before the run (the epoch lines go on
// from its epoch count, up to `epochs`), save= writes one after it, predict= writes one line
// `node class confidence` per node after it; epochs= overrides the parameter file's.
// multilabel=1 (command line or parameter file): multi-label classification, pgcn_params.multilabel
// -- the labels come from the sidecar file data/<name>.labels (line i: the class ids of node i),
// the epoch lines' accuracy column is the Hamming accuracy, and predict= writes `node id id ...`
// (the classes with a positive logit) per node.
// attention=1 (command line or parameter file): graph attention layers in the GraphSums' place,
// pgcn_params.attention; heads=<K> runs its hidden layers with K heads concatenated inside their
// widths and attn_dropout=<p> drops attention weights in training (pgcn_params.attention_heads /
// attention_dropout; `gcn-par cora attention=1 heads=8 attn_dropout=0.6` with hidden_dims=64 is
// the published GAT), both also keys of the parameter file.
// aggregator=mean|max (or 1|2) [root_weight=1] (command line or parameter file): GraphSAGE layers
// in the GraphSums' place, pgcn_params.aggregator / root_weight; `gcn-par cora aggregator=max
// root_weight=1` trains the max-pooling variant with a self term.
// readout=sum|mean|max (or 1|2|3; command line or parameter file): graph classification,
// pgcn_params.readout -- the nodes are a batch of graphs read from the sidecar file
// data/<name>.graphs (line g: `<rows> <label> <split>`), loss and accuracy are per graph, and
// predict= writes one line `graph class confidence` per graph.
// link=dot (or 1) [embed=<D>, default 32] (command line or parameter file): link prediction,
// pgcn_params.link_decoder -- the pairs come from the sidecar file data/<name>.links (line e:
// `<src> <dst> <label> <split>`), the output layer is a D-wide node embedding, loss and accuracy
// are per pair, and predict= writes one line `src dst score probability` per pair.  The adjacency
// is used as loaded: keep validation and test positives out of it.
// rank=1 (with link=): after the run, one line with the filtered ranking metrics of the test split
// (pgcn_gcn_link_ranks; mean ties) for both sides: `rank side=dst queries=.. mrr=.. hits@10=..
// hits@50=.. hits@100=.. side=src ...`; rank=<file> also writes `src dst greater equal` per test
// positive pair for the dst side.
// recommend=<file> [topk=<K>, default 10, at most 128] (with link=): after the run, one line per
// node `node v1 s1 v2 s2 ...` with the K best destinations for the node as a source
// (pgcn_gcn_top_links: dst side, filtered -- the node, its neighbours and its known links are left
// out -- best first, ties to the lower index; a node with fewer than K candidates gets a shorter
// line).
#include <algorithm>
#include <vector>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "../../include/pgcn.h"

static void trim(std::string &s) {
  size_t a = s.find_first_not_of(" \t\r\n"), b = s.find_last_not_of(" \t\r\n");
  s = a == std::string::npos ? "" : s.substr(a, b - a + 1);
}

// aggregator=: mean / max by name or 0 / 1 / 2; anything else is left for the engine to refuse
static int aggregator_id(const std::string &v) {
  if (v == "mean") return 1;
  if (v == "max") return 2;
  if (v == "gcn" || v == "none") return 0;
  char *end = nullptr;
  const long x = std::strtol(v.c_str(), &end, 10);
  return (end && *end == '\0' && !v.empty()) ? (int)x : -1;
}

// readout=: sum / mean / max by name or 0 .. 3; anything else is left for the engine to refuse
static int readout_id(const std::string &v) {
  if (v == "sum") return 1;
  if (v == "mean") return 2;
  if (v == "max") return 3;
  if (v == "none") return 0;
  char *end = nullptr;
  const long x = std::strtol(v.c_str(), &end, 10);
  return (end && *end == '\0' && !v.empty()) ? (int)x : -1;
}

// link=: dot by name or 0 / 1; anything else is left for the engine to refuse
static int link_id(const std::string &v) {
  if (v == "dot") return 1;
  if (v == "none") return 0;
  char *end = nullptr;
  const long x = std::strtol(v.c_str(), &end, 10);
  return (end && *end == '\0' && !v.empty()) ? (int)x : -1;
}

static bool load_params(const char *path, pgcn_params *p, int *embed) {
  std::ifstream f(path);
  if (!f.is_open()) return false;
  std::string line;
  while (std::getline(f, line)) {
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line = line.substr(0, hash);
    const size_t eq = line.find('=');
    if (eq == std::string::npos) continue;
    std::string k = line.substr(0, eq), v = line.substr(eq + 1);
    trim(k);
    trim(v);
    auto list = [&](auto *dst, bool is_float) {
      std::stringstream ss(v);
      std::string tok;
      int n = 0;
      while (std::getline(ss, tok, ',') && n < PGCN_MAX_LAYERS) {
        if (is_float) ((float *)dst)[n++] = std::strtof(tok.c_str(), nullptr);
        else ((int *)dst)[n++] = std::atoi(tok.c_str());
      }
      return n;
    };
    if (k == "n_layers") p->n_layers = std::atoi(v.c_str());
    else if (k == "hidden_dims") list(p->hidden_dims, false);
    else if (k == "dropouts") list(p->dropouts, true);
    else if (k == "epochs") p->epochs = std::atoi(v.c_str());
    else if (k == "early_stopping") p->early_stopping = std::atoi(v.c_str());
    else if (k == "learning_rate") p->learning_rate = std::strtof(v.c_str(), nullptr);
    else if (k == "weight_decay") p->weight_decay = std::strtof(v.c_str(), nullptr);
    else if (k == "beta1") p->beta1 = std::strtof(v.c_str(), nullptr);
    else if (k == "beta2") p->beta2 = std::strtof(v.c_str(), nullptr);
    else if (k == "eps") p->eps = std::strtof(v.c_str(), nullptr);
    else if (k == "seed") p->seed = (unsigned)std::strtoul(v.c_str(), nullptr, 10);
    else if (k == "residual") p->residual = std::atoi(v.c_str());
    else if (k == "layer_norm") p->layer_norm = std::atoi(v.c_str());
    else if (k == "attention") p->attention = std::atoi(v.c_str());
    else if (k == "multilabel") p->multilabel = std::atoi(v.c_str());
    else if (k == "heads") p->attention_heads = std::atoi(v.c_str());
    else if (k == "attn_dropout") p->attention_dropout = std::strtof(v.c_str(), nullptr);
    else if (k == "aggregator") p->aggregator = aggregator_id(v);
    else if (k == "root_weight") p->root_weight = std::atoi(v.c_str());
    else if (k == "readout") p->readout = readout_id(v);
    else if (k == "link") p->link_decoder = link_id(v);
    else if (k == "embed") *embed = std::atoi(v.c_str());
  }
  return true;
}

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "Give one input file name as argument [cora pubmed citeseer reddit]\n");
    return EXIT_FAILURE;
  }
  const char *name = argv[1];
  std::string root = ".", file;
  bool cache = false;  // cache=1: read/write the binary dataset cache data/<name>.pgcnbin
  bool no_feature = false;  // no_feature=1: the PART2 NO_FEATURE build (feature values 1.0)
  std::string load, save, predict, rank, recommend;
  int topk = 10;
  int epochs = -1, residual = -1, layer_norm = -1, multilabel = -1, attention = -1, heads = -1;
  float attn_dropout = -1.0f;
  int root_weight = -1;
  std::string aggregator, readout, link;
  int embed = 32, embed_arg = -1;
  for (int i = 2; i < argc; i++) {
    if (!std::strncmp(argv[i], "file=", 5)) file = argv[i] + 5;
    if (!std::strncmp(argv[i], "root=", 5)) root = argv[i] + 5;
    if (!std::strcmp(argv[i], "cache=1")) cache = true;
    if (!std::strcmp(argv[i], "no_feature=1")) no_feature = true;
    if (!std::strncmp(argv[i], "load=", 5)) load = argv[i] + 5;
    if (!std::strncmp(argv[i], "save=", 5)) save = argv[i] + 5;
    if (!std::strncmp(argv[i], "predict=", 8)) predict = argv[i] + 8;
    if (!std::strncmp(argv[i], "epochs=", 7)) epochs = std::atoi(argv[i] + 7);
    if (!std::strncmp(argv[i], "residual=", 9)) residual = std::atoi(argv[i] + 9);
    if (!std::strncmp(argv[i], "layer_norm=", 11)) layer_norm = std::atoi(argv[i] + 11);
    if (!std::strncmp(argv[i], "multilabel=", 11)) multilabel = std::atoi(argv[i] + 11);
    if (!std::strncmp(argv[i], "attention=", 10)) attention = std::atoi(argv[i] + 10);
    if (!std::strncmp(argv[i], "heads=", 6)) heads = std::atoi(argv[i] + 6);
    if (!std::strncmp(argv[i], "attn_dropout=", 13))
      attn_dropout = std::strtof(argv[i] + 13, nullptr);
    if (!std::strncmp(argv[i], "aggregator=", 11)) aggregator = argv[i] + 11;
    if (!std::strncmp(argv[i], "root_weight=", 12)) root_weight = std::atoi(argv[i] + 12);
    if (!std::strncmp(argv[i], "readout=", 8)) readout = argv[i] + 8;
    if (!std::strncmp(argv[i], "link=", 5)) link = argv[i] + 5;
    if (!std::strncmp(argv[i], "embed=", 6)) embed_arg = std::atoi(argv[i] + 6);
    if (!std::strncmp(argv[i], "rank=", 5)) rank = argv[i] + 5;
    if (!std::strncmp(argv[i], "recommend=", 10)) recommend = argv[i] + 10;
    if (!std::strncmp(argv[i], "topk=", 5)) topk = std::atoi(argv[i] + 5);
  }
  pgcn_params p;
  pgcn_params_default(&p);
  if (!file.empty() && !load_params(file.c_str(), &p, &embed)) {
    fprintf(stderr, "cannot read parameter file %s\n", file.c_str());
    return EXIT_FAILURE;
  }
  if (epochs >= 0) p.epochs = epochs;
  if (residual >= 0) p.residual = residual;
  if (layer_norm >= 0) p.layer_norm = layer_norm;
  if (multilabel >= 0) p.multilabel = multilabel;
  if (attention >= 0) p.attention = attention;
  if (heads >= 0) p.attention_heads = heads;
  if (attn_dropout >= 0.0f) p.attention_dropout = attn_dropout;
  if (!aggregator.empty()) p.aggregator = aggregator_id(aggregator);
  if (root_weight >= 0) p.root_weight = root_weight;
  if (!readout.empty()) p.readout = readout_id(readout);
  if (!link.empty()) p.link_decoder = link_id(link);
  if (embed_arg >= 0) embed = embed_arg;
  pgcn_dataset *ds = nullptr;
  const int lst = cache ? pgcn_dataset_load_cached(root.c_str(), name, &ds, nullptr)
                        : pgcn_dataset_load(root.c_str(), name, &ds);
  if (lst != PGCN_OK) {
    fprintf(stderr, "Cannot read input: %s\n", name);
    return EXIT_FAILURE;
  }
  if (no_feature) pgcn_dataset_binarize(ds);
  if (p.multilabel) {
    const std::string labels = root + "/data/" + name + ".labels";
    if (pgcn_dataset_load_labels(ds, labels.c_str(), 0) != PGCN_OK) {
      fprintf(stderr, "Cannot read labels: %s\n", labels.c_str());
      return EXIT_FAILURE;
    }
  }
  if (p.readout) {
    const std::string graphs = root + "/data/" + name + ".graphs";
    if (pgcn_dataset_load_graphs(ds, graphs.c_str(), 0) != PGCN_OK) {
      fprintf(stderr, "Cannot read graphs: %s\n", graphs.c_str());
      return EXIT_FAILURE;
    }
  }
  if (p.link_decoder) {
    const std::string links = root + "/data/" + name + ".links";
    if (pgcn_dataset_load_links(ds, links.c_str(), embed) != PGCN_OK) {
      fprintf(stderr, "Cannot read links: %s (embed=%d)\n", links.c_str(), embed);
      return EXIT_FAILURE;
    }
  }
  pgcn_data view;
  pgcn_dataset_view(ds, &view, &p.input_dim, &p.output_dim);
  p.num_nodes = view.num_nodes;
  pgcn_gcn *g = nullptr;
  int st = pgcn_gcn_create(&p, &view, 0, &g);
  if (st != PGCN_OK) {
    fprintf(stderr, "GCN creation failed: %s\n", pgcn_status_string(st));
    return EXIT_FAILURE;
  }
  if (!load.empty() && (st = pgcn_gcn_load(g, load.c_str(), 0)) != PGCN_OK) {
    fprintf(stderr, "cannot resume from %s: %s\n", load.c_str(), pgcn_status_string(st));
    return EXIT_FAILURE;
  }
  st = pgcn_gcn_run(g, 1);
  if (st == PGCN_OK && !save.empty() && (st = pgcn_gcn_save(g, save.c_str())) != PGCN_OK)
    fprintf(stderr, "cannot save %s: %s\n", save.c_str(), pgcn_status_string(st));
  if (st == PGCN_OK && !predict.empty() && p.multilabel) {
    const int words = (p.output_dim + 31) / 32;
    std::vector<uint32_t> bits((size_t)view.num_nodes * words);
    const long long n = pgcn_gcn_predict_multilabel(g, bits.data(), nullptr);
    FILE *f = n >= 0 ? std::fopen(predict.c_str(), "w") : nullptr;
    if (!f) {
      fprintf(stderr, "cannot write predictions to %s\n", predict.c_str());
      st = n < 0 ? (int)n : PGCN_E_IO;
    } else {
      for (long long i = 0; i < n; i++) {
        fprintf(f, "%lld", i);
        for (int j = 0; j < p.output_dim; j++)
          if ((bits[(size_t)i * words + j / 32] >> (j % 32)) & 1u) fprintf(f, " %d", j);
        fprintf(f, "\n");
      }
      std::fclose(f);
    }
  } else if (st == PGCN_OK && !predict.empty() && p.link_decoder) {
    std::vector<float> score((size_t)view.num_pairs), prob((size_t)view.num_pairs);
    const long long n = pgcn_gcn_predict_links(g, score.data(), prob.data());
    FILE *f = n >= 0 ? std::fopen(predict.c_str(), "w") : nullptr;
    if (!f) {
      fprintf(stderr, "cannot write predictions to %s\n", predict.c_str());
      st = n < 0 ? (int)n : PGCN_E_IO;
    } else {
      for (long long e = 0; e < n; e++)
        fprintf(f, "%d %d %.6f %.6f\n", view.pair_src[e], view.pair_dst[e], score[(size_t)e],
                prob[(size_t)e]);
      std::fclose(f);
    }
  } else if (st == PGCN_OK && !predict.empty()) {
    // (one row per node, or per graph under readout)
    const size_t rows = (size_t)std::max(view.num_nodes, view.num_graphs);
    std::vector<int> cls(rows);
    std::vector<float> conf(rows);
    const long long n = pgcn_gcn_predict(g, cls.data(), conf.data(), nullptr);
    FILE *f = n >= 0 ? std::fopen(predict.c_str(), "w") : nullptr;
    if (!f) {
      fprintf(stderr, "cannot write predictions to %s\n", predict.c_str());
      st = n < 0 ? (int)n : PGCN_E_IO;
    } else {
      for (long long i = 0; i < n; i++)
        fprintf(f, "%lld %d %.6f\n", i, cls[(size_t)i], conf[(size_t)i]);
      std::fclose(f);
    }
  }
  if (st == PGCN_OK && !rank.empty() && rank != "0" && p.link_decoder) {
    printf("rank");
    for (int side = 0; side < 2 && st == PGCN_OK; side++) {
      const long long q = pgcn_gcn_link_ranks(g, 3, side, 1, nullptr, nullptr);
      std::vector<long long> greater((size_t)std::max(q, 0LL)), equal(greater.size());
      const long long got = q < 0 ? q : pgcn_gcn_link_ranks(g, 3, side, 1, greater.data(), equal.data());
      if (got < 0) {
        st = (int)got;
        break;
      }
      double rr = 0.0;
      long long hits[3] = {0, 0, 0};
      const double at[3] = {10.0, 50.0, 100.0};
      for (long long e = 0; e < q; e++) {
        const double r = (double)greater[(size_t)e] + (double)equal[(size_t)e] / 2.0 + 1.0;
        rr += 1.0 / r;
        for (int k = 0; k < 3; k++) hits[k] += r <= at[k];
      }
      const double den = q > 0 ? (double)q : 1.0;
      printf(" side=%s queries=%lld mrr=%.6f hits@10=%.6f hits@50=%.6f hits@100=%.6f",
             side == 0 ? "dst" : "src", q, rr / den, hits[0] / den, hits[1] / den, hits[2] / den);
      if (side == 0 && rank != "1") {
        FILE *f = std::fopen(rank.c_str(), "w");
        if (!f) {
          fprintf(stderr, "cannot write ranks to %s\n", rank.c_str());
          st = PGCN_E_IO;
        } else {
          long long k = 0;
          for (long long e = 0; e < view.num_pairs; e++)
            if (view.pair_label[e] == 1 && view.pair_split[e] == 3) {
              fprintf(f, "%d %d %lld %lld\n", view.pair_src[e], view.pair_dst[e], greater[(size_t)k],
                      equal[(size_t)k]);
              k++;
            }
          std::fclose(f);
        }
      }
    }
    printf("\n");
    if (st != PGCN_OK) fprintf(stderr, "ranking failed: %s\n", pgcn_status_string(st));
  }
  if (st == PGCN_OK && !recommend.empty() && p.link_decoder) {
    const long long m = view.num_nodes;
    std::vector<int> nodes((size_t)m), idx((size_t)m * (size_t)std::max(topk, 0));
    std::vector<float> score(idx.size());
    for (long long i = 0; i < m; i++) nodes[(size_t)i] = (int)i;
    const long long got = pgcn_gcn_top_links(g, nodes.data(), m, topk, 0, 1, idx.data(), score.data());
    FILE *f = got >= 0 ? std::fopen(recommend.c_str(), "w") : nullptr;
    if (!f) {
      fprintf(stderr, "cannot write recommendations to %s%s%s\n", recommend.c_str(),
              got < 0 ? ": " : "", got < 0 ? pgcn_status_string((int)got) : "");
      st = got < 0 ? (int)got : PGCN_E_IO;
    } else {
      for (long long i = 0; i < m; i++) {
        fprintf(f, "%lld", i);
        for (int j = 0; j < topk && idx[(size_t)(i * topk + j)] >= 0; j++)
          fprintf(f, " %d %.6f", idx[(size_t)(i * topk + j)], score[(size_t)(i * topk + j)]);
        fprintf(f, "\n");
      }
      std::fclose(f);
    }
  }
  pgcn_gcn_destroy(g);
  pgcn_dataset_free(ds);
  return st == PGCN_OK ? EXIT_SUCCESS : EXIT_FAILURE;
}
