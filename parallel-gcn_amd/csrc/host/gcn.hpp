// parallel-gcn_amd/csrc/host/gcn.hpp -- GCNParams / AdamParams / Adam / GCN.
//
// Mirrors include/gcn.cuh:40-122 and include/optim.cuh:16-50 of the reference (and
// hpdga-spring23/include/gcn.h, optim.h): same parameter structs and defaults, the same
// L-layer builders (insert_first_layer / insert_layer / insert_last_layer,
// src/gcn.cu:47-142), the same module and variable order, train_epoch / eval / run.
// Numerics follow the sequential CPU reference (hpdga-spring23), not the CUDA one: CPU
// xorshift128+ dropout masks and glorot init, loss normalised by the labelled count.
#pragma once
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "comm.hpp"
#include "data.hpp"
#include "graph.hpp"
#include "module.hpp"
#include "runtime.hpp"

namespace pgcn {

// GraphSum row chunks of the edge-cut engine at world > 1 (knob rs_chunks): chunk k's
// reduce-scatter overlaps chunk k+1's local sum.  1 by default (r04, reddit-114M, one rank's
// GraphSum timed on one GPU: 58.7 us at world 8 for the whole column block against 81.3 us
// for two row chunks, whose 30 rowset batches leave half the CUs idle; a 13 MB exchange at
// 300 GB/s then fits in the 22.6 us the second chunk would have hidden, and above that rate
// one chunk is ahead; profiles/r04/rank_graphsum_c1.json, rank_graphsum_c2.json)

struct GCNParams {
  int num_nodes = 0, input_dim = 0, output_dim = 0;
  std::vector<int> hidden_dims = {16};
  std::vector<float> dropouts = {0.5f, 0.5f};
  int epochs = 100, early_stopping = 0;
  int n_layers = 2;
  // compute the last layer as (Â H) W instead of Â (H W) when that narrows the GraphSum
  // (hidden < classes); exact algebra, fp32 rounding order only (see insert_last_layer)
  bool reassociate_last = false;
  unsigned seed = 0;  // PART2 `seed`: 0 = hpdga's unseeded rand(), else srand(seed)
  // middle layers whose width equals the layer before get a ResidualConnection after their
  // ReLU: H_l = relu(Â (A_{l-1} W_l)) + A_{l-1} (insert_layer)
  bool residual = false;
  // every hidden layer gets a LayerNorm between its GraphSum and its ReLU (LayerNorm,
  // module.hpp); its scale / shift tensor is one more weight (no decay) behind the layers'
  bool layer_norm = false;
  // multi-label classification: GCNData::label_bits targets, BCEWithLogitsLoss as the last
  // module (the output Matmul unfused), count = labelled rows x classes
  bool multilabel = false;
  // every layer's GraphSum is a GraphAttention (module.hpp) on the pattern as loaded; its
  // attention vectors are one more weight (no decay), the last of all.  Single GPU, widths <= 128
  bool attention = false;
  // ... its hidden layers with this many heads concatenated inside their widths (the output
  // layer keeps one), and dropout on every attention layer's normalised weights (p > 0: one
  // DropoutRng per layer behind the Dropout modules' in the epoch's draws, init_dropout_rng)
  int attention_heads = 1;
  float attention_dropout = 0.0f;
  // GraphSAGE: every layer's GraphSum is a SageAggregate (module.hpp) on the pattern as loaded,
  // 1 = the mean over a row's slots (GraphSum kernels on 1 / len values), 2 = the element-wise
  // max (k_sage.hip); with root_weight every W_l is [d_in][2 d_l] and the layer's own row enters
  // through the first d_l columns of H W_l.  Single GPU, widths <= 128
  int aggregator = 0;
  bool root_weight = false;
  // graph classification: 1 sum, 2 mean, 3 max -- a Readout module (module.hpp) between the
  // output layer's node logits and the loss, which then runs over GCNData::num_graphs rows with
  // the graphs' labels and splits.  Single GPU, not with multilabel
  int readout = 0;
  // link prediction: 1 dot product -- a LinkDecoder module (module.hpp) between the output
  // layer's node embedding and a one-class BCEWithLogitsLoss over GCNData's pairs with their
  // labels and splits.  Single GPU, not with multilabel or readout
  int link_decoder = 0;
};

struct AdamParams {
  float learning_rate = 0.01f, beta1 = 0.9f, beta2 = 0.999f, eps = 1e-8f, weight_decay = 5e-4f;
};

// include/optim.cuh:23-50; hpdga optim.cpp:5-35.  Weight decay on W1 only
// (src/gcn.cu:157-158, hpdga gcn.cpp:127).
class Adam {
  struct Var {
    shared_ptr<Variable> w;
    DeviceBuffer<float> m, v;
    bool decay;
  };
  std::vector<Var> vars;
  AdamParams params;
  int step_count = 0;

 public:
  Adam() = default;
  Adam(const std::vector<shared_ptr<Variable>> &weights, const std::vector<bool> &decays,
       const AdamParams &p);
  // defer (one GPU): the weight gradients' deferred last reduction passes (tn_defer), run by
  // this launch for the tensors whose gradients they write, launched before it otherwise
  // peer (edge-cut, processes): the gradients' all-reduce left its sum to this launch --
  // tensor t's gradient is the rank-order sum of peer's slots at its offset in `arena`
  // draws (mask_adam, one GPU): the next training forward's masks drawn by the same launch
  void step(const Stream &s, TnDeferList *defer = nullptr, const PeerRecv *peer = nullptr,
            const float *arena = nullptr, const MaskDraw *draws = nullptr, int n_draws = 0,
            const void *table = nullptr);
  // the reference's per-tensor schedule (src/optim.cu:57-95): one step, tensor i on
  // streams[i], then events[i] recorded there (null: none); the same arithmetic as step()
  void step_each(const std::vector<hipStream_t> &streams, const std::vector<hipEvent_t> &events);
  size_t size() const { return vars.size(); }
  // epoch graphs: the same launches reading the step size from table[ctr[0] % cap] on the
  // device (the host counts the step with advance() at every replay)
  void step_graph(const Stream &s, const float *table, const int *ctr, int cap,
                  TnDeferList *defer = nullptr, const PeerRecv *peer = nullptr,
                  const float *arena = nullptr) const;
  void advance() { step_count++; }
  int steps() const { return step_count; }
  // the moments of every tensor in order, appended to m / v (checkpoints)
  void moments_to_host(std::vector<float> *m, std::vector<float> *v) const;
  // the moments from host arrays laid out as moments_to_host writes them (null: zero) and
  // the step count; the caller has synchronised the engine's streams
  void restore(const float *m, const float *v, int steps);
  float step_size(int t) const;  // hpdga optim.cpp:24, step t (1-based)

 private:
  void launch(const Stream &s, float st, const float *table, const int *ctr, int cap,
              TnDeferList *defer, const PeerRecv *peer, const float *arena,
              const MaskDraw *draws = nullptr, int n_draws = 0,
              const void *jump_table = nullptr) const;
};

struct DistSpec {
  int rank = 0, world = 1;
  const void *unique_id = nullptr;  // 128 bytes (RCCL)
  // in-process ranks on one device (PeerComm over raw pointers); world = group->world()
  std::shared_ptr<LoopbackGroup> loopback;
  // one process per GPU over peer-mapped slots (PeerComm over hipIpc handles, exchanged by
  // this host all-gather) instead of RCCL
  PeerComm::AllGather allgather;
  bool solo = false;  // timing only: PeerComm with no peers (every push lands in this rank)
};

class GCN {
 public:
  GCN(const GCNParams &params, const AdamParams &adam, const GCNData &data, int device,
      const DistSpec *dist = nullptr);
  ~GCN();
  std::pair<float, float> train_epoch();
  std::pair<float, float> eval(int split);
  void epoch_async();  // train_epoch + eval(2) without a host sync
  void sync();
  std::vector<float> results(int n);  // last n epochs x {tl, ta, vl, va}
  void run(bool verbose);

  int num_vars() const { return (int)variables.size(); }
  std::vector<float> get_var(int idx, int which);
  // weights only, get_var's layout; drops what was computed ahead from the old weights
  void set_var(int idx, int which, const float *host_src, long long count);
  // whole training state to / from one file (host/checkpoint.hpp); load flags: PGCN_LOAD_*
  void save(const std::string &path);
  void load(const std::string &path, int flags);
  // eval-mode forward over every row of this rank (no split, no row restriction), then
  // k_predict_rows; host outputs, any may be null; the training state is left as it was
  long long predict(int *cls, float *conf, float *probs);
  // predict + k_confusion against `split`'s labels: counts[c * c] of this rank's rows
  void confusion(int split, long long *counts);
  // multi-label engines: predict()'s forward, then k_predict_multilabel: bits [rows][words],
  // probs [rows][C] dense (either may be null); and k_multilabel_counts against `split`'s
  // labels: counts [3][C] = tp, fp, fn of this rank's rows
  long long predict_multilabel(uint32_t *bits, float *probs);
  void multilabel_counts(int split, long long *counts);
  // link engines: predict()'s forward, then the pairs' scores and sigmoids (either may be null);
  // k_multilabel_counts with one class against `split`'s labelled pairs: counts[3] = tp, fp, fn;
  // and the same forward followed by launch_link_score_fwd over m caller-given pairs
  long long predict_links(float *scores, float *probs);
  void link_counts(int split, long long *counts);
  void score_pairs(const int *src, const int *dst, long long m, float *scores);
  // the same forward, then launch_link_rank over `split`'s positive pairs in pair order (side 0:
  // the destination is ranked among all nodes, side 1: the source; filtered: build_rank_filter's
  // lists): their number, and with outputs their greater / equal counts.  Both outputs null: the
  // number only, nothing runs.  The query set of a (split, side, filtered) is built once
  long long link_ranks(int split, int side, int filtered, long long *greater, long long *equal);
  // the same forward, then launch_link_topk over the output embedding for m anchor nodes: idx /
  // score [m][k] on the host (side, filtered: build_topk_filter's lists).  kTopKChunk queries at a
  // time, the query set and the device outputs of a chunk freed after it
  void top_links(const int *nodes, long long m, int k, int side, int filtered, int *idx,
                 float *score);
  long long adam_steps() const { return optimizer.steps(); }
  void set_profile(bool on);
  void profile_read_mm(double *ms, long long *calls, double *flops);  // XW contractions
  void profile_read(double *ms, long long *calls, double *bytes);
  const Partition &partition() const { return part; }
  const GCNParams &get_params() const { return params; }
  // the knobs this engine and its graphs were built with (pgcn_debug_set changes nothing here)
  const Knobs &knobs() const { return knobs_; }
  const Comm *communicator() const { return comm.get(); }
  bool symmetric() const { return graph_symmetric; }
  long long epochs_run() const { return epoch_count; }
  // device time of the Â X precompute at build (eval_ax; 0 when off)
  float eval_ax_build_ms() const { return ax_build_ms; }
  // GraphSum calls of width 16 take the LDS-staged kernel (large tables)
  bool graphsum_lds() const;
  // the output layer runs as (Â H) W (reassociate_last requested, hidden < classes, Â symmetric)
  bool reassociated() const { return reassociated_; }
  int fused_tails() const { return fused_tails_; }
  int residual_layers() const { return (int)residuals_.size(); }
  // ... of which the last training forward ran inside a GraphSum's final write
  int fused_residuals() const;
  int norm_layers() const { return (int)norms_.size(); }
  int attention_layers() const { return attn_var ? L : 0; }
  // the heads of its hidden layers, and the layers that drop attention weights in training
  int attention_heads() const { return attn_var ? params.attention_heads : 1; }
  int attention_dropout_layers() const { return (int)attn_rngs.size(); }
  int aggregator() const { return params.aggregator; }
  int num_graphs() const { return num_graphs_; }
  long long num_pairs() const { return num_pairs_; }
  bool root_weight() const { return params.root_weight; }
  // ... of which the last training forward ran its ReLU / add / Dropout tail in the LayerNorm kernel
  int fused_norm_tails() const;
  // diagnostics (syncs): non-zero elements in the edge-cut padding rows of the variables the
  // LayerNorms write (a normalised zero row would be beta: they process this rank's rows only)
  long long norm_padding_nonzero();

 private:
  void build(const GCNData &data);
  void upload_features(const GCNData &data);
  void init_dropout_rng(const GCNData &data, long long glorot_draws);
  void insert_first_layer();
  void insert_layer(int in_dim, int out_dim, float dropout, int layer);
  void insert_last_layer();
  void fuse_epilogues();
  void fuse_matmul_tails();
  void fuse_output_layer();
  void prepare_graphs();
  void check_comm() const;
  void build_eval_ax();
  struct FoldScope;
  void backward_pass(FoldScope &fold, TnDeferList *defer);
  PeerRecv adam_peer;  // the pass's gradient all-reduce left its sum to Adam (world > 0)
  // mask_adam: the next training forward's input (and co-drawn hidden) masks for the Adam
  // launch; returns how many (0: not applicable, or drawn already)
  int mask_with_adam(MaskDraw out[2]);
  // mask_xstream: the next training forward's masks drawn by eval's first-layer product
  bool mask_in_eval() const;
  void join_side();
  std::vector<const ResidualConnection *> residuals_;
  std::vector<const LayerNorm *> norms_;
  // layer_norm: per hidden layer gamma_l[d_l] then beta_l[d_l], one tensor (one optimizer entry:
  // the one-batch Adam paths take at most kAdamBatch tensors), the last of `weights` and of
  // `variables`; null without layer_norm
  shared_ptr<Variable> norm_var;
  void insert_layer_norm(const shared_ptr<Variable> &var2, int layer);
  // attention: per layer a_dst_l[d_l] then a_src_l[d_l] (d_l the layer's output width), one
  // tensor, the last of `weights` and of `variables` (behind norm_var); null without attention
  shared_ptr<Variable> attn_var;
  // aggregator 1: the mean graphs every SageAggregate sums over (pgcn_graph_create_mean's two)
  std::unique_ptr<DevGraph> mean_fwd_graph, mean_bwd_graph;
  // layer l's weight has this many columns: 2 d_l under root_weight
  int weight_cols(int d) const { return params.root_weight ? 2 * d : d; }
  // an engine whose aggregation is not a GraphSum module: no reassociated output layer, no Â X
  // precompute, no output-row restriction, the loss unfused
  bool custom_aggregation() const { return params.attention || params.aggregator != 0; }
  // readout, link_decoder: every node row carries gradient, so nothing may rely on only a split's labelled rows
  // mattering -- no reassociated output layer, no output-row restriction or compact buffers, no
  // column-subset backward, the loss unfused
  bool all_rows_matter() const {
    return custom_aggregation() || params.readout != 0 || params.link_decoder != 0;
  }
  // readout: the graphs (0: none), their row ranges, and the pooled logits the loss reads
  int num_graphs_ = 0;
  std::vector<int> graph_ptr_host;
  shared_ptr<Variable> pooled;
  // the rows the loss, predict() and confusion() run over: the graphs, or this rank's nodes
  int loss_rows() const { return head_rows() ? head_rows() : part.local_rows(); }
  int loss_prow() const { return head_rows() ? head_rows() : part.maxrows; }
  int head_rows() const { return params.readout ? num_graphs_ : num_pairs_; }
  // link_decoder: the pairs (0: none), their index on the device (its backward entries: the
  // training split's labelled pairs), the node embedding the decoder reads and its scores [E][4]
  int num_pairs_ = 0;
  std::unique_ptr<LinkIndexDev> links_;
  shared_ptr<Variable> link_embed, link_scores;
  // link_ranks: the pattern and the pairs on the host (src, dst, label, split), and per
  // (split, side, filtered) the query set on the device with its counts [2][queries]
  SparseIndex rank_graph_;
  std::vector<int> rank_pairs_[4];
  struct RankSet {
    std::unique_ptr<RankQueriesDev> q;
    DeviceBuffer<unsigned> counts;
  };
  std::map<int, RankSet> rank_sets_;
  // the layer's aggregation from var1 to var2: a GraphSum, a GraphAttention on attn_var or a
  // SageAggregate
  void insert_aggregation(const shared_ptr<Variable> &var1, const shared_ptr<Variable> &var2,
                          int dim, int layer, bool last);
  int fused_tails_ = 0;  // GraphSum epilogues carrying ReLU / Dropout work (forward + backward)
  void set_split(int split);
  // the eval forward of predict(): every row, no labels, no results slot; the logits stay in
  // the loss module's input variable
  void predict_forward();
  // every mask and product computed ahead of its use is dropped (masks: a load moved the RNG
  // stream; products: the weights changed), and the epoch graph's device counters re-sync
  void forget_ahead(bool masks);
  void reseed_dropout(long long draw_epochs);
  void finalize(int slot_offset, bool graph = false, hipStream_t s = nullptr);
  // the eval forward + finalize of ring slot offset `off` (eval_tail: its last GraphSum's
  // exchange and the output layer on side_stream, ModuleContext::tail_stream)
  void eval_forward(int off, bool graph);
  int tail_gs = -1;  // eval_tail: index in `modules` of the last GraphSum; -1 = off
  void enqueue_epoch(bool graph);
  bool graph_eligible() const;
  void capture_epoch();
  void drop_epoch_graph();

  const Knobs knobs_;
  GCNParams params;
  AdamParams adam_params;
  int device;
  int L;
  Partition part;
  std::unique_ptr<Comm> comm;
  Stream stream;
  Stream comm_stream;  // edge-cut: reduce-scatters run here, overlapping the next chunk's sum
  Stream side_stream;  // the next epoch's input-dropout mask, beside the weight-gradient pass
  ModuleContext ctx;

  std::unique_ptr<DevGraph> graph;                    // one GPU: the whole Â
  std::vector<std::unique_ptr<DevGraph>> chunk_graphs;  // edge-cut: Â's column block per RS chunk
  DevFeatures feats;
  DeviceBuffer<int> truth[4];  // [1..3] per split; [0] no labels at all (predict_forward)
  int counts[4] = {0, 0, 0, 0};
  // output-layer row restriction (set_split): per split, its labelled rows and Â on them
  std::vector<int> split_rows_host[4];
  std::vector<int> split_rows_global[4];  // edge-cut: the split's labelled global node ids
  DeviceBuffer<int> split_rows_dev[4];
  std::unique_ptr<DevGraph> split_graphs[4], split_colgraphs[4];
  // edge-cut: per split, per RS chunk, the chunk graph on the split's rows + their row ids
  std::vector<std::unique_ptr<DevGraph>> chunk_split_graphs[4];
  std::vector<DeviceBuffer<int>> chunk_split_rows[4];
  std::vector<std::unique_ptr<DevGraph>> chunk_col_graphs;  // training split's columns
  DeviceBuffer<int> truth_compact[4];                // the split's labels, compact row order
  // multilabel: this rank's rows of the label bit matrix ([maxrows][label_words]; the same for
  // every split: truth[s] selects the rows), and per split its labelled rows' words compacted
  DeviceBuffer<uint32_t> label_bits, label_bits_compact[4];
  int label_words = 0;
  // the loss's count of a split: its labelled rows (global), x classes on a multi-label engine
  int loss_count(int split) const {
    return params.multilabel ? counts[split] * params.output_dim : counts[split];
  }
  std::unique_ptr<Variable> compact_z, compact_out;  // compact output layer (ModuleContext)
  long long nnz_x_global = 0;
  // Â equals its transpose (csr_symmetric at build): the reassociated output layer's
  // W.grad = (Â H)^T dOut equals the reference's H^T Â dOut only then
  bool graph_symmetric = false;
  std::vector<int> feat_indptr_global;  // for the input dropout ranges

  std::vector<shared_ptr<Variable>> variables;
  std::vector<std::unique_ptr<Module>> modules;
  std::vector<shared_ptr<Variable>> weights;
  std::vector<bool> decays;
  std::vector<shared_ptr<DropoutRng>> rngs;  // [0] input, then one per hidden layer
  // attention_dropout > 0: one per attention layer (nnz * K_l weights), behind rngs in the epoch
  std::vector<shared_ptr<DropoutRng>> attn_rngs;
  // the heads of layer l's attention: the output layer keeps one
  int layer_heads(int l) const { return l == L - 1 ? 1 : params.attention_heads; }
  std::vector<const Dropout *> dropouts_;
  Adam optimizer;
  DeviceBuffer<float> tn_pool;  // tn_fold: the deferred reduction passes' inputs
  // fuse_finish: the loss kernel's arrival ticket, per-block partials and the pass descriptor
  DeviceBuffer<unsigned> fin_ticket;
  DeviceBuffer<float> fin_part4;
  DeviceBuffer<unsigned> fin_gticket;  // two-level finish: a ticket per 64-B line per group
  DeviceBuffer<float> fin_gpart4;
  int fin_blocks = 0;
  XentFinal fin_desc;
  void arm_finish(int dst_offset, bool graph);
  DeviceBuffer<float> grad_arena;  // all weight grads, one all-reduce
  DeviceBuffer<uint8_t> jump_table;
  DeviceBuffer<uint4> mask_lut;  // the nibble tables in global memory (mask_xstream)
  DeviceBuffer<float> gemm_ws, gemm_ws_side;
  DeviceBuffer<float> xent_partials, sums, results_ring;
  // edge-cut: per ring slot and pass, the all-reduced {loss sum, wrong, sum W1^2, count}; the
  // host composes loss and accuracy from them (compose_raw), so a pass needs no compose launch
  DeviceBuffer<float> raw_ring;
  void compose_raw(const float *raw4, float *out2) const;
  std::pair<float, float> read_slot(int off);
  PinnedBuffer<float> pinned;
  int ring_cap = 1024;
  long long epoch_count = 0;
  // training forwards since the build: the dropout stream stands at glorot_draws + draw_epochs
  // * draw_period (differs from the Adam step count after a weights-only load)
  long long draw_epochs = 0;
  long long glorot_draws = 0;
  unsigned long long draw_period = 0;
  // a loaded checkpoint's results rows: epochs [hist_end - rows, hist_end), served by results()
  // in place of the device ring (one GPU keeps composed rows there, edge-cut raw sums)
  std::vector<float> hist;
  long long hist_end = 0;
  // predict()'s device outputs (allocated at its first call)
  DeviceBuffer<int> pred_cls;
  DeviceBuffer<float> pred_conf, pred_probs;
  DeviceBuffer<unsigned> pred_counts;
  DeviceBuffer<uint32_t> pred_bits;
  bool last_forward_training = false;
  bool reassociated_ = false;
  float ax_build_ms = 0.0f;
  // the last forward ran the output layer over the split's rows only (split_rows): the
  // variables in restricted_vars hold stale rows
  bool out_restricted = false;
  std::vector<int> restricted_vars;

  // Per-epoch hipGraph: epoch_async() replays one captured
  // train_epoch + eval(2).  Everything that changes between epochs lives on the device:
  // the dropout RNG chunk states advance themselves, the Adam step size comes from a host-
  // computed table indexed by a device step counter, the results-ring slot from a device
  // epoch counter, both advanced by the epoch's last kernel.
  hipGraph_t epoch_graph = nullptr;
  hipGraphExec_t epoch_exec = nullptr;
  DeviceBuffer<int> dev_ctr;          // {Adam steps done, epochs done}
  DeviceBuffer<float> step_table;     // step sizes of steps table_block * cap + 1 ...
  static constexpr int kStepTable = 4096;
  long long table_block = -1;
  bool ctr_valid = false;             // dev_ctr equals the host counters
  bool warm = false;                  // one eager epoch_async ran (lazy buffers exist)

  std::vector<std::pair<Event, Event>> gs_events;
  std::vector<std::pair<Event, Event>> mm_events;
  std::vector<double> mm_flops;
  std::vector<double> gs_bytes;
};

}  // namespace pgcn
