// parallel-gcn_amd/csrc/host/module.hpp -- Variable and the Module family.
//
// Same classes, constructor shapes and forward/backward contract as the reference's
// include/variable.cuh:11-29 and include/module.cuh:21-161:
//   virtual void forward(bool training, const Stream &) const;
//   virtual void backward(const Stream &) const;
// Each module launches its HIP kernels asynchronously on the stream it is given; data
// stays on the device.  Differences from the reference, by design:
//   * the input features X are never rewritten: the input Dropout only produces the mask
//     bits that SparseMatmul applies on the fly (the reference mutates X in place and
//     restores it with set_input_kernel every pass, src/gcn.cu:181-200);
//   * dropout masks are the CPU reference's xorshift128+ masks, bit for bit;
//   * weight gradients are reduced deterministically (no float atomics);
//   * with an edge-cut communicator, GraphSum combines partial sums with an RCCL
//     reduce-scatter and weight grads are all-reduced by the optimizer.
#pragma once
#include <memory>
#include <vector>

#include "comm.hpp"
#include "graph.hpp"
#include "runtime.hpp"

namespace pgcn {

using std::shared_ptr;

// include/variable.cuh:11-29. Node-sized variables are [rows][ld] with ld = round_up(cols,4)
// (padding columns are kept zero); weights are dense [rows][cols].
class Variable {
 public:
  DeviceBuffer<float> dev_data, dev_grad;
  // ResidualConnection(prev, current) links its two variables (module.hpp, ResidualConnection):
  //   current->dev_grad_z: the ReLU backward on `current` writes its masked gradient here and
  //     leaves dev_grad -- the gradient of relu(Z) + prev -- as it is; the GraphSum backward
  //     that produced `current` reads dev_grad_z;
  //   prev->skip_from = current: the Matmul that writes prev.grad adds current.grad to it.
  DeviceBuffer<float> dev_grad_z;
  const Variable *skip_from = nullptr;
  int rows = 0, cols = 0, ld = 0;
  long long size = 0;  // logical rows * cols
  Variable(int rows_, int cols_, bool requires_grad, int ld_ = -1);
  Variable() = default;
  void zero(hipStream_t s) const { dev_data.zero_async(s); }
  void zero_grad(hipStream_t s) const {
    if (dev_grad) dev_grad.zero_async(s);
  }
  // logical (unpadded) copy to host, which: 0 data, 1 grad
  std::vector<float> to_host(int which) const;
};

// Input features on the device (the feature half of DevGCNData, src/gcn.cu:30-43).
struct DevFeatures {
  bool dense = false;
  int rows = 0, cols = 0;  // local rows, input_dim
  long long nnz = 0;
  // dense: [rows][ldx] fp32, CSR order == row-major order
  DeviceBuffer<float> x;
  int ldx = 0;
  // eval_ax: Â X ([rows][ldx], computed once at engine build; Â and X are constants), so
  // eval's first layer is (Â X) W1 -- one GEMM pass instead of X W1 and a GraphSum
  DeviceBuffer<float> ax;
  // dense + X-stream kernels: the input dropout's keep bits in the nibble layout
  // (k_mask_nibbles, [rows][16] words), rebuilt by every training forward
  DeviceBuffer<uint64_t> maskT;
  // dense + wide first layer (k_gemm_wide.hip, 33..128 outputs, F <= 1024): the same nibble
  // layout for the wide kernels' dropout bits, rebuilt by every training forward
  DeviceBuffer<uint64_t> maskW;
  // sparse: CSR (+ transposed index for the weight gradient)
  DeviceBuffer<int> indptr, indices, csc_ptr, csc_row, csc_pos;
  DeviceBuffer<int> csc_order;  // features by descending column length (weight-gradient order)
  DeviceBuffer<float> values;
  std::vector<float> host_values;  // for reporting the dropped input (API parity)
};

// Dropout mask + xorshift chunk states for one Dropout module on this rank.
struct DropoutRng {
  DeviceBuffer<uint64_t> states;  // 2 per chunk
  DeviceBuffer<uint64_t> mask;    // 1 word per chunk: the last training forward's mask
  DeviceBuffer<uint64_t> mask_ahead;  // the next one, when drawn ahead (input dropout)
  long long chunk_lo = 0, n_chunks = 0;
  // 64-draw mask words per stored state (k_dropout_mask's PER; one state per 128 draws;
  // "mask_per" knob)
  int per = 2;
  long long elem_begin = 0, elem_end = 0;  // global element range of this rank
  long long mask_base = 0;                 // bit of local element 0 in `mask`
};

class Module {
 public:
  virtual void forward(bool training, const Stream &s) const = 0;
  virtual void backward(const Stream &s) const = 0;
  virtual void set_num_samples(int) {}
  virtual int get_num_samples() const { return 0; }
  virtual ~Module() {}
};

class ReLU;
class GraphSum;
class Dropout;
class ResidualConnection;

// Shared per-GCN state the modules read (current split, comm, profiling, RNG table).
struct ModuleContext {
  // the owning engine's snapshot (GCN), or the process table itself (the C++ API's context)
  const Knobs *knobs = &process_knobs();
  // eval computes the next training forward's first product too (an engine's
  // knobs->train_ahead; off in the C++ API, whose caller decides what runs next)
  bool train_ahead = true;
  // (measured and removed, r01/r02: drawing the next input mask on a side stream beside the
  // weight-gradient pass, the eval forward's X-stream product or its output layer -- the RNG
  // kernel and the pass beside it slow each other down, DESIGN.md §3 "Streams")
  hipStream_t side_stream = nullptr;  // mm_side's stream
  // "eval_tail" (edge-cut, peer exchange between processes): the eval pass's last GraphSum
  // pushes, waits and sums on tail_stream (set by GCN for that call), and the output layer and
  // the loss follow there, beside the next epoch's mask draw and first-layer product on the
  // stream; tail_done is recorded after them, and the next GraphSum on the stream waits for it
  // (tail_pending) -- it reuses the partial buffer and the slots' parity
  hipStream_t tail_stream = nullptr;
  Event tail_fork, tail_done;
  bool tail_pending = false;
  bool tail_used = false;  // the GraphSum given tail_stream ran its exchange there
  // "mm_side": a Matmul's weight gradient (b.grad = a^T c.grad, needed only by the optimizer)
  // runs on side_stream beside the rest of the backward pass (the reference's S2/S3 streams,
  // src/module.cu:445-472); GCN joins it (side_join) before the all-reduce / optimizer
  bool mm_side = false;
  Event mm_fork, side_join;
  void *gemm_workspace_side = nullptr;
  bool side_pending = false;
  // output-layer row restriction (single GPU; the edge-cut engine uses chunk_split_graphs):
  // the last GraphSum's forward computes only the current split's labelled rows -- the only
  // rows the loss, the accuracy and (through the loss gradient, zero elsewhere) the weight
  // gradients depend on
  DevGraph *split_graph = nullptr;  // Â restricted to those rows (null: all rows)
  const int *split_rows = nullptr;  // their row ids (device)
  // ... and its backward: the loss gradient is zero outside those rows, so Â out.grad only
  // needs the edges into them (Â's columns of the split)
  DevGraph *split_colgraph = nullptr;
  // compact output layer (reassociated order + row restriction): the last GraphSum writes the
  // split's rows compactly ([compact_n][ld]) and the output Matmul and the loss work on those
  // rows only; compact_n = 0: all rows
  int compact_n = 0;
  const int *compact_truth = nullptr;  // the split's labels in compact row order
  Variable *compact_z = nullptr;       // last GraphSum output / Matmul input (+ grad)
  Variable *compact_out = nullptr;     // logits (+ grad)
  const int *truth = nullptr;  // current split's truth (device)
  // multi-label engines: the label bit matrix of this rank's rows ([rows][label_words]) and of
  // the current split's rows in compact order (beside compact_truth)
  const uint32_t *label_bits = nullptr, *compact_label_bits = nullptr;
  int label_words = 0;
  // labelled rows of the current split (global); multi-label: times the classes
  int count = 0;
  float *xent_partials = nullptr;
  int xent_blocks = 0;
  // one GPU ("fuse_finish"): the pass's scalars finished by the loss kernel's last block
  // (XentFinal); set by GCN for the pass being enqueued, fin_taken by the loss module that
  // passed it on (GCN::finalize then launches nothing)
  const XentFinal *fin = nullptr;
  bool fin_taken = false;
  Comm *comm = nullptr;        // null on one GPU
  hipStream_t comm_stream = nullptr;      // edge-cut: stream of the reduce-scatters
  int local_rows = 0;                     // edge-cut: this rank's rows (the rest is padding)
  std::vector<DevGraph *> chunk_graphs;   // edge-cut: Â column block per RS row chunk
  // edge-cut output-layer row restriction: per RS chunk, the chunk graph restricted to the
  // current split's labelled rows (padded chunk row ids in chunk_split_rows); empty: off
  std::vector<DevGraph *> chunk_split_graphs;
  std::vector<const int *> chunk_split_rows;
  // ... and its backward: per RS chunk, the chunk graph on the columns (local rows) of the
  // training split, where the loss gradient is non-zero; empty: off
  std::vector<DevGraph *> chunk_col_graphs;
  const void *jump_table = nullptr;  // M^period byte tables (device)
  // mask_xstream: the next training forward's masks, drawn by eval's first-layer product
  // (SparseMatmul, eval_ax) -- xs_draw for the ring NN kernel, xs_draw_md for a separate
  // launch when that product takes another kernel; n = 0: none pending
  XsDraw xs_draw;
  MaskDraw xs_draw_md[2];
  void *gemm_workspace = nullptr;
  size_t gemm_workspace_bytes = 0;
  // profiling of GraphSum calls
  bool profile = false;
  std::vector<std::pair<Event, Event>> *gs_events = nullptr;
  std::vector<double> *gs_bytes = nullptr;
  // ... and of the XW contractions on the MFMA kernels (dense X W, H W, their gradients)
  std::vector<std::pair<Event, Event>> *mm_events = nullptr;
  std::vector<double> *mm_flops = nullptr;
  std::vector<Event> *event_pool = nullptr;
};

// Builders shared by GCN and the public C++ API (host/gcn.cpp)
void build_dev_features(DevFeatures &feats, const int *fptr, const int *indices,
                        const float *values, int first, int rows, int F, bool dense, int hidden0);
void init_dropout_rng_range(DropoutRng &r, const uint64_t seed[2], unsigned long long offset,
                            long long elem_begin, long long elem_end, int mask_per);
void glorot_fill(std::vector<float> &w, int in_size, int out_size, uint64_t s[2]);

// include/module.cuh:33-43
class Dropout : public Module {
  shared_ptr<Variable> in;  // null for the input features
  shared_ptr<DropoutRng> rng;
  float p;
  ModuleContext *ctx;

 public:
  Dropout(shared_ptr<Variable> in_, float p_, shared_ptr<DropoutRng> rng_, ModuleContext *ctx_);
  void forward(bool training, const Stream &s) const override;
  void backward(const Stream &s) const override;
  float scale() const { return 1.0f / (1.0f - p); }
  const DropoutRng &state() const { return *rng; }
  // Draws the NEXT training forward's mask now (the xorshift stream position is the same
  // whenever it is drawn); that forward then uses it instead of drawing again.  With `ready`,
  // the draw runs on stream s and `ready` is recorded after it: users of the mask on another
  // stream wait for it (wait_ahead).
  void draw_ahead(hipStream_t s, const Event *ready = nullptr) const;
  // The same draw handed to another launch (the optimizer's, mask_adam): fills out[0] (and
  // out[1]: co_draw's next mask) and marks both drawn; returns how many (0: already drawn)
  int ahead_descs(MaskDraw out[2]) const;
  bool drawn_ahead() const { return ahead; }
  void wait_ahead(hipStream_t s) const;
  const uint64_t *mask_ahead() const { return rng->mask_ahead.get(); }
  // Fused into the GraphSum next to it (GraphSum::forward/backward apply this module's work in
  // their epilogue): the training forward's mask is drawn by draw_fused(), and the next
  // forward / backward call of this module is skipped.
  const Variable *variable() const { return in.get(); }
  void draw_fused(hipStream_t s) const;
  mutable bool skip_forward = false, skip_backward = false;
  // the input dropout's training draw also draws `co_draw`'s mask (one launch: the same stream
  // positions, so the same bits); that module's next forward / fused draw then uses it
  // (GCN::build, "co_draw"; sparse X only: the dense input has its own layouts)
  const Dropout *co_draw = nullptr;
  mutable bool pre_drawn = false;
  // a checkpoint load moved the RNG stream (GCN::load): any mask drawn ahead or with another
  // module's draw came from the old position and is dropped
  void forget_draws() const {
    ahead = false;
    ahead_ready = nullptr;
    pre_drawn = false;
  }

 private:
  void draw(hipStream_t s, uint64_t *mask, int max_blocks = 0) const;
  mutable bool ahead = false;
  mutable const Event *ahead_ready = nullptr;  // recorded after an ahead draw on a side stream
};

// include/module.cuh:47-68: c = drop(X) * W
class SparseMatmul : public Module {
  const DevFeatures *x;
  shared_ptr<Variable> b, c;
  const Dropout *drop;  // the input Dropout (its mask, when training)
  ModuleContext *ctx;
  mutable bool last_training = false;
  // train-ahead (dense X-stream path): an eval forward also computes the next training
  // forward's drop(X) W into `ahead` (same weights: no optimizer step between them), which
  // that forward then swaps in instead of streaming X again
  mutable DeviceBuffer<float> ahead;
  mutable bool ahead_valid = false;

 public:
  SparseMatmul(const DevFeatures *x_, shared_ptr<Variable> b_, shared_ptr<Variable> c_,
               const Dropout *drop_, ModuleContext *ctx_);
  // eval_ax: the first GraphSum's output, written by an eval forward from Â X
  shared_ptr<Variable> eval_out;
  // the GraphSum reading c (training) / standing for eval_out (eval): the X-stream product's
  // epilogue writes that GraphSum's ring table (training) or applies its fused ReLU and
  // writes the next GraphSum's table (eval), when fuse_epilogue & kFuseXstream
  const GraphSum *consumer = nullptr;
  void forward(bool training, const Stream &s) const override;
  void backward(const Stream &s) const override;
  // the weights changed outside an optimizer step (GCN::set_var / load): a product computed
  // ahead from the old ones is dropped
  void forget_ahead() const { ahead_valid = false; }
};

// include/module.cuh:72-86
class GraphSum : public Module {
  shared_ptr<Variable> in, out;
  DevGraph *graph;
  int dim;
  ModuleContext *ctx;
  bool last_layer;                   // the output layer's GraphSum (row restriction applies)
 public:
  bool first_layer = false;          // eval_ax: its eval forward was done by SparseMatmul
 private:
  mutable DeviceBuffer<float> compact;  // restricted forward: [split rows][out->ld]
  // edge-cut: per row chunk, the [world*chunk_rows][ld] partial sums and their events
  std::vector<DeviceBuffer<float>> partial;
  std::vector<Event> computed;
  Event reduced;

 public:
  GraphSum(shared_ptr<Variable> in_, shared_ptr<Variable> out_, DevGraph *graph_, int dim_,
           ModuleContext *ctx_, bool last_layer_ = false);
  void forward(bool training, const Stream &s) const override;
  void backward(const Stream &s) const override;
  const Variable *input() const { return in.get(); }
  const Variable *output() const { return out.get(); }
  int width() const { return dim; }
  // Element-wise tails fused into this GraphSum's final writes (GCN::fuse_epilogues; null: the
  // modules run on their own): forward, the ReLU (and Dropout) on `out` that follow it;
  // backward, the Dropout (and ReLU) on `in` whose backward follows it
  ReLU *fwd_relu = nullptr;
  const ResidualConnection *fwd_res = nullptr;  // between that ReLU and that Dropout
  const Dropout *fwd_drop = nullptr;
  ReLU *bwd_relu = nullptr;
  const Dropout *bwd_drop = nullptr;
  // ... and the GraphSum that reads this one's fused output next (forward: `out`; backward:
  // in.grad): the epilogue also writes its prescaled input table (ring schedule), so that
  // GraphSum skips its prescale launch (prestaged_*, consumed by its next call)
  GraphSum *fwd_next = nullptr, *bwd_next = nullptr;
  mutable bool prestaged_fwd = false, prestaged_bwd = false;
  // the graph this module's next forward / backward sums over (single GPU)
  DevGraph *forward_graph() const;
  DevGraph *backward_graph() const;
  // ... and the graph whose prescaled table that call reads (edge-cut: row chunk 0's)
  DevGraph *forward_table_graph() const;
  DevGraph *backward_table_graph() const;
  // for a producer of this GraphSum's next forward input with `rows` rows and 16 columns:
  // the ring table (and its scale) that call reads, marked as written by the producer
  // (prestaged_fwd); null when that call has none
  float4 *claim_forward_table(int rows, int ld, const float **scale) const;
  // for the fused loss kernel writing this GraphSum's next backward input (out.grad, `rows` x
  // 16, ld 16): that call's ring table, scale and row map (XentTable), marked as written by
  // it (prestaged_bwd); false when that call has none (single GPU only)
  bool claim_backward_table(int rows, int ld, XentTable *t) const;

 private:
  // mode (edge-cut output layer): 0 all rows, 1 forward over ctx->chunk_split_graphs (the
  // split's rows), 2 backward over ctx->chunk_col_graphs (the split's columns)
  void run(const float *src, float *dst, const Stream &s, int mode = 0,
           const GsEpilogue *epi = nullptr, bool prestaged = false) const;
  // points the epilogue's next_table at `next`'s input table on graph `ng`, if it has one
  void stage_next(GsEpilogue &e, GraphSum *next, DevGraph *ng, bool fwd) const;
  // the fused tails of this call (mode 0 when none applies)
  bool tail_ok(const DevGraph *g, int ld_in, int ld_out) const;
  GsEpilogue forward_epilogue(bool training, const Stream &s, const DevGraph *g) const;
  GsEpilogue backward_epilogue(const DevGraph *g) const;
  // where this call's backward writes in.grad: in.dev_grad_z when the fused tail masks it for a
  // residual layer's ReLU (the epilogue stores the unmasked gradient to in.dev_grad: GsEpilogue::res)
  float *backward_dst(const GsEpilogue &e) const;
};

// Graph attention in GraphSum's place (the reference has none; k_gat.hip): out = sum over row
// i's slots of alpha_s in_j with alpha the row softmax of leaky(in_i . a_dst + in_j . a_src), on
// the adjacency pattern as loaded (the Â coefficients are not used).  a_dst [dim] then a_src [dim]
// sit at `offset` of the engine's one attention tensor `attn`; their gradients at the same offset
// of its grad.  A training forward keeps alpha for the backward, which reads out->dev_grad_z when
// that buffer exists (a residual layer), else out->dev_grad, and writes in->dev_grad.  Single GPU
// only.  It owns u, v, alpha, the backward's workspace (dx per slot, du, dv, partials) and a copy
// of Z as the training forward wrote it: the modules behind it (LayerNorm, ReLU, the residual add,
// Dropout, the loss's max shift) rewrite `out` in place, and the backward needs G_i . Z_i.
// `heads` heads are concatenated inside dim (head h: columns [h dim / heads, ...), its slice of
// a_dst / a_src; u, v [n][heads], alpha [nnz][heads]).  With `rng` (attention dropout p > 0; its
// range is the nnz * heads weights, element s * heads + h) a training forward draws the layer's
// mask itself, one launch on its own stream right before its kernels -- never ahead, never with
// another module's draw -- and the forward and the backward apply it with scale 1 / (1 - p);
// alpha keeps the weights before dropout.  heads == 1 without rng: the single-head kernels.
class GraphAttention : public Module {
  shared_ptr<Variable> in, out, attn;
  DevGraph *graph;
  int dim;
  long long offset;
  int heads;
  float p;
  shared_ptr<DropoutRng> rng;
  ModuleContext *ctx;
  DeviceBuffer<float> u, v, alpha, ws, z;

 public:
  static constexpr float kSlope = 0.2f;
  GraphAttention(shared_ptr<Variable> in_, shared_ptr<Variable> out_, DevGraph *graph_, int dim_,
                 shared_ptr<Variable> attn_, long long offset_, int heads_ = 1, float p_ = 0.0f,
                 shared_ptr<DropoutRng> rng_ = nullptr, ModuleContext *ctx_ = nullptr);
  void forward(bool training, const Stream &s) const override;
  void backward(const Stream &s) const override;
  const Variable *input() const { return in.get(); }
  const Variable *output() const { return out.get(); }
  int width() const { return dim; }
  int head_count() const { return heads; }
  const DropoutRng *mask_state() const { return rng.get(); }
  float scale() const { return 1.0f / (1.0f - p); }
};

// GraphSAGE aggregation in GraphSum's place (the reference has none).  `in` is the layer's H W:
// [rows][dim] (no root weight: Q = in) or [rows][2 dim] (root weight: R = in[:, 0:dim], Q =
// in[:, dim:2 dim]); out_i = R_i + aggr over row i's slots of Q_j on the pattern as loaded.
//   mean (aggregator 1): `mean_fwd` / `mean_bwd` are the engine's two make_mean_graph graphs;
//     the forward is mean_fwd's graphsum (whatever kernel DevGraph picks) and one strided add of
//     R, the backward mean_bwd's graphsum of out.grad.
//   max (aggregator 2): launch_agg_max_fwd adds R in its final write and a training forward
//     keeps the winning slots in `arg` (owned here) for launch_agg_max_bwd.
// The backward reads out->dev_grad_z when that buffer exists (a residual layer), else
// out->dev_grad, and writes in->dev_grad whole: dR = that gradient (one strided copy), dQ beside
// it.  When dim is no multiple of 4 (an output layer) the Q half of `in` does not start on the
// 16-byte grid: Q and dQ then pass through the staging buffers `q` / `dq` (one strided copy each
// way).  Single GPU only.
class SageAggregate : public Module {
  shared_ptr<Variable> in, out;
  DevGraph *graph, *mean_fwd, *mean_bwd;
  int dim, aggregator;
  bool root;
  DeviceBuffer<int> arg;
  DeviceBuffer<float> q, dq;
  int ld_s;  // the stride of arg, q and dq: round_up4(dim)
  bool staged() const { return root && dim % 4 != 0; }

 public:
  SageAggregate(shared_ptr<Variable> in_, shared_ptr<Variable> out_, DevGraph *graph_,
                DevGraph *mean_fwd_, DevGraph *mean_bwd_, int dim_, int aggregator_, bool root_);
  void forward(bool training, const Stream &s) const override;
  void backward(const Stream &s) const override;
};

// Graph-level readout behind the output layer (the reference has none): `in` [n][dim] holds the
// node logits of a batch of G graphs, graph g owning rows [graph_ptr[g], graph_ptr[g + 1]); out
// [G][dim] = their sum (mode 1), mean (2) or maximum (3) per graph (launch_readout_fwd: one launch
// unless a range is longer than kReadoutChunk).  A training forward of the max keeps the winning
// rows in `arg` (owned here).  The backward reads out->dev_grad -- the loss's gradient per graph --
// and writes every row of in->dev_grad (launch_readout_bwd).  It draws nothing from the dropout
// stream.  Single GPU only.
class Readout : public Module {
  shared_ptr<Variable> in, out;
  int n, G, dim, mode, max_len = 0;
  DeviceBuffer<int> graph_ptr, node_graph, arg;
  DeviceBuffer<float> ws;
  int ld_s;  // arg's stride: round_up4(dim)

 public:
  Readout(shared_ptr<Variable> in_, shared_ptr<Variable> out_, const std::vector<int> &graph_ptr_,
          int dim_, int mode_);
  const Variable *input() const { return in.get(); }
  const Variable *output() const { return out.get(); }
  int graphs() const { return G; }
  void forward(bool training, const Stream &s) const override;
  void backward(const Stream &s) const override;
};

// Link prediction's decoder behind the output layer (the reference has none): `in` [n][dim] is
// the node embedding, out [E][4] = {H[src_e] . H[dst_e], 0, 0, 0} per pair of `links`
// (launch_link_score_fwd, one launch).  The backward reads out->dev_grad -- the loss's gradient per
// pair in column 0 -- and writes every row of in->dev_grad (launch_link_score_bwd) over the pairs
// `links` selected for it.  No weights, nothing drawn from the dropout stream.  Single GPU only.
class LinkDecoder : public Module {
  shared_ptr<Variable> in, out;
  const LinkIndexDev *links;  // owned by the engine
  int dim;

 public:
  LinkDecoder(shared_ptr<Variable> in_, shared_ptr<Variable> out_, const LinkIndexDev *links_,
              int dim_);
  const Variable *input() const { return in.get(); }
  const Variable *output() const { return out.get(); }
  void forward(bool training, const Stream &s) const override;
  void backward(const Stream &s) const override;
};

// include/module.cuh:90-99
class ReLU : public Module {
  shared_ptr<Variable> in;
  DeviceBuffer<uint8_t> mask;

 public:
  explicit ReLU(shared_ptr<Variable> in_);
  void forward(bool training, const Stream &s) const override;
  void backward(const Stream &s) const override;
  const Variable *variable() const { return in.get(); }
  uint8_t *mask_ptr() const { return const_cast<uint8_t *>(mask.get()); }
  mutable bool skip_forward = false, skip_backward = false;  // done by a GraphSum epilogue
};

// include/module.cuh:149-161: current += prev, "works only if hidden dimension are the same".
// The reference's backward is empty (and its GCN never inserts the module); here the skip
// gradient prev.grad += current.grad is real.  Matmul::backward overwrites prev.grad after this
// module's place in the reverse order, so the add is made there (Variable::skip_from), from
// current.grad kept unmasked (Variable::dev_grad_z): this module's own backward launches nothing.
class ResidualConnection : public Module {
  shared_ptr<Variable> prev, cur;

 public:
  ResidualConnection(shared_ptr<Variable> prev_, shared_ptr<Variable> current_);
  ~ResidualConnection() override;
  void forward(bool training, const Stream &s) const override;
  void backward(const Stream &s) const override;
  const Variable *previous() const { return prev.get(); }
  const Variable *current() const { return cur.get(); }
  mutable bool skip_forward = false;  // done by a GraphSum epilogue
  mutable bool last_fused = false;    // ... in the last training forward
};

// LayerNorm over the columns of a hidden layer's var2, between its GraphSum and its ReLU (the
// reference has none): in = gamma * xhat + beta in place, over this rank's `rows` rows (edge-cut
// padding rows stay zero: a normalised zero row would be beta).  gamma [d] then beta [d] sit at
// `offset` of the engine's one scale / shift tensor `norm`; their gradients at the same offset of
// its grad.  A training forward keeps xhat and rstd for the backward, which transforms in place
// the buffer the layer's GraphSum backward reads (in.dev_grad, or dev_grad_z on a residual
// layer) after the Dropout / ReLU backward have run on it.
class LayerNorm : public Module {
  shared_ptr<Variable> in, norm;
  long long offset;
  int rows;
  DeviceBuffer<float> xhat, rstd, ws;

 public:
  static constexpr float kEps = 1e-5f;
  LayerNorm(shared_ptr<Variable> in_, shared_ptr<Variable> norm_, long long offset_, int rows_);
  void forward(bool training, const Stream &s) const override;
  void backward(const Stream &s) const override;
  const Variable *variable() const { return in.get(); }
  // The element-wise modules behind it, run in this kernel's final write (GCN::fuse_epilogues;
  // null: they run on their own) -- GraphSum's forward tail without the next table
  ReLU *fwd_relu = nullptr;
  const ResidualConnection *fwd_res = nullptr;
  const Dropout *fwd_drop = nullptr;
  mutable bool last_fused = false;  // the last training forward ran that tail
};

// include/module.cuh:103-124: c = a * b
class Matmul : public Module {
  shared_ptr<Variable> a, b, c;
  int m, n, p;
  ModuleContext *ctx;

 public:
  bool last_layer = false;  // the output layer's Matmul (compact rows apply)
  bool fused_forward = false;  // its forward runs inside the loss's (CrossEntropyLoss::fused)
  mutable bool input_grad_done = false;  // ... which also wrote a.grad (this training pass)
  mutable bool weight_grad_done = false;  // ... and b.grad
  // the Dropout (and ReLU) on `a` whose backward follows this one's: applied in the a.grad
  // product's final write when that product runs on k_xstream_nn (GCN::fuse_epilogues)
  const Dropout *bwd_drop = nullptr;
  ReLU *bwd_relu = nullptr;
  Matmul(shared_ptr<Variable> a_, shared_ptr<Variable> b_, shared_ptr<Variable> c_, int m_,
         int n_, int p_, ModuleContext *ctx_);
  const Variable *input() const { return a.get(); }
  const Variable *weight() const { return b.get(); }
  const Variable *output() const { return c.get(); }
  int inner() const { return n; }
  void forward(bool training, const Stream &s) const override;
  void backward(const Stream &s) const override;
  // the two halves of backward(), for callers that schedule them on their own streams (the
  // C++ API's reference schedule, src/module.cu:431-472): a.grad = c.grad b^T on s, and
  // b.grad = a^T c.grad on `ws` (a workspace of gemm_tn_workspace(m, p, n) bytes owned by the
  // caller when the stream is not the module's usual one)
  void backward_input(const Stream &s) const;
  void backward_weight(hipStream_t s, void *ws) const;

 private:
  void add_skip_grad(const Stream &s) const;
};

// include/module.cuh:128-145
class CrossEntropyLoss : public Module {
  shared_ptr<Variable> logits;
  int num_classes;
  ModuleContext *ctx;
  int num_samples = 0;

 public:
  CrossEntropyLoss(shared_ptr<Variable> logits_, int num_classes_, ModuleContext *ctx_);
  // the output layer's Matmul whose forward this loss computes with its own (null: none)
  const Matmul *fused = nullptr;
  // ... and the GraphSum whose backward reads that Matmul's input grad (the reassociated
  // output layer's): the fused kernel also writes its prescaled table (claim_backward_table)
  const GraphSum *dh_reader = nullptr;
  const Variable *input() const { return logits.get(); }
  void forward(bool training, const Stream &s) const override;
  void backward(const Stream &s) const override;
  void set_num_samples(int n) override { num_samples = n; }
  int get_num_samples() const override { return num_samples; }
};

// The multi-label loss in CrossEntropyLoss's place (the reference has none): per-class sigmoid
// with binary cross-entropy against ctx->label_bits on the rows with ctx->truth >= 0, mean over
// ctx->count = labelled rows x classes (k_bce_fwd).  Full rows or the compact output layer's, as
// the unfused branch of CrossEntropyLoss::forward; the logits are left as the Matmul / GraphSum
// wrote them.  It does not take ctx->fin: GCN::finalize launches k_reduce_scalars.
class BCEWithLogitsLoss : public Module {
  shared_ptr<Variable> logits;
  int num_classes;
  ModuleContext *ctx;
  int num_samples = 0;

 public:
  BCEWithLogitsLoss(shared_ptr<Variable> logits_, int num_classes_, ModuleContext *ctx_);
  const Variable *input() const { return logits.get(); }
  void forward(bool training, const Stream &s) const override;
  void backward(const Stream &s) const override;
  void set_num_samples(int n) override { num_samples = n; }
  int get_num_samples() const override { return num_samples; }
};

}  // namespace pgcn
