// parallel-gcn_amd/csrc/host/module.cpp
#include "module.hpp"

#include <algorithm>
#include <utility>

#include "../kernels.hpp"

namespace pgcn {

namespace {
// Profiling scope of one XW contraction (MFMA kernels): HIP events around the launches on
// the module's stream and the contraction's 2*M*N*K flops (ctx->profile only).
struct MmProfile {
  ModuleContext *ctx;
  hipStream_t s;
  double flops;
  Event e0, e1;
  MmProfile(ModuleContext *c, hipStream_t st, double f) : ctx(c), s(st), flops(f) {
    if (!on()) return;
    e0 = Event::create(true);
    e1 = Event::create(true);
    e0.record(s);
  }
  bool on() const { return ctx->profile && ctx->mm_events && flops > 0; }
  ~MmProfile() {
    if (!on()) return;
    e1.record(s);
    ctx->mm_events->emplace_back(e0, e1);
    ctx->mm_flops->push_back(flops);
  }
};
}  // namespace

Variable::Variable(int rows_, int cols_, bool requires_grad, int ld_)
    : rows(rows_), cols(cols_), ld(ld_ < 0 ? cols_ : ld_), size((long long)rows_ * cols_) {
  const size_t n = (size_t)rows * (size_t)ld;
  dev_data.allocate(n);
  dev_data.zero();
  if (requires_grad) {
    dev_grad.allocate(n);
    dev_grad.zero();
  }
}

std::vector<float> Variable::to_host(int which) const {
  const DeviceBuffer<float> &b = which ? dev_grad : dev_data;
  std::vector<float> out;
  if (!b) return out;
  std::vector<float> raw((size_t)rows * ld);
  b.download(raw.data(), raw.size());
  out.resize((size_t)rows * cols);
  for (int r = 0; r < rows; r++)
    for (int c = 0; c < cols; c++) out[(size_t)r * cols + c] = raw[(size_t)r * ld + c];
  return out;
}

// "defer_wgrad": up to this many loss blocks (cora 43, citeseer 52): pubmed_synth's 309 partials per weight
// element made the Adam launch's sum as long as the two launches it saved (7.73-7.74k vs
// 7.78-7.80k epochs/s, profiles/r06/s)
constexpr int kDeferWgradMaxBlocks = 128;

// ------------------------------------------------------------------------------------------
// Dropout (src/module.cu:6-99; hpdga module.cpp:196-228)
// ------------------------------------------------------------------------------------------
Dropout::Dropout(shared_ptr<Variable> in_, float p_, shared_ptr<DropoutRng> rng_,
                 ModuleContext *ctx_)
    : in(std::move(in_)), rng(std::move(rng_)), p(p_), ctx(ctx_) {}

void Dropout::draw(hipStream_t s, uint64_t *mask, int max_blocks) const {
  const DropoutRng &r = *rng;
  launch_dropout_mask(r.states.get(), r.n_chunks, 64 * r.chunk_lo, r.elem_end, p, mask,
                      ctx->jump_table, s, max_blocks, r.per);
}

void Dropout::draw_ahead(hipStream_t s, const Event *ready) const {
  PGCN_CHECK(!ahead && !in, PGCN_E_INVALID, "dropout: one mask ahead, input dropout only");
  // into its own buffer: `mask` stays the last training forward's (backward, get_var)
  if (!rng->mask_ahead) {
    rng->mask_ahead.allocate(rng->mask.size());
    rng->mask_ahead.zero();
  }
  if (co_draw && !ready && !co_draw->pre_drawn && !co_draw->ahead) {
    // with the hidden dropout's next mask (co_draw; the eval forward uses neither)
    const DropoutRng &r = *rng, &q = co_draw->state();
    const MaskDraw a{r.states.get(), r.n_chunks, 64 * r.chunk_lo, r.elem_end, p,
                     rng->mask_ahead.get(), r.per};
    const MaskDraw b{q.states.get(), q.n_chunks, 64 * q.chunk_lo, q.elem_end, co_draw->p,
                     q.mask.get(), q.per};
    launch_dropout_mask2(a, b, ctx->jump_table, s);
    co_draw->pre_drawn = true;
  } else {
    // on a side stream: two workgroups per CU, leaving room for the main stream's kernels
    draw(s, rng->mask_ahead.get(), ready ? 2 * kCUs : 0);
  }
  if (ready) ready->record(s);
  ahead_ready = ready;
  ahead = true;
}

int Dropout::ahead_descs(MaskDraw out[2]) const {
  PGCN_CHECK(!in, PGCN_E_INVALID, "dropout: one mask ahead, input dropout only");
  if (ahead) return 0;
  if (!rng->mask_ahead) {
    rng->mask_ahead.allocate(rng->mask.size());
    rng->mask_ahead.zero();
  }
  const DropoutRng &r = *rng;
  out[0] = MaskDraw{r.states.get(), r.n_chunks, 64 * r.chunk_lo, r.elem_end, p,
                    rng->mask_ahead.get(), r.per};
  int n = 1;
  if (co_draw && !co_draw->pre_drawn && !co_draw->ahead) {
    const DropoutRng &q = co_draw->state();
    out[1] = MaskDraw{q.states.get(), q.n_chunks, 64 * q.chunk_lo, q.elem_end, co_draw->p,
                      q.mask.get(), q.per};
    co_draw->pre_drawn = true;
    n = 2;
  }
  ahead_ready = nullptr;
  ahead = true;
  return n;
}

void Dropout::wait_ahead(hipStream_t s) const {
  if (ahead && ahead_ready) {
    ahead_ready->wait_on(s);
    ahead_ready = nullptr;
  }
}

void Dropout::draw_fused(hipStream_t s) const {
  PGCN_CHECK(in && !ahead, PGCN_E_INVALID, "dropout: fused draw of a hidden dropout only");
  if (pre_drawn)
    pre_drawn = false;
  else
    draw(s, rng->mask.get());
  skip_forward = true;
}

void Dropout::forward(bool training, const Stream &s) const {
  if (!training) return;  // hpdga module.cpp:209
  if (skip_forward) {  // drawn and applied by the GraphSum before it (epilogue)
    skip_forward = false;
    return;
  }
  const DropoutRng &r = *rng;
  if (ahead) {  // drawn ahead (during the last weight-gradient pass, or by the eval forward)
    wait_ahead(s.get());
    std::swap(rng->mask, rng->mask_ahead);
    ahead = false;
  } else if (pre_drawn) {  // drawn with the input dropout's mask (co_draw)
    pre_drawn = false;
  } else if (co_draw && !co_draw->pre_drawn && !co_draw->ahead) {
    const DropoutRng &q = co_draw->state();
    const MaskDraw a{r.states.get(), r.n_chunks, 64 * r.chunk_lo, r.elem_end, p, r.mask.get(),
                     r.per};
    const MaskDraw b{q.states.get(), q.n_chunks, 64 * q.chunk_lo, q.elem_end, co_draw->p,
                     q.mask.get(), q.per};
    launch_dropout_mask2(a, b, ctx->jump_table, s.get());
    co_draw->pre_drawn = true;
  } else {
    draw(s.get(), rng->mask.get());
  }
  if (in) {
    // a grad-carrying variable is dropped in place (module.cpp:215); its rows are the
    // first (elem_end - elem_begin) elements of the local variable
    launch_dropout_apply_based(in->dev_data.get(), r.elem_end - r.elem_begin, r.mask.get(),
                               r.mask_base, scale(), s.get());
  }
}

void Dropout::backward(const Stream &s) const {
  if (!in || !in->dev_grad) return;  // module.cpp:222: no mask => nothing to do
  if (skip_backward) {  // applied by the GraphSum backward before it (epilogue)
    skip_backward = false;
    return;
  }
  const DropoutRng &r = *rng;
  launch_dropout_apply_based(in->dev_grad.get(), r.elem_end - r.elem_begin, r.mask.get(),
                             r.mask_base, scale(), s.get());
}

// ------------------------------------------------------------------------------------------
// SparseMatmul (src/module.cu:104-163; hpdga module.cpp:49-72)
// ------------------------------------------------------------------------------------------
SparseMatmul::SparseMatmul(const DevFeatures *x_, shared_ptr<Variable> b_,
                           shared_ptr<Variable> c_, const Dropout *drop_, ModuleContext *ctx_)
    : x(x_), b(std::move(b_)), c(std::move(c_)), drop(drop_), ctx(ctx_) {}

// The X-stream ring kernels (xstream_ring_ok) read the dropout bitmap as it was drawn (XsMask);
// the register-streamed ones read the nibble layout k_mask_nibbles builds from it (x->maskT)
static bool xs_flat(const DevFeatures *x) { return xstream_ring_ok(x->cols, x->ldx); }

void SparseMatmul::forward(bool training, const Stream &s) const {
  last_training = training;
  const uint64_t *mask = training ? drop->state().mask.get() : nullptr;
  const long long base = drop->state().mask_base;
  const float scale = drop->scale();
  if (!training && x->ax && eval_out) {  // eval_ax: (Â X) W1 straight into the GraphSum's output
    if (xstream_ok(b->cols, x->cols)) {
      // eval: out = relu(Â X W1) (GraphSum, then its fused ReLU; the Dropout after it is the
      // identity in eval), which the reassociated output layer's GraphSum reads next
      XsEpilogue e;
      if ((ctx->knobs->fuse_epilogue & kFuseXstream) && consumer && consumer->fwd_relu) {
        e.relu = 1;
        consumer->fwd_relu->skip_forward = true;
        if (consumer->fwd_next)
          e.next_table =
              consumer->fwd_next->claim_forward_table(x->rows, eval_out->ld, &e.next_scale);
        e.next_sr = RING_SR;
      }
      // mask_xstream: the next training forward's masks drawn by extra waves of this product
      // (an unmasked pass on the ring kernel), else by their own launch below
      XsDraw dr;
      if (ctx->xs_draw.n > 0 && xstream_ring_ok(x->cols, x->ldx)) {
        dr = ctx->xs_draw;
        e.draw = &dr;
        ctx->xs_draw.n = 0;
      }
      launch_xstream_nn(x->rows, b->cols, x->cols, x->ax.get(), x->ldx, b->dev_data.get(), b->ld,
                        0, eval_out->dev_data.get(), eval_out->ld, nullptr, 1.0f, s.get(), nullptr,
                        &e);
    } else
      launch_gemm_nn(x->rows, b->cols, x->cols, x->ax.get(), x->ldx, b->dev_data.get(), b->ld, 0,
                     eval_out->dev_data.get(), eval_out->ld, nullptr, 0, 0, 1.0f, s.get());
    if (ctx->xs_draw.n > 0) {  // drawn ahead all the same: the forward expects them
      if (ctx->xs_draw.n == 2)
        launch_dropout_mask2(ctx->xs_draw_md[0], ctx->xs_draw_md[1], ctx->jump_table, s.get());
      else
        launch_dropout_mask(ctx->xs_draw_md[0].states, ctx->xs_draw_md[0].n_chunks,
                            ctx->xs_draw_md[0].elem0, ctx->xs_draw_md[0].elem_end,
                            ctx->xs_draw_md[0].p, ctx->xs_draw_md[0].mask, ctx->jump_table,
                            s.get(), 0, ctx->xs_draw_md[0].per);
      ctx->xs_draw.n = 0;
    }
    return;
  }
  if (training && ahead_valid) {  // computed by the eval forward before this one
    std::swap(c->dev_data, ahead);
    ahead_valid = false;
    return;
  }
  if (!training && ctx->train_ahead && !x->dense && ctx->knobs->sparse_dual && !ahead_valid) {
    // sparse X: eval's X W1 and the next training forward's drop(X) W1 from one pass over X
    // (k_spmm_csr<true>; the next input mask -- and its co-drawn hidden mask -- drawn now)
    if (!ahead) {
      ahead.allocate(c->dev_data.size());
      ahead.zero();
    }
    if (drop->drawn_ahead())
      drop->wait_ahead(s.get());
    else
      drop->draw_ahead(s.get());
    launch_spmm_csr_dual(x->rows, b->cols, c->ld, x->indptr.get(), x->indices.get(),
                         x->values.get(), drop->mask_ahead(), base, scale, b->dev_data.get(),
                         c->dev_data.get(), ahead.get(), s.get());
    ahead_valid = true;
    return;
  }
  if (!training && ctx->train_ahead && x->dense && x->maskT && !ahead_valid) {
    // eval forward + the next training forward's product, one pass over X (the next mask is
    // usually drawn already, on the side stream during the last weight-gradient pass)
    if (!ahead) {
      ahead.allocate(c->dev_data.size());
      ahead.zero();  // rows past x->rows (edge-cut padding) and padding columns stay zero
    }
    if (drop->drawn_ahead())
      drop->wait_ahead(s.get());
    else
      drop->draw_ahead(s.get());
    const uint64_t *m = drop->mask_ahead();
    const bool flat = xs_flat(x);
    const XsMask fm{m, base, x->cols, (long long)drop->state().mask.size()};  // (ahead: same size)
    if (!flat) launch_mask_nibbles(m, base, x->cols, x->rows, x->cols, x->maskT.get(), s.get());
    launch_xstream_nn(x->rows, b->cols, x->cols, x->x.get(), x->ldx, b->dev_data.get(), b->ld, 0,
                      c->dev_data.get(), c->ld, flat ? nullptr : x->maskT.get(), scale, s.get(),
                      ahead.get(), nullptr, flat ? &fm : nullptr);
    ahead_valid = true;
    return;
  }
  MmProfile prof(ctx, s.get(), x->dense ? 2.0 * x->rows * b->cols * x->cols : 0.0);
  if (x->dense && x->maskT) {  // X-stream kernels (N <= 16, K <= 640)
    const bool flat = mask && xs_flat(x);
    const XsMask fm{mask, base, x->cols, (long long)drop->state().mask.size()};
    if (mask && !flat)
      launch_mask_nibbles(mask, base, x->cols, x->rows, x->cols, x->maskT.get(), s.get());
    XsEpilogue e;  // the first GraphSum's prescaled input, written beside c
    if ((ctx->knobs->fuse_epilogue & kFuseXstream) && consumer && (training || !eval_out)) {
      e.next_table = consumer->claim_forward_table(x->rows, c->ld, &e.next_scale);
      e.next_sr = RING_SR;
    }
    launch_xstream_nn(x->rows, b->cols, x->cols, x->x.get(), x->ldx, b->dev_data.get(), b->ld, 0,
                      c->dev_data.get(), c->ld, mask && !flat ? x->maskT.get() : nullptr, scale,
                      s.get(), nullptr, &e, flat ? &fm : nullptr);
  } else if (x->dense) {
    // wide outputs: the mask in the nibble layout too (one pass over the bitmap; the wide
    // kernels then read one word per row and 4 steps, and the backward reuses it)
    const uint64_t *mw = mask && x->maskW ? x->maskW.get() : nullptr;
    if (mw)
      launch_mask_nibbles(mask, base, x->cols, x->rows, x->cols, x->maskW.get(), s.get());
    launch_gemm_nn(x->rows, b->cols, x->cols, x->x.get(), x->ldx, b->dev_data.get(), b->ld, 0,
                   c->dev_data.get(), c->ld, mask, base, x->cols, scale, s.get(), mw);
  } else {
    launch_spmm_csr(x->rows, b->cols, c->ld, x->indptr.get(), x->indices.get(), x->values.get(),
                    mask, base, scale, b->dev_data.get(), c->dev_data.get(), s.get());
  }
}

void SparseMatmul::backward(const Stream &s) const {
  // b.grad = drop(X)^T * c.grad  (the dropped X of the last training forward)
  const uint64_t *mask = last_training ? drop->state().mask.get() : nullptr;
  const long long base = drop->state().mask_base;
  const float scale = drop->scale();
  MmProfile prof(ctx, s.get(), x->dense ? 2.0 * x->rows * b->cols * x->cols : 0.0);
  if (x->dense && x->maskT) {  // the mask of the last training forward (flat or nibbles)
    const bool flat = mask && xs_flat(x);
    const XsMask fm{mask, base, x->cols, (long long)drop->state().mask.size()};
    launch_xstream_tn(x->rows, b->cols, x->cols, x->x.get(), x->ldx, c->dev_grad.get(), c->ld,
                      b->dev_grad.get(), b->ld, mask && !flat ? x->maskT.get() : nullptr, scale,
                      ctx->gemm_workspace, s.get(), flat ? &fm : nullptr);
  } else if (x->dense) {
    launch_gemm_tn(x->rows, b->cols, x->cols, x->x.get(), x->ldx, c->dev_grad.get(), c->ld,
                   b->dev_grad.get(), b->ld, mask, base, x->cols, scale, ctx->gemm_workspace,
                   s.get(), mask && x->maskW ? x->maskW.get() : nullptr);
  } else {
    launch_spmm_csc_bwd(x->cols, b->cols, c->ld, x->csc_ptr.get(), x->csc_row.get(),
                        x->csc_pos.get(), x->values.get(), mask, base, scale, c->dev_grad.get(),
                        b->dev_grad.get(), s.get(), x->nnz, x->csc_order.get(),
                        ctx->knobs->csc_tree != 0);
  }
}

// ------------------------------------------------------------------------------------------
// GraphSum (src/module.cu:168-210; hpdga module.cpp:82-111)
// ------------------------------------------------------------------------------------------
GraphSum::GraphSum(shared_ptr<Variable> in_, shared_ptr<Variable> out_, DevGraph *graph_,
                   int dim_, ModuleContext *ctx_, bool last_layer_)
    : in(std::move(in_)), out(std::move(out_)), graph(graph_), dim(dim_), ctx(ctx_),
      last_layer(last_layer_) {
  if (ctx->comm && ctx->comm->world() > 1) {  // (one rank sums straight into `out`)
    for (DevGraph *gk : ctx->chunk_graphs) {
      partial.emplace_back();
      partial.back().allocate((size_t)gk->rows() * out->ld);
      partial.back().zero();
      computed.push_back(Event::create());
    }
    reduced = Event::create();
  }
}

DevGraph *GraphSum::forward_graph() const {
  if (ctx->comm) return nullptr;
  return last_layer && ctx->split_graph ? ctx->split_graph : graph;
}

DevGraph *GraphSum::backward_graph() const {
  if (ctx->comm) return nullptr;
  return last_layer && ctx->split_colgraph ? ctx->split_colgraph : graph;
}

// the graph whose prescaled input table this module's next forward / backward reads first
// (edge-cut: row chunk 0's, which the other chunks share)
DevGraph *GraphSum::forward_table_graph() const {
  if (!ctx->comm) return forward_graph();
  if (last_layer && !ctx->chunk_split_graphs.empty()) return nullptr;
  return ctx->chunk_graphs.empty() ? nullptr : ctx->chunk_graphs[0];
}

DevGraph *GraphSum::backward_table_graph() const {
  if (!ctx->comm) return backward_graph();
  if (last_layer && !ctx->chunk_col_graphs.empty()) return ctx->chunk_col_graphs[0];
  return ctx->chunk_graphs.empty() ? nullptr : ctx->chunk_graphs[0];
}

float4 *GraphSum::claim_forward_table(int rows, int ld, const float **scale) const {
  DevGraph *g = forward_table_graph();
  if (!g || !(ctx->knobs->fuse_epilogue & kFusePrestage) || dim != 16 || in->ld != 16 ||
      ld != 16 || g->cols() != rows)
    return nullptr;
  float *t = g->ring_table(dim, scale);
  if (!t) return nullptr;
  prestaged_fwd = true;
  return reinterpret_cast<float4 *>(t);
}

bool GraphSum::claim_backward_table(int rows, int ld, XentTable *t) const {
  if (ctx->comm || !(ctx->knobs->fuse_epilogue & kFusePrestage) || dim != 16 || ld != 16 ||
      out->ld != 16 || out->rows != rows)
    return false;
  DevGraph *g = backward_graph();
  const float *sc = nullptr;
  const int *pos = nullptr;
  int pos_rows = 0;
  float *tab = g ? g->ring_table_mapped(dim, &sc, &pos, &pos_rows) : nullptr;
  if (!tab || pos_rows != rows) return false;
  t->table = tab;
  t->scale = sc;
  t->pos = pos;
  t->rows = pos_rows;
  prestaged_bwd = true;
  return true;
}

void GraphSum::stage_next(GsEpilogue &e, GraphSum *next, DevGraph *ng, bool fwd) const {
  if (!next || !ng || !(ctx->knobs->fuse_epilogue & kFusePrestage)) return;
  const float *sc = nullptr;
  float *t = ng->ring_table(next->dim, &sc);
  if (!t) return;
  e.next_table = reinterpret_cast<float4 *>(t);
  e.next_scale = sc;
  e.next_sr = RING_SR;
  (fwd ? next->prestaged_fwd : next->prestaged_bwd) = true;
}

// Where this GraphSum's fused tails can run: in the kernel that forms the final rows (one
// GPU: `g`'s combine), or (edge-cut) in k_gs_finish on this rank's rows once the
// reduce-scatter has summed them
bool GraphSum::tail_ok(const DevGraph *g, int ld_in, int ld_out) const {
  if (ctx->comm) {
    if (dim % 4 != 0 || ld_out % 4 != 0) return false;
    if (ctx->comm->world() > 1) return true;
    // one rank: run() hands the tail to the column block's own GraphSum (its combine)
    const DevGraph *cg = g ? g : (ctx->chunk_graphs.empty() ? nullptr : ctx->chunk_graphs[0]);
    return cg && cg->epilogue_ok(dim, ld_in, ld_out);
  }
  return g && g->epilogue_ok(dim, ld_in, ld_out);
}

// The fused forward tail: ReLU on `out` (its mask when training), then the hidden Dropout
// (training), both skipped as modules for this pass.  mode 0 when `g` cannot take an epilogue.
GsEpilogue GraphSum::forward_epilogue(bool training, const Stream &s, const DevGraph *g) const {
  GsEpilogue e;
  if (!fwd_relu || !tail_ok(g, in->ld, out->ld)) return e;
  e.mode = 1;
  e.relu_mask = training ? fwd_relu->mask_ptr() : nullptr;
  e.relu_ld = out->ld;
  if (training && fwd_drop) {
    fwd_drop->draw_fused(s.get());
    const DropoutRng &r = fwd_drop->state();
    e.drop_mask = r.mask.get();
    e.drop_base = r.mask_base;
    e.drop_cols = out->cols;
    e.drop_scale = fwd_drop->scale();
  }
  if (fwd_res) {  // ResidualConnection: out = relu(out) + prev, before the dropout and the table
    e.res = const_cast<float *>(fwd_res->previous()->dev_data.get());  // (read only)
    e.res_ld = fwd_res->previous()->ld;
    fwd_res->skip_forward = true;
  }
  fwd_relu->skip_forward = true;
  if (fwd_next) stage_next(e, fwd_next, fwd_next->forward_table_graph(), true);
  return e;
}

// The fused backward tail: the Dropout backward on in.grad (mask of the last training
// forward), then the ReLU backward, both skipped as modules for this pass.
GsEpilogue GraphSum::backward_epilogue(const DevGraph *g) const {
  GsEpilogue e;
  if (!bwd_relu || !tail_ok(g, out->ld, in->ld)) return e;
  e.mode = 2;
  e.relu_mask = bwd_relu->mask_ptr();
  e.relu_ld = in->ld;
  if (bwd_drop) {
    const DropoutRng &r = bwd_drop->state();
    e.drop_mask = r.mask.get();
    e.drop_base = r.mask_base;
    e.drop_cols = in->cols;
    e.drop_scale = bwd_drop->scale();
    bwd_drop->skip_backward = true;
  }
  bwd_relu->skip_backward = true;
  if (in->dev_grad_z) {  // residual layer: in.grad keeps the unmasked gradient
    e.res = in->dev_grad.get();
    e.res_ld = in->ld;
  }
  if (bwd_next) stage_next(e, bwd_next, bwd_next->backward_table_graph(), false);
  return e;
}

float *GraphSum::backward_dst(const GsEpilogue &e) const {
  return e.mode == 2 && e.res ? in->dev_grad_z.get() : in->dev_grad.get();
}

void GraphSum::run(const float *src, float *dst, const Stream &s, int mode,
                   const GsEpilogue *epi, bool prestaged) const {
  if (ctx->comm && !ctx->tail_stream) {
    // the last eval pass's tail (eval_tail) still reads the partial buffer and its slots: every
    // collective entry waits for it (Comm::enter; the weight-gradient all-reduce and the loss
    // pair's too)
    ctx->comm->enter(s.get());
    ctx->tail_pending = false;
  }
  Event e0, e1;
  if (ctx->profile) {
    e0 = Event::create(true);
    e1 = Event::create(true);
    e0.record(s.get());
  }
  double bytes = 0;
  const std::vector<DevGraph *> &cgs = mode == 2 ? ctx->chunk_col_graphs : ctx->chunk_graphs;
  if (ctx->comm && ctx->comm->world() == 1 && cgs.size() == 1 && mode != 1) {
    // one rank: its column block is all of Â and the reduce-scatter would be a copy -- the
    // block's sums are final, formed with the tail in the combine as on one GPU
    cgs[0]->graphsum(src, in->ld, dst, out->ld, dim, s.get(), false, epi, prestaged);
    bytes = cgs[0]->algorithmic_bytes(dim);
    if (ctx->profile) e1.record(s.get());
  } else if (ctx->comm && partial.empty()) {
    // one rank, the split's rows only (split_rows): their sums scattered straight into `out`
    // (the other rows keep their last values, as the partials' do at world > 1)
    DevGraph *sk = ctx->chunk_split_graphs[0];
    if (sk->rows() > 0) {
      const size_t need = (size_t)sk->rows() * out->ld;
      if (compact.size() < need) compact.allocate(need);
      sk->graphsum(src, in->ld, compact.get(), out->ld, dim, s.get());
      launch_scatter_rows(compact.get(), ctx->chunk_split_rows[0], sk->rows(), out->ld, dst,
                          s.get());
      bytes = sk->algorithmic_bytes(dim);
    }
    if (ctx->profile) e1.record(s.get());
  } else if (ctx->comm && mode != 1 && ctx->chunk_graphs.size() == 1 &&
             dynamic_cast<PeerComm *>(ctx->comm) && cgs[0]->uses_lds(dim)) {
    // Peer-mapped exchange (PeerComm, k_peer.hip): the ring sums of every padded row from this
    // rank's columns, combined over the column blocks and pushed straight into each owner's
    // receive slot of this rank (k_gs_lds_combine's push mode, over xGMI); then the wait for
    // every rank's push and one kernel that sums the W slots of this rank's rows in rank order
    // and applies the fused tail (k_gs_gather_finish).  No partial buffer, no reduce-scatter.
    auto *pc = static_cast<PeerComm *>(ctx->comm);
    DevGraph *gk = cgs[0];
    const int h = out->rows;  // padded rows per rank (one chunk)
    // eval_tail: this call's push, wait and sum on the tail stream (the eval pass's last
    // GraphSum); any other call first waits for the last tail (partial buffer, slot parity)
    hipStream_t ts = s.get();
    if (ctx->tail_stream && dim <= 16) {
      ts = ctx->tail_stream;
      ctx->tail_used = true;
    }
    PeerSink k = pc->sink(h, (size_t)out->ld);
    pc->note((size_t)h * out->ld * ctx->comm->world() * sizeof(float), 1.0);
    gk->graphsum(src, in->ld, nullptr, out->ld, dim, s.get(), false, nullptr, prestaged, false, &k,
                 ts != s.get() ? ts : nullptr, ctx->tail_fork.get());
    bytes = gk->algorithmic_bytes(dim);
    pc->wait(ts);
    launch_gs_gather_finish(dst, out->ld, ctx->local_rows, (dim + 3) / 4 * 4,
                            epi && epi->mode ? *epi : GsEpilogue{}, pc->recv(), ts);
    if (ctx->profile) e1.record(ts);
  } else if (ctx->comm) {
    // Per row chunk: partial sums of the chunk's (padded) rows from this rank's columns on
    // the compute stream, then its reduce-scatter on the comm stream, which hands every rank
    // its own rows of the chunk while the next chunk is summed.  The chunks share one
    // prescaled table of this rank's columns (DevGraph::share_tables): prescaled once, by
    // the producer's epilogue (prestaged) or by chunk 0's call.
    const size_t h = (size_t)out->rows / ctx->chunk_graphs.size();
    for (size_t k = 0; k < ctx->chunk_graphs.size(); k++) {
      if (mode == 1) {
        // only the split's rows of the chunk; the chunk's other partial rows keep their last
        // values (finite), which reach only rows the loss skips and whose loss gradient is 0
        DevGraph *sk = ctx->chunk_split_graphs[k];
        if (sk->rows() > 0) {
          const size_t need = (size_t)sk->rows() * out->ld;
          if (compact.size() < need) compact.allocate(need);
          sk->graphsum(src, in->ld, compact.get(), out->ld, dim, s.get());
          launch_scatter_rows(compact.get(), ctx->chunk_split_rows[k], sk->rows(), out->ld,
                              partial[k].get(), s.get());
          bytes += sk->algorithmic_bytes(dim);
        }
      } else {
        DevGraph *gk = cgs[k];
        const bool shared = k > 0 && gk->table_owner() == cgs[0] && gk->can_share_tables(dim, in->ld);
        gk->graphsum(src, in->ld, partial[k].get(), out->ld, dim, s.get(), false, nullptr,
                     k == 0 && prestaged, shared);
        bytes += gk->algorithmic_bytes(dim);
      }
      if (ctx->chunk_graphs.size() == 1) {
        // one chunk: nothing to overlap -- the reduce-scatter follows on the compute stream
        // (two cross-stream hand-offs per GraphSum cost ~10 us each on the rank epoch)
        ctx->comm->reduce_scatter_sum(partial[k].get(), dst, h * out->ld, s.get());
        continue;
      }
      computed[k].record(s.get());
      computed[k].wait_on(ctx->comm_stream);
      ctx->comm->reduce_scatter_sum(partial[k].get(), dst + k * h * out->ld, h * out->ld,
                                    ctx->comm_stream);
    }
    if (ctx->chunk_graphs.size() > 1) {
      reduced.record(ctx->comm_stream);
      reduced.wait_on(s.get());  // dst complete, partials free for the next call
    }
    // the fused tail on this rank's rows of the summed output (padding rows stay zero)
    if (epi && epi->mode) launch_gs_finish(dst, out->ld, ctx->local_rows, dim, *epi, s.get());
    if (ctx->profile) e1.record(s.get());
  } else {
    graph->graphsum(src, in->ld, dst, out->ld, dim, s.get(), false, epi, prestaged);
    bytes = graph->algorithmic_bytes(dim);
    if (ctx->profile) e1.record(s.get());
  }
  if (ctx->profile) {
    ctx->gs_events->emplace_back(e0, e1);
    ctx->gs_bytes->push_back(bytes);
  }
}

void GraphSum::forward(bool training, const Stream &s) const {
  const bool pre = prestaged_fwd;  // this call's input table was written by the producer
  prestaged_fwd = false;
  PGCN_CHECK(!pre || ((training || !first_layer) &&
                      !(last_layer && ctx->comm && !ctx->chunk_split_graphs.empty())),
             PGCN_E_INVALID, "graphsum: prestaged input on a path that does not read it");
  if (!training && first_layer) return;  // eval_ax: SparseMatmul wrote Â X W1 already
  if (last_layer && ctx->comm && !ctx->chunk_split_graphs.empty()) {
    run(in->dev_data.get(), out->dev_data.get(), s, 1);
    return;
  }
  DevGraph *sg = last_layer && !ctx->comm ? ctx->split_graph : nullptr;
  if (!sg) {
    const GsEpilogue epi = forward_epilogue(training, s, graph);
    run(in->dev_data.get(), out->dev_data.get(), s, 0, &epi, pre);
    return;
  }
  // output layer: only the split's labelled rows, summed compactly and scattered to their
  // rows; the other rows keep their last (finite) values, which meet only zero loss-gradient
  // rows in Matmul::backward and are skipped by the loss
  float *dst;
  if (ctx->compact_n) {  // the output Matmul and the loss read the compact rows themselves
    dst = ctx->compact_z->dev_data.get();
  } else {
    const size_t need = (size_t)std::max(sg->rows(), 1) * out->ld;
    if (compact.size() < need) compact.allocate(need);
    dst = compact.get();
  }
  Event e0, e1;
  if (ctx->profile) {
    e0 = Event::create(true);
    e1 = Event::create(true);
    e0.record(s.get());
  }
  sg->graphsum(in->dev_data.get(), in->ld, dst, out->ld, dim, s.get(), false, nullptr, pre);
  if (ctx->profile) {
    e1.record(s.get());
    ctx->gs_events->emplace_back(e0, e1);
    ctx->gs_bytes->push_back(sg->algorithmic_bytes(dim));
  }
  if (!ctx->compact_n)
    launch_scatter_rows(dst, ctx->split_rows, sg->rows(), out->ld, out->dev_data.get(), s.get());
}

void GraphSum::backward(const Stream &s) const {
  // the same gather on grads (Â symmetric): in.grad = Â out.grad (module.cpp:98-111)
  const bool pre = prestaged_bwd;  // out.grad's input table was written by its producer
  prestaged_bwd = false;
  if (last_layer && ctx->comm && !ctx->chunk_col_graphs.empty()) {
    // edge-cut: out.grad is zero outside the training split's rows, so each chunk graph keeps
    // only the edges from those columns (all rows stay: the partials are written whole)
    const GsEpilogue epi = backward_epilogue(ctx->chunk_col_graphs[0]);
    run(out->dev_grad.get(), backward_dst(epi), s, 2, &epi, pre);
    return;
  }
  DevGraph *cg = last_layer && !ctx->comm ? ctx->split_colgraph : nullptr;
  if (!cg) {
    const GsEpilogue epi = backward_epilogue(graph);
    // (a residual layer's out.grad stays unmasked: its ReLU backward wrote dev_grad_z)
    const float *src = out->dev_grad_z ? out->dev_grad_z.get() : out->dev_grad.get();
    run(src, backward_dst(epi), s, 0, &epi, pre);
    return;
  }
  // output layer: out.grad is the loss gradient, zero outside the split's labelled rows, so
  // only the edges into those rows contribute (the column-subset graph gathers them itself)
  Event e0, e1;
  if (ctx->profile) {
    e0 = Event::create(true);
    e1 = Event::create(true);
    e0.record(s.get());
  }
  // (compact: the Matmul left out.grad in compact rows, which the column-subset graph reads
  // as its columns directly; else it gathers them from the full rows)
  const float *g_in = ctx->compact_n ? ctx->compact_z->dev_grad.get() : out->dev_grad.get();
  const GsEpilogue epi = backward_epilogue(cg);
  cg->graphsum(g_in, out->ld, backward_dst(epi), in->ld, dim, s.get(), ctx->compact_n > 0, &epi,
               pre);
  if (ctx->profile) {
    e1.record(s.get());
    ctx->gs_events->emplace_back(e0, e1);
    ctx->gs_bytes->push_back(cg->algorithmic_bytes(dim));
  }
}

// ------------------------------------------------------------------------------------------
// GraphAttention (k_gat.hip)
// ------------------------------------------------------------------------------------------
GraphAttention::GraphAttention(shared_ptr<Variable> in_, shared_ptr<Variable> out_,
                               DevGraph *graph_, int dim_, shared_ptr<Variable> attn_,
                               long long offset_, int heads_, float p_,
                               shared_ptr<DropoutRng> rng_, ModuleContext *ctx_)
    : in(std::move(in_)), out(std::move(out_)), attn(std::move(attn_)), graph(graph_), dim(dim_),
      offset(offset_), heads(heads_), p(p_), rng(std::move(rng_)), ctx(ctx_) {
  PGCN_CHECK(in && out && attn && graph && dim >= 1 && dim <= kGatMaxWidth && in->cols == dim &&
                 out->cols == dim && graph->rows() == graph->cols() && in->rows >= graph->rows() &&
                 out->rows >= graph->rows() && offset >= 0 && offset + 2LL * dim <= attn->size,
             PGCN_E_INVALID, "attention: widths up to 128 on a square pattern");
  PGCN_CHECK(gat_heads_ok(dim, heads) && heads <= kGatMaxHeads, PGCN_E_INVALID,
             "attention: heads must divide the width into head widths of 4, 8, 16, 32, 64 or 128");
  PGCN_CHECK(p >= 0.0f && p < 1.0f && (p > 0.0f) == (rng != nullptr) && (!rng || ctx),
             PGCN_E_INVALID, "attention: dropout in [0, 1), with its mask stream");
  const GatPattern &g = graph->gat_pattern();  // (host build and upload: now, not in an epoch)
  PGCN_CHECK(!rng || (rng->elem_begin == 0 && rng->elem_end == g.nnz * heads), PGCN_E_INVALID,
             "attention: the mask stream covers nnz * heads weights");
  u.allocate((size_t)std::max(g.n, 1) * heads);
  v.allocate((size_t)std::max(g.n, 1) * heads);
  alpha.allocate((size_t)std::max<long long>(g.nnz, 1) * heads);
  ws.allocate(std::max<size_t>(gat_bwd_workspace(g, dim, heads) / sizeof(float), 4));
  z.allocate((size_t)std::max(g.n, 1) * out->ld);
  for (const auto *b : {&u, &v, &alpha, &ws, &z}) b->zero();
}

void GraphAttention::forward(bool training, const Stream &s) const {
  const GatPattern &p = graph->gat_pattern();
  const float *a = attn->dev_data.get() + offset;
  const bool drop = training && rng;
  if (drop)  // this epoch's mask of the layer: the stream moves on by one period per draw
    launch_dropout_mask(rng->states.get(), rng->n_chunks, 64 * rng->chunk_lo, rng->elem_end,
                        this->p, rng->mask.get(), ctx->jump_table, s.get(), 0, rng->per);
  launch_gat_scores(in->dev_data.get(), in->ld, p.n, dim, heads, a, a + dim, u.get(), v.get(),
                    s.get());
  launch_gat_fwd(p, in->dev_data.get(), in->ld, u.get(), v.get(), kSlope, out->dev_data.get(),
                 out->ld, dim, heads, drop ? rng->mask.get() : nullptr, drop ? rng->mask_base : 0,
                 scale(), training ? alpha.get() : nullptr, s.get());
  if (training && p.n > 0)
    PGCN_HIP(hipMemcpyAsync(z.get(), out->dev_data.get(), sizeof(float) * (size_t)p.n * out->ld,
                            hipMemcpyDeviceToDevice, s.get()));
}

void GraphAttention::backward(const Stream &s) const {
  if (!in->dev_grad || !out->dev_grad || !attn->dev_grad) return;
  const GatPattern &p = graph->gat_pattern();
  const float *a = attn->dev_data.get() + offset;
  // (a residual layer's out.grad stays unmasked: its ReLU backward wrote dev_grad_z)
  const float *g = out->dev_grad_z ? out->dev_grad_z.get() : out->dev_grad.get();
  // (the mask of the training forward this backward belongs to)
  launch_gat_bwd(p, in->dev_data.get(), in->ld, u.get(), v.get(), kSlope, alpha.get(), z.get(),
                 out->ld, g, out->ld, a, a + dim, in->dev_grad.get(), in->ld, dim, heads,
                 rng ? rng->mask.get() : nullptr, rng ? rng->mask_base : 0, scale(),
                 attn->dev_grad.get() + offset, ws.get(), s.get());
}

// ------------------------------------------------------------------------------------------
// SageAggregate (k_sage.hip; the mean on DevGraph::graphsum)
// ------------------------------------------------------------------------------------------
SageAggregate::SageAggregate(shared_ptr<Variable> in_, shared_ptr<Variable> out_,
                             DevGraph *graph_, DevGraph *mean_fwd_, DevGraph *mean_bwd_, int dim_,
                             int aggregator_, bool root_)
    : in(std::move(in_)), out(std::move(out_)), graph(graph_), mean_fwd(mean_fwd_),
      mean_bwd(mean_bwd_), dim(dim_), aggregator(aggregator_), root(root_),
      ld_s((dim_ + 3) / 4 * 4) {
  PGCN_CHECK(in && out && graph && dim >= 1 && dim <= kSageMaxWidth &&
                 in->cols == (root ? 2 : 1) * dim && out->cols == dim &&
                 graph->rows() == graph->cols() && in->rows >= graph->rows() &&
                 out->rows >= graph->rows() && in->ld % 4 == 0 && out->ld % 4 == 0,
             PGCN_E_INVALID, "sage: widths up to 128 on a square pattern");
  PGCN_CHECK(aggregator == 2 || (aggregator == 1 && mean_fwd && mean_bwd &&
                                 mean_fwd->rows() == graph->rows() &&
                                 mean_bwd->rows() == graph->rows()),
             PGCN_E_INVALID, "sage: aggregator 1 (mean, with its two graphs) or 2 (max)");
  const size_t n = (size_t)std::max(graph->rows(), 1);
  if (aggregator == 2) {  // (host build and upload: now, not in an epoch)
    graph->sage_ws();
    arg.allocate(n * ld_s);
    arg.zero();
  } else {
    mean_fwd->prepare(dim);
    mean_bwd->prepare(dim);
  }
  if (staged()) {  // (the padding columns stay zero: the copies write [0, dim) only)
    q.allocate(n * ld_s);
    dq.allocate(n * ld_s);
    q.zero();
    dq.zero();
  }
}

void SageAggregate::forward(bool training, const Stream &s) const {
  const int n = graph->rows();
  const float *P = in->dev_data.get(), *R = root ? P : nullptr;
  const float *Q = root ? P + dim : P;
  int ld_q = in->ld;
  if (staged()) {
    launch_copy_cols(Q, in->ld, q.get(), ld_s, n, dim, false, s.get());
    Q = q.get();
    ld_q = ld_s;
  }
  if (aggregator == 2) {
    launch_agg_max_fwd(graph->gat_pattern(), graph->sage_ws(), Q, ld_q, dim, R, in->ld,
                       out->dev_data.get(), out->ld, training ? arg.get() : nullptr, ld_s, s.get());
    return;
  }
  mean_fwd->graphsum(Q, ld_q, out->dev_data.get(), out->ld, dim, s.get());
  if (R) launch_copy_cols(R, in->ld, out->dev_data.get(), out->ld, n, dim, true, s.get());
}

void SageAggregate::backward(const Stream &s) const {
  if (!in->dev_grad || !out->dev_grad) return;
  const int n = graph->rows();
  // (a residual layer's out.grad stays unmasked: its ReLU backward wrote dev_grad_z)
  const float *g = out->dev_grad_z ? out->dev_grad_z.get() : out->dev_grad.get();
  float *din = in->dev_grad.get();
  float *dQ = staged() ? dq.get() : root ? din + dim : din;
  const int ld_dq = staged() ? ld_s : in->ld;
  if (aggregator == 2)
    launch_agg_max_bwd(graph->gat_pattern(), graph->sage_ws(), g, out->ld, arg.get(), ld_s, dim,
                       dQ, ld_dq, s.get());
  else
    mean_bwd->graphsum(g, out->ld, dQ, ld_dq, dim, s.get());
  if (staged()) launch_copy_cols(dQ, ld_s, din + dim, in->ld, n, dim, false, s.get());
  if (root) launch_copy_cols(g, out->ld, din, in->ld, n, dim, false, s.get());
}

// ------------------------------------------------------------------------------------------
// Readout (k_readout.hip)
// ------------------------------------------------------------------------------------------
Readout::Readout(shared_ptr<Variable> in_, shared_ptr<Variable> out_,
                 const std::vector<int> &graph_ptr_, int dim_, int mode_)
    : in(std::move(in_)), out(std::move(out_)), n(graph_ptr_.empty() ? 0 : graph_ptr_.back()),
      G((int)graph_ptr_.size() - 1), dim(dim_), mode(mode_), ld_s((dim_ + 3) / 4 * 4) {
  PGCN_CHECK(in && out && G >= 1 && dim >= 1 && dim <= kReadoutMaxWidth && in->cols == dim &&
                 out->cols == dim && in->rows >= n && out->rows >= G && in->ld % 4 == 0 &&
                 out->ld % 4 == 0 && mode >= kReadoutSum && mode <= kReadoutMax &&
                 graph_ptr_.front() == 0,
             PGCN_E_INVALID, "readout: widths up to 128, mode 1..3, graph_ptr from 0");
  std::vector<int> ng((size_t)std::max(n, 1), 0);
  for (int g = 0; g < G; g++) {
    PGCN_CHECK(graph_ptr_[(size_t)g + 1] >= graph_ptr_[(size_t)g], PGCN_E_INVALID,
               "readout: graph_ptr must not decrease");
    max_len = std::max(max_len, graph_ptr_[(size_t)g + 1] - graph_ptr_[(size_t)g]);
    for (int i = graph_ptr_[(size_t)g]; i < graph_ptr_[(size_t)g + 1]; i++) ng[(size_t)i] = g;
  }
  graph_ptr.allocate(graph_ptr_.size());
  graph_ptr.upload(graph_ptr_);
  node_graph.allocate(ng.size());
  node_graph.upload(ng);
  if (mode == kReadoutMax) {
    arg.allocate((size_t)G * ld_s);
    arg.zero();
  }
  if (max_len > kReadoutChunk) ws.allocate(readout_workspace(n) / sizeof(float));
}

void Readout::forward(bool training, const Stream &s) const {
  launch_readout_fwd(in->dev_data.get(), in->ld, graph_ptr.get(), G, n, dim, mode, max_len,
                     out->dev_data.get(), out->ld,
                     training && mode == kReadoutMax ? arg.get() : nullptr, ld_s,
                     ws ? ws.get() : nullptr, s.get());
}

void Readout::backward(const Stream &s) const {
  if (!in->dev_grad || !out->dev_grad) return;
  launch_readout_bwd(out->dev_grad.get(), out->ld, graph_ptr.get(), node_graph.get(),
                     mode == kReadoutMax ? arg.get() : nullptr, ld_s, G, n, dim, mode,
                     in->dev_grad.get(), in->ld, s.get());
}

// ------------------------------------------------------------------------------------------
// LinkDecoder (k_link.hip)
// ------------------------------------------------------------------------------------------
LinkDecoder::LinkDecoder(shared_ptr<Variable> in_, shared_ptr<Variable> out_,
                         const LinkIndexDev *links_, int dim_)
    : in(std::move(in_)), out(std::move(out_)), links(links_), dim(dim_) {
  PGCN_CHECK(in && out && links && dim >= 1 && dim <= kLinkMaxWidth && in->cols == dim &&
                 in->rows >= links->index().n && in->ld % 4 == 0 && out->cols == 1 &&
                 out->ld % 4 == 0 && out->ld >= 4 && out->rows >= links->index().n_pairs,
             PGCN_E_INVALID, "link decoder: embedding width up to 128, scores [pairs][4]");
}

void LinkDecoder::forward(bool, const Stream &s) const {
  launch_link_score_fwd(links->index(), in->dev_data.get(), in->ld, dim, out->dev_data.get(),
                        out->ld, s.get());
}

void LinkDecoder::backward(const Stream &s) const {
  if (!in->dev_grad || !out->dev_grad) return;
  launch_link_score_bwd(links->index(), in->dev_data.get(), in->ld, dim, out->dev_grad.get(),
                        out->ld, in->dev_grad.get(), in->ld, s.get());
}

// ------------------------------------------------------------------------------------------
// ReLU (src/module.cu:215-265)
// ------------------------------------------------------------------------------------------
ReLU::ReLU(shared_ptr<Variable> in_) : in(std::move(in_)) {
  mask.allocate((size_t)in->rows * in->ld);
  mask.zero();
}

void ReLU::forward(bool training, const Stream &s) const {
  if (skip_forward) {  // applied by the GraphSum before it (epilogue)
    skip_forward = false;
    return;
  }
  launch_relu_fwd(in->dev_data.get(), (long long)in->rows * in->ld, mask.get(), training, s.get());
}

void ReLU::backward(const Stream &s) const {
  if (skip_backward) {  // applied by the GraphSum backward before it (epilogue)
    skip_backward = false;
    return;
  }
  if (in->dev_grad_z)  // residual layer: dev_grad stays the gradient of the sum
    launch_relu_bwd_to(in->dev_grad.get(), (long long)in->rows * in->ld, mask.get(),
                       in->dev_grad_z.get(), s.get());
  else
    launch_relu_bwd(in->dev_grad.get(), (long long)in->rows * in->ld, mask.get(), s.get());
}

// ------------------------------------------------------------------------------------------
// ResidualConnection (src/module.cu:566-593)
// ------------------------------------------------------------------------------------------
ResidualConnection::ResidualConnection(shared_ptr<Variable> prev_, shared_ptr<Variable> current_)
    : prev(std::move(prev_)), cur(std::move(current_)) {
  PGCN_CHECK(prev && cur && prev != cur, PGCN_E_INVALID, "residual: two distinct variables");
  PGCN_CHECK(prev->rows == cur->rows && prev->cols == cur->cols && prev->ld == cur->ld,
             PGCN_E_INVALID, "residual: prev and current must have the same size");
  PGCN_CHECK(!prev->skip_from && !cur->dev_grad_z, PGCN_E_INVALID,
             "residual: one connection per variable pair");
  if (prev->dev_grad && cur->dev_grad) {
    cur->dev_grad_z.allocate(cur->dev_grad.size());
    cur->dev_grad_z.zero();
    prev->skip_from = cur.get();
  }
}

ResidualConnection::~ResidualConnection() {
  if (prev->skip_from == cur.get()) prev->skip_from = nullptr;
}

void ResidualConnection::forward(bool training, const Stream &s) const {
  if (skip_forward) {  // added by the GraphSum before it (epilogue)
    skip_forward = false;
    if (training) last_fused = true;
    return;
  }
  if (training) last_fused = false;
  launch_residual_fwd(cur->dev_data.get(), prev->dev_data.get(), (long long)cur->rows * cur->ld,
                      s.get());
}

// prev.grad += current.grad is made by the Matmul that writes prev.grad (Variable::skip_from)
void ResidualConnection::backward(const Stream &) const {}

// ------------------------------------------------------------------------------------------
// LayerNorm (k_layernorm.hip)
// ------------------------------------------------------------------------------------------
LayerNorm::LayerNorm(shared_ptr<Variable> in_, shared_ptr<Variable> norm_, long long offset_,
                     int rows_)
    : in(std::move(in_)), norm(std::move(norm_)), offset(offset_), rows(rows_) {
  PGCN_CHECK(in && norm && in->cols >= 1 && in->cols <= kLayerNormMaxWidth && rows >= 0 &&
                 rows <= in->rows && offset >= 0 && offset + 2LL * in->cols <= norm->size,
             PGCN_E_INVALID, "layer_norm: widths up to 1024");
  xhat.allocate((size_t)std::max(in->rows, 1) * in->ld);
  xhat.zero();
  rstd.allocate((size_t)std::max(in->rows, 1));
  rstd.zero();
  ws.allocate(std::max<size_t>(layernorm_bwd_workspace(rows, in->cols) / sizeof(float), 1));
}

void LayerNorm::forward(bool training, const Stream &s) const {
  GsEpilogue e;
  if (fwd_relu && in->ld == in->cols) {  // the tail's element order is the storage order
    e.mode = 1;
    e.relu_mask = training ? fwd_relu->mask_ptr() : nullptr;
    e.relu_ld = in->ld;
    if (training && fwd_drop) {
      fwd_drop->draw_fused(s.get());
      const DropoutRng &r = fwd_drop->state();
      e.drop_mask = r.mask.get();
      e.drop_base = r.mask_base;
      e.drop_cols = in->cols;
      e.drop_scale = fwd_drop->scale();
    }
    if (fwd_res) {
      e.res = const_cast<float *>(fwd_res->previous()->dev_data.get());  // (read only)
      e.res_ld = fwd_res->previous()->ld;
      fwd_res->skip_forward = true;
    }
    fwd_relu->skip_forward = true;
  }
  if (training) last_fused = e.mode != 0;
  const float *gamma = norm->dev_data.get() + offset;
  launch_layernorm_fwd(in->dev_data.get(), in->ld, in->dev_data.get(), in->ld, rows, in->cols,
                       gamma, gamma + in->cols, kEps, training ? xhat.get() : nullptr, in->ld,
                       training ? rstd.get() : nullptr, &e, s.get());
}

void LayerNorm::backward(const Stream &s) const {
  if (!in->dev_grad || !norm->dev_grad) return;
  float *g = in->dev_grad_z ? in->dev_grad_z.get() : in->dev_grad.get();
  float *dgamma = norm->dev_grad.get() + offset;
  launch_layernorm_bwd(g, in->ld, xhat.get(), in->ld, rstd.get(), norm->dev_data.get() + offset,
                       rows, in->cols, g, in->ld, dgamma, dgamma + in->cols, ws.get(), s.get());
}

// ------------------------------------------------------------------------------------------
// Matmul (src/module.cu:270-472; hpdga module.cpp:13-38)
// ------------------------------------------------------------------------------------------
Matmul::Matmul(shared_ptr<Variable> a_, shared_ptr<Variable> b_, shared_ptr<Variable> c_,
               int m_, int n_, int p_, ModuleContext *ctx_)
    : a(std::move(a_)), b(std::move(b_)), c(std::move(c_)), m(m_), n(n_), p(p_), ctx(ctx_) {}

void Matmul::forward(bool training, const Stream &s) const {
  if (fused_forward && !(last_layer && ctx->compact_n)) return;  // CrossEntropyLoss::forward
  const bool cmp = last_layer && ctx->compact_n;  // compact output layer: the split's rows
  const Variable &A = cmp ? *ctx->compact_z : *a, &C = cmp ? *ctx->compact_out : *c;
  MmProfile prof(ctx, s.get(), 2.0 * (cmp ? ctx->compact_n : m) * p * n);
  launch_gemm_nn(cmp ? ctx->compact_n : m, p, n, A.dev_data.get(), A.ld, b->dev_data.get(), b->ld,
                 0, C.dev_data.get(), C.ld, nullptr, 0, 0, 1.0f, s.get());
}

void Matmul::backward_input(const Stream &s) const {
  launch_gemm_nn(m, n, p, c->dev_grad.get(), c->ld, b->dev_data.get(), b->ld, 1, a->dev_grad.get(),
                 a->ld, nullptr, 0, 0, 1.0f, s.get());
  add_skip_grad(s);
}

// a is the `prev` of a ResidualConnection: a.grad += current.grad (the unmasked gradient of
// relu(Z) + a), one element-wise launch over this rank's rows
void Matmul::add_skip_grad(const Stream &s) const {
  if (!a->skip_from || !a->dev_grad) return;
  launch_residual_bwd(a->dev_grad.get(), a->skip_from->dev_grad.get(), (long long)m * a->ld,
                      s.get());
}

void Matmul::backward_weight(hipStream_t s, void *ws) const {
  launch_gemm_tn(m, p, n, a->dev_data.get(), a->ld, c->dev_grad.get(), c->ld, b->dev_grad.get(),
                 b->ld, nullptr, 0, 0, 1.0f, ws, s);
}

void Matmul::backward(const Stream &s) const {
  const bool cmp = last_layer && ctx->compact_n;
  const bool a_done = input_grad_done && !cmp;  // a.grad written by the loss kernel (forward)
  const bool b_done = weight_grad_done && !cmp;  // b.grad too
  input_grad_done = weight_grad_done = false;
  const Variable &A = cmp ? *ctx->compact_z : *a, &C = cmp ? *ctx->compact_out : *c;
  const int rows = cmp ? ctx->compact_n : m;
  const bool side = ctx->mm_side && ctx->side_stream && ctx->gemm_workspace_side && !ctx->profile;
  // (the contractions the loss kernel did are profiled there; a side-stream b.grad is not)
  MmProfile prof(ctx, s.get(), 2.0 * rows * p * n * ((a_done ? 0 : 1) + (side || b_done ? 0 : 1)));
  if (side) {
    // b.grad = a^T * c.grad on the side stream, from here (a.data and c.grad are final; nothing
    // later in the backward pass writes them), joined before the optimizer (GCN)
    ctx->mm_fork.record(s.get());
    ctx->mm_fork.wait_on(ctx->side_stream);
    launch_gemm_tn(rows, p, n, A.dev_data.get(), A.ld, C.dev_grad.get(), C.ld, b->dev_grad.get(),
                   b->ld, nullptr, 0, 0, 1.0f, ctx->gemm_workspace_side, ctx->side_stream);
    ctx->side_pending = true;
  }
  // a.grad = c.grad * b^T   (b stored [n][p] => trans_b); the Dropout / ReLU backward on a
  // in its final write when gemm_nn would take k_xstream_nn anyway (same product, same bits)
  // (not next to a ResidualConnection: the skip gradient comes between the product and the tail)
  if (!a_done && bwd_relu && !cmp && !A.skip_from && !A.dev_grad_z && A.ld == n &&
      xstream_ok(n, p) && !xstream_ring_ok(p, C.ld)) {
    XsEpilogue e;
    if (bwd_drop) {
      e.bwd_drop = bwd_drop->state().mask.get();
      e.drop_base = bwd_drop->state().mask_base;
      e.drop_scale = bwd_drop->scale();
      bwd_drop->skip_backward = true;
    }
    e.bwd_relu = bwd_relu->mask_ptr();
    bwd_relu->skip_backward = true;
    launch_xstream_nn(rows, n, p, C.dev_grad.get(), C.ld, b->dev_data.get(), b->ld, 1,
                      A.dev_grad.get(), A.ld, nullptr, 1.0f, s.get(), nullptr, &e);
  } else if (!a_done) {
    launch_gemm_nn(rows, n, p, C.dev_grad.get(), C.ld, b->dev_data.get(), b->ld, 1,
                   A.dev_grad.get(), A.ld, nullptr, 0, 0, 1.0f, s.get());
  }
  if (!cmp) add_skip_grad(s);
  // b.grad = a^T * c.grad (deterministic split-M reduction)
  if (!side && !b_done)
    launch_gemm_tn(rows, p, n, A.dev_data.get(), A.ld, C.dev_grad.get(), C.ld, b->dev_grad.get(),
                   b->ld, nullptr, 0, 0, 1.0f, ctx->gemm_workspace, s.get());
}

// ------------------------------------------------------------------------------------------
// CrossEntropyLoss (src/module.cu:477-562; hpdga module.cpp:122-156)
// ------------------------------------------------------------------------------------------
CrossEntropyLoss::CrossEntropyLoss(shared_ptr<Variable> logits_, int num_classes_,
                                   ModuleContext *ctx_)
    : logits(std::move(logits_)), num_classes(num_classes_), ctx(ctx_) {}

// The fused loss kernel also writes the output layer's input grad (on MFMA in k_xstream_nn's
// sequence: bit-identical; reddit A/B 517.7 -> 520.1 epochs/s) and, at fuse_output >= 2,
// per-block partials of the Matmul's weight grad, reduced in block order right after it
// (deterministic; the same sums as k_gemm_tn's in another grouping): 2 on graphs of >= 65,536
// rows (small graphs keep k_gemm_tn's order: nothing to gain there), 3 on any graph

void CrossEntropyLoss::forward(bool training, const Stream &s) const {
  if (fused && !ctx->compact_n) {
    const Variable &Hv = *fused->input(), &Wv = *fused->weight();
    // the fused output layer's contractions (logits = H W; training: dH = dOut W^T and the
    // W.grad partials) over the fused kernel's time, which includes the loss itself
    const double mm = 2.0 * logits->rows * num_classes * fused->inner();
    MmProfile prof(ctx, s.get(), training ? 3.0 * mm : mm);
    float *dH = Hv.dev_grad ? Hv.dev_grad.get() : nullptr;
    const int nb = xent_blocks(logits->rows);
    float *dWp = nullptr;
    bool deferred = false;
    const Knobs &kn = *ctx->knobs;
    // (an edge-cut rank's rows are a slice of a large graph: the block partials too)
    if (training && kn.fuse_output >= 2 &&
        (kn.fuse_output == 3 || logits->rows >= 65536 || ctx->comm) &&
        Wv.dev_grad && logits->ld <= 48 &&
        !ctx->mm_side &&
        tn_reduce_blocks_workspace(nb, fused->inner(), 48) <= ctx->gemm_workspace_bytes)
      dWp = static_cast<float *>(ctx->gemm_workspace);
    // r06: a small graph's partials straight into the deferred-reduction pool when tn_fold is
    // on (the Adam launch sums them in block order): the output layer's W.grad needs no launch
    // of its own (k_xstream_tn before; the same sums in another grouping)
    // (tn_fold 0, or no room: the same one ordered pass as its own launch -- the same bits)
    bool one_pass = false;
    if (training && !dWp && kn.fuse_output >= 2 && kn.defer_wgrad && !ctx->comm &&
        nb <= kDeferWgradMaxBlocks && Wv.dev_grad && logits->ld <= 48 && !ctx->mm_side) {
      dWp = tn_defer_blocks(nb, fused->inner(), num_classes, 48, Wv.dev_grad.get(), Wv.ld);
      deferred = dWp != nullptr;
      if (!dWp && (size_t)nb * fused->inner() * 48 * sizeof(float) <= ctx->gemm_workspace_bytes) {
        dWp = static_cast<float *>(ctx->gemm_workspace);
        one_pass = true;
      }
    }
    // training: dH also to the ring table of the GraphSum backward that reads it
    XentTable tb;
    const bool staged = training && dH && dh_reader && fused->inner() == 16 &&
                        dh_reader->claim_backward_table(Hv.rows, Hv.ld, &tb);
    launch_out_xent(Hv.dev_data.get(), Hv.ld, fused->inner(), Wv.dev_data.get(), Wv.ld,
                    logits->dev_data.get(), logits->ld, training ? logits->dev_grad.get() : nullptr,
                    ctx->truth, logits->rows, num_classes, ctx->count, training ? 1 : 0,
                    ctx->xent_partials, s.get(), dH, Hv.ld, dWp, staged ? &tb : nullptr, ctx->fin);
    ctx->fin_taken = ctx->fin != nullptr;
    if (one_pass)
      launch_tn_reduce_one_pass(dWp, nb, fused->inner(), num_classes, 48, Wv.dev_grad.get(),
                                Wv.ld, s.get());
    else if (dWp && !deferred)
      launch_tn_reduce_blocks(dWp, nb, fused->inner(), num_classes, 48, Wv.dev_grad.get(), Wv.ld,
                              s.get());
    fused->input_grad_done = training && dH;
    fused->weight_grad_done = dWp != nullptr;
    return;
  }
  const Variable &L = ctx->compact_n ? *ctx->compact_out : *logits;
  launch_xent_fwd(L.dev_data.get(), L.ld, training ? L.dev_grad.get() : nullptr,
                  ctx->compact_n ? ctx->compact_truth : ctx->truth,
                  ctx->compact_n ? ctx->compact_n : logits->rows, num_classes, ctx->count,
                  training ? 1 : 0, ctx->xent_partials, s.get(), ctx->compact_n ? 0 : 1,
                  ctx->fin);
  ctx->fin_taken = ctx->fin != nullptr;
}

void CrossEntropyLoss::backward(const Stream &) const {}  // module.cpp:155-156

// ------------------------------------------------------------------------------------------
// BCEWithLogitsLoss (multi-label; k_multilabel.hip)
// ------------------------------------------------------------------------------------------
BCEWithLogitsLoss::BCEWithLogitsLoss(shared_ptr<Variable> logits_, int num_classes_,
                                     ModuleContext *ctx_)
    : logits(std::move(logits_)), num_classes(num_classes_), ctx(ctx_) {}

void BCEWithLogitsLoss::forward(bool training, const Stream &s) const {
  const bool cmp = ctx->compact_n != 0;
  const Variable &L = cmp ? *ctx->compact_out : *logits;
  PGCN_CHECK(ctx->label_bits && (!cmp || ctx->compact_label_bits), PGCN_E_INVALID,
             "BCEWithLogitsLoss: no label bits");
  launch_bce_fwd(L.dev_data.get(), L.ld, training ? L.dev_grad.get() : nullptr,
                 cmp ? ctx->compact_truth : ctx->truth,
                 cmp ? ctx->compact_label_bits : ctx->label_bits, ctx->label_words,
                 cmp ? ctx->compact_n : logits->rows, num_classes, std::max(ctx->count, 1),
                 training ? 1 : 0, ctx->xent_partials, s.get());
}

void BCEWithLogitsLoss::backward(const Stream &) const {}  // the forward wrote the gradient

}  // namespace pgcn
