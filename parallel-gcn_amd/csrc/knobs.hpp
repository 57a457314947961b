// parallel-gcn_amd/csrc/knobs.hpp -- the engine knobs of pgcn_debug_set: one struct, one table.
// pgcn_debug_set writes process_knobs(); a knob applies to what is created after it was set:
//   engine scope   GCN copies process_knobs() at construction and its modules, optimizer and
//                  communicator read that copy (ModuleContext::knobs; the C++ API has no engine:
//                  its context points at process_knobs() itself);
//   graph scope    DevGraph keeps the Knobs it is constructed with (GCN's copy; process_knobs()
//                  from the C-ABI creators) for every schedule it builds later;
//   process scope  read at the call.
#pragma once

namespace pgcn {

// "fuse_epilogue" bits
constexpr int kFuseTails = 1, kFusePrestage = 2, kFuseXstream = 4, kFuseMatmulTails = 8;

struct Knobs {
  // ---- engine scope
  // eval's first-layer forward also computes the next training forward's product (SparseMatmul,
  // one pass over dense X)
  int train_ahead = 1;
  // the output layer's GraphSum forward computes only the current split's labelled rows.  Off by
  // default: the reference's forward produces the logits of every row, and so does the default
  // engine (r02); on, rows outside the split keep stale logits (get_var refuses them)
  int split_rows = 0;
  // the output layer's GraphSum backward keeps only the edges from the training split's columns.
  // The loss gradient is exactly zero on every other row, so the skipped terms are exact zeros:
  // in.grad is the full gradient of every row
  int split_cols = 1;
  // eval's first layer as (Â X) W1 from Â X computed once (Â and X are constants: exact
  // algebra, fp32 rounding order differs)
  int eval_ax = 1;
  // replay a captured per-epoch hipGraph when eligible; measured no faster than eager launches
  int epoch_graph = 0;  // (r01: GPU-bound epochs)
  // bits, all bit-identical to separate launches:
  //   1 (kFuseTails)    the ReLU / Dropout modules next to a GraphSum run in its final-write
  //                     epilogue (gs_epilogue.hpp);
  //   2 (kFusePrestage) ... and that epilogue also writes the next GraphSum's prescaled input
  //                     table, which then skips its prescale launch;
  //   4 (kFuseXstream)  the first layer's X-stream product applies the eval ReLU / writes the
  //                     first GraphSum's table;
  //   8 (kFuseMatmulTails) the Dropout / ReLU backward before a Matmul run in its input-grad
  //                     product's final write (k_xstream_nn: outputs of <= 16 columns; the
  //                     small graphs' second layer -- two launches fewer per epoch).
  int fuse_epilogue = kFuseTails | kFusePrestage | kFuseXstream | kFuseMatmulTails;
  // 0 = separate Matmul + loss; 1 = the output layer's Matmul forward and input grad run inside
  // the loss (launch_out_xent) when the Matmul produces the logits (the reassociated order:
  // GraphSum, then Matmul) from at most 16 columns (bit-identical); 2 (default) = ... and its
  // weight grad's block partials on graphs of >= 65,536 rows or on an edge-cut rank (the same
  // sums in another grouping); 3 = ... on any graph
  int fuse_output = 2;
  // Matmul weight gradients on the side stream (ModuleContext) on graphs of at least kMmSideRows
  // rows; 2 = on every graph.  Off: r02 A/B on reddit-114M, three runs each, 486.5 (on) vs 487.4
  // (off) epochs/s -- the LDS GraphSum holds every CU with one workgroup, so the side kernels
  // find no room to overlap; cora 5,957 vs 7,136 (the stream hand-offs cost more than the ~7 us
  // of kernels they hide)
  int mm_side = 0;
  // the edge-cut eval pass's last exchange and output layer on the (high-priority) comm stream
  // beside the next epoch's mask draw and first-layer product (ModuleContext::tail_stream; peer
  // exchange between processes only; bit-identical).  Off: on the solo timing form, where the
  // push has no link time to hide, the overlapped kernels slow each other -- W = 8 rank epoch
  // 0.511-0.514 vs 0.489-0.495 ms (0.502-0.506 on the low-priority side stream;
  // profiles/r05/s).  An 8-GPU run with slow links may still gain (the eval push's link time
  // beside ~48 us of compute): `bench.py --knob eval_tail=1`
  int eval_tail = 0;
  // the hidden dropout's mask drawn in the input dropout's launch (1: sparse X; 2: dense X too;
  // bit-identical)
  int co_draw = 2;
  // sparse X with train_ahead: eval's first-layer product also computes the next training
  // forward's (k_spmm_csr<true>, one pass; bit-identical)
  int sparse_dual = 1;
  // one GPU, the weight gradients' last reduction pass runs inside the Adam launch
  // (GCN::backward_pass; bit-identical)
  int tn_fold = 1;
  // one GPU, the loss kernel's last block sums the pass's scalars and writes its results ring
  // slot (XentFinal; one launch fewer per pass): 1 (default) up to kFinishMaxBlocks loss blocks,
  // 2 also above them with two levels of arrivals (reddit: measured even, 615.2-616.0 vs 615.4
  // epochs/s -- the loss kernels' tails grew by what the reduce launches cost, profiles/r06/x)
  int fuse_finish = 1;
  // 64-draw mask words per stored RNG state (1 or 2); 0 = by size: 2 from kMaskPer2Chunks words
  // on (reddit's input mask: half the period jumps, 68.3 -> 65.2 us for both masks), else 1 (a
  // W = 8 rank's input mask, 274 k words: twice the threads, each chain half as long -- 17.3 ->
  // 14.5 us, profiles/r06/o)
  int mask_per = 0;
  // sparse X's W1.grad summed as a fixed tree over each feature's entries (k_spmm_csc_tree)
  // instead of hpdga's sequential scatter order (k_spmm_csc_bwd, bit-exact); deterministic, the
  // sums in another order.  Off: measured slower where it counts (same box, 400 epochs,
  // profiles/r06/k: citeseer 11.6-11.7k vs 12.1k epochs/s, pubmed_synth 6.57-6.59k vs 7.06k,
  // cora 10.7-12.4k vs 12.3k) -- the chain's one-wave tail is not what bounds the launch
  int csc_tree = 0;
  // one GPU, the next input mask drawn by the Adam launch
  int mask_adam = 1;
  // dense X with eval_ax, one GPU -- the next input mask drawn by eval's first-layer X-stream
  // pass instead (GCN::mask_in_eval).  Off: bit-identical but slower -- two drawing waves per CU
  // (all the VGPR budget leaves beside the consumers) take 202 us for what k_dropout_mask's 32
  // waves per CU draw in 63, so the pass doubles (reddit 604-605 vs 617-619 epochs/s,
  // profiles/r06/z2)
  int mask_xstream = 0;
  // on graphs of fewer than kMmSideRows nodes the output layer runs in the reassociated order
  // (Â H) W even when the classes are no more than the last hidden width (<= 16), so its Matmul
  // runs inside the loss kernel: a small graph's epoch is bound by its launches, not by the
  // GraphSum's width (the fp32 order differs, like reddit's)
  int reassoc_small = 1;
  // "defer_wgrad": a small graph's fused loss kernel writes the output layer's W.grad block
  // partials into the deferred-reduction pool (tn_fold), summed by the Adam launch
  int defer_wgrad = 1;
  // the peer exchange's receive slots in uncached device memory (hipDeviceMallocUncached, MTYPE
  // UC) instead of plain device memory -- no cache holds a slot line on the receiver; the
  // pushes are then write-through (0.3 TB/s on one GPU, r05)
  int peer_uncached = 0;
  // ---- graph scope
  // d = 16 feature tables above this many KB take the LDS GraphSum; -1 = the default,
  // DevGraph::kLdsMinBytes (the plain path blocks its columns per XCD above DevGraph::kL2Budget:
  // below it one XCD's 4 MB L2 holds the whole table).  The LDS path also wants rows to fill its
  // workgroups (kLdsMinRows).  r02, the edge-cut engine's per-rank graphs of reddit-114M
  // (tools/rank_graphsum.py, 118 k padded rows): 3.7 MB table (4 ranks) LDS 0.123 vs plain
  // 0.249 ms, 1.9 MB (8 ranks) 0.083 vs 0.114 ms; 15 MB (1 rank) 0.33 vs 1.04 ms
  int lds_min_kb = -1;
  // column blocks of the LDS schedule; 0 = by shape (r01, reddit): 4 blocks when the graph has
  // about as many rows as columns (the full graph and its column subsets: one round of 256
  // workgroups, half the partials; the same kernel time, combine 18 -> 11 us), 8 for a small row
  // subset (its 256 workgroups then stream half the table each: val rows 0.11 vs 0.22 ms)
  int lds_blocks = 0;
  // the rows of the plain unblocked path longer than one work item: 0 = their items write slots
  // that a combine launch sums; 1 = the last of a row's items to finish sums them in the same
  // launch (an arrival counter per row, the combine's order: the same bits), on graphs of <=
  // kSmallNnz slots (each arrival writes its XCD's L2 back: costly when many rows split --
  // pubmed_synth lost 4 % at 8-iteration items); 2 = on those graphs, rows up to 8 items long
  // stay one item (no slots; another summation order); 3 = as 1, but rows of up to 8
  // workgroup-wide iterations are summed by one whole workgroup (4 waves, an LDS reduce in wave
  // order: no cross-workgroup hand-off; another summation order), power-of-two row widths
  int gs_split = 3;
  // group iterations per work item of the plain unblocked path on graphs of <= kSmallNnz slots
  // with gs_split 1 / 3 (32 elsewhere).  A small graph's GraphSum lasts as long as its longest
  // item (one index -> gather round trip per iteration), so its long rows are cut short and
  // summed in-kernel or by workgroup items.  0 (default) = by shape with gs_split 3: the
  // shortest of 2, 4, 8, 16, 32 that leaves at most kWideCap workgroup items (r04 late: cora 224
  // rows at 2 iterations, 11.5k vs 11.1k epochs/s at 8; pubmed_synth 3,215 rows at 2 lost 2 %,
  // 1,321 at 4 gained 1 %: profiles/r04/ab_item_iters.txt)
  int gs_item_iters = 0;
  // a column subset's unblocked plain GraphSum gathers the input's own rows through the original
  // column ids (1) instead of compacting them first (0)
  int gs_orig_cols = 1;
  // the blocked d = 16 path's kernel (GraphSchedule::gather16): 0 = by shape -- the interleaved
  // k_graphsum<4, 16> when a row's segment in a column block averages under 16 slots (r05 late,
  // one call: reddit-11.6M, ~12 slots, 341 vs 595 us; reddit-114M, ~60 slots, k_graphsum16 1,016
  // vs 1,089 us; profiles/r05/y, z), 1 = k_graphsum16, 2 = the interleaved kernel
  int gs16_gather = 0;
  // ring schedule: rowsets in lockstep pairs (build_ring_host)
  int ring_pair = 0;
  // ring schedule: slices a visit reads; 0 = by shape (ring_window_for), 2 or 3
  int ring_window = 0;
  // ---- process scope
  // host threads of Parser::parse (0 = up to 16); the loader has no engine to carry it
  int parse_threads = 0;
  // 1 = the loader + MFMA-wave kernels of k_xstream_lds.hip for the X-stream products where
  // they apply (default), 0 = the register-streamed k_xstream_nn / k_xstream_tn (the
  // oracle-tested fallback of every other width); read in xstream_ring_ok (see the table)
  int xstream_ring = 1;
};

enum class KnobScope { Engine, Graph, Process };
// One row per knob: accepted values are allowed[0 .. n_allowed), or lo .. hi with no list
struct KnobRow {
  const char *name;
  int Knobs::*field;
  KnobScope scope;
  int lo, hi, n_allowed, allowed[7];
  bool accepts(int v) const;
};
extern const KnobRow kKnobTable[];
extern const int kKnobCount;
const KnobRow *find_knob(const char *name);  // null: no such knob
Knobs &process_knobs();

}  // namespace pgcn
