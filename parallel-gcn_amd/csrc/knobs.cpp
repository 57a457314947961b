// parallel-gcn_amd/csrc/knobs.cpp -- the knob table (knobs.hpp).
#include "knobs.hpp"

#include <algorithm>
#include <climits>
#include <cstring>

namespace pgcn {
static constexpr KnobScope E = KnobScope::Engine, G = KnobScope::Graph, P = KnobScope::Process;
#define PGCN_KNOB(field, scope, lo, hi) {#field, &Knobs::field, scope, lo, hi, 0, {}}
#define PGCN_KNOB_LIST(field, scope, n, ...) {#field, &Knobs::field, scope, 0, 0, n, {__VA_ARGS__}}
const KnobRow kKnobTable[] = {
    PGCN_KNOB(train_ahead, E, 0, 1),
    PGCN_KNOB(split_rows, E, 0, 1),
    PGCN_KNOB(split_cols, E, 0, 1),
    PGCN_KNOB(eval_ax, E, 0, 1),
    PGCN_KNOB(epoch_graph, E, 0, 1),
    PGCN_KNOB(fuse_epilogue, E, 0, 15),
    PGCN_KNOB(fuse_output, E, 0, 3),
    PGCN_KNOB(mm_side, E, 0, 2),
    PGCN_KNOB(eval_tail, E, 0, 1),
    PGCN_KNOB(co_draw, E, 0, 2),
    PGCN_KNOB(sparse_dual, E, 0, 1),
    PGCN_KNOB(tn_fold, E, 0, 1),
    PGCN_KNOB(fuse_finish, E, 0, 2),
    PGCN_KNOB(mask_per, E, 0, 2),
    PGCN_KNOB(csc_tree, E, 0, 1),
    PGCN_KNOB(mask_adam, E, 0, 1),
    PGCN_KNOB(mask_xstream, E, 0, 1),
    PGCN_KNOB(reassoc_small, E, 0, 1),
    PGCN_KNOB(defer_wgrad, E, 0, 1),
    PGCN_KNOB(peer_uncached, E, 0, 1),
    PGCN_KNOB(lds_min_kb, G, INT_MIN, INT_MAX),  // < 0: the default
    PGCN_KNOB_LIST(lds_blocks, G, 7, 0, 1, 2, 4, 8, 16, 32),
    PGCN_KNOB(gs_split, G, 0, 3),
    PGCN_KNOB_LIST(gs_item_iters, G, 6, 0, 2, 4, 8, 16, 32),
    PGCN_KNOB(gs_orig_cols, G, 0, 1),
    PGCN_KNOB(gs16_gather, G, 0, 2),
    PGCN_KNOB(ring_pair, G, 0, 1),
    PGCN_KNOB_LIST(ring_window, G, 3, 0, 2, 3),
    PGCN_KNOB(parse_threads, P, 0, 4096),
    // process scope: read in xstream_ring_ok (k_xstream_lds.hip), the launcher dispatch that the
    // bare C-ABI GEMM entries share with the engine (threading it through launch_gemm_nn ->
    // launch_xstream_nn is left for later)
    PGCN_KNOB(xstream_ring, P, 0, 1),
};
#undef PGCN_KNOB
#undef PGCN_KNOB_LIST
const int kKnobCount = (int)(sizeof(kKnobTable) / sizeof(kKnobTable[0]));

bool KnobRow::accepts(int v) const {
  if (!n_allowed) return v >= lo && v <= hi;
  return std::find(allowed, allowed + n_allowed, v) != allowed + n_allowed;
}

const KnobRow *find_knob(const char *name) {
  for (int i = 0; i < kKnobCount; i++)
    if (!std::strcmp(kKnobTable[i].name, name)) return &kKnobTable[i];
  return nullptr;
}

Knobs &process_knobs() {
  static Knobs k;
  return k;
}

}  // namespace pgcn
