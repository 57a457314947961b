// parallel-gcn_amd/csrc/k_heur.hip -- the neighbourhood link heuristics for gfx950 (the reference
// has no pair-level model): Common Neighbours, Adamic-Adar and Resource Allocation over a cleaned
// CSR pattern (CnIndexDev, host/graph.hpp), as exact unsigned 64-bit fixed-point sums
//     S(a, v) = sum over z in G(a) & G(v) of w(z)
// with G(u) the ascending distinct neighbours of u other than u and w one of three host-made
// weight tables (include/pgcn.h has the contract).  Integer addition does not depend on its order,
// so the pair kernel and the sweep give the same bits for the same (a, v), scores are compared with
// > and ==, and nothing here adds floats.
//
//   k_heur_pairs<GL, MODE>: a group of GL lanes per pair, 64 / GL pairs per wave (GL from the mean
//       row length, as k_link.hip picks its group from the width).  The lanes split the SHORTER of
//       the two rows, every lane searching the longer one for its entries and adding w[z] on a hit
//       to a 64-bit accumulator; an xor butterfly over the group's lanes sums them.  A long row
//       above kHeurHeadMin entries first has kHeurHead evenly spaced pivots staged in the group's
//       LDS: the search's top five levels then probe LDS and only the last log2(len / 32) global
//       memory.  MODE 0 serves explicit pairs (fx and / or float scores; also a rank call's
//       thresholds); MODE 1 is the rank call's filter
//       correction: a group per filter entry f of query e computes S(a_e, f) and takes what the
//       sweep counted for it out of the counts (integer atomics).
//   k_heur_sweep: persistent workgroups of 16 waves (a hub anchor's expansion is one workgroup's
//       work, and the adds wait on their returned values: more waves, more adds in flight), each
//       with a private dense row acc[n] (u64) and a touched
//       list [n] in the index's workspace; workgroup b serves queries b, b + grid, ...  Phase A
//       expands the anchor's 2-hop neighbourhood: waves take z in G(a) with w(z) != 0, lanes take
//       v in the reverse row of z and add w(z) to acc[v] with an integer atomic whose old value 0
//       marks the first touch (every weight added is positive), which appends v to the touched
//       list through an LDS counter.  After a barrier phase B swaps every touched acc[v] for 0 --
//       an atomic exchange, so the row's values come from where the adds went and the row is left
//       zeroed for the next query -- and counts S > T and S == T in registers, skipping the target;
//       the untouched nodes score 0 and join `equal` only when T == 0.  No workgroup waits for
//       another: a plain launch.
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"

namespace pgcn {

namespace {

typedef unsigned long long u64;

constexpr int kHeurThreads = 256;        // the pair kernel's workgroup
constexpr int kHeurSweepThreads = 1024;  // the sweep's: 16 waves share a query's expansion
constexpr int kHeurHead = 32;      // pivots a group stages of a long row
constexpr int kHeurHeadMin = 128;  // rows above this length are searched through the staged head

__device__ __forceinline__ int clamp_node(int v, int n) { return min(max(v, 0), n - 1); }

__device__ __forceinline__ float heur_float(u64 s, int kind) {
  return kind == kHeurCN ? (float)s : (float)((double)s * 0x1p-32);
}

// The group's sum S(a, v): every lane of the group returns it.  head: the group's kHeurHead LDS
// words.  All 256 threads of the workgroup call this together (two workgroup barriers inside);
// `live` is false for a group without a pair, which then adds nothing.
template <int GL>
__device__ __forceinline__ u64 heur_pair(const CnIndex &x, const u64 *__restrict__ w, bool live,
                                         int a, int v, int li, int *head) {
  int sb = 0, sl = 0, lb = 0, ll = 0;
  if (live) {
    const int ab = x.ptr[a], al = x.ptr[a + 1] - ab, vb = x.ptr[v], vl = x.ptr[v + 1] - vb;
    const bool a_short = al <= vl;
    sb = a_short ? ab : vb;
    sl = a_short ? al : vl;
    lb = a_short ? vb : ab;
    ll = a_short ? vl : al;
  }
  const int *__restrict__ lrow = x.idx + lb;
  // the staged head: pivot j = lrow[j * step], INT_MAX behind the row's end
  const bool staged = ll > kHeurHeadMin;
  const int step = (ll + kHeurHead - 1) / kHeurHead;
  if (staged)
    for (int j = li; j < kHeurHead; j += GL) {
      const long long p = (long long)j * step;
      head[j] = p < ll ? lrow[p] : 0x7fffffff;
    }
  __syncthreads();
  u64 acc = 0;
  for (int k = li; k < sl; k += GL) {
    const int z = x.idx[sb + k];
    int lo = 0, hi = ll;  // the entry, if present, lies in [lo, hi)
    if (staged) {
      // the last pivot <= z (pivot 0 is the row's first entry)
      int pl = 0, ph = kHeurHead;
      while (ph - pl > 1) {
        const int mid = (pl + ph) >> 1;
        if (head[mid] <= z) pl = mid; else ph = mid;
      }
      lo = pl * step;
      hi = min(ll, lo + step);
    }
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const int c = lrow[mid];
      if (c < z) lo = mid + 1; else hi = mid;
    }
    if (lo < ll && lrow[lo] == z) acc += w[z];
  }
  __syncthreads();  // (the head is free for the group's next pair)
#pragma unroll
  for (int off = 1; off < GL; off <<= 1) acc += __shfl_xor(acc, off, kWave);
  return acc;
}

}  // namespace

template <int GL, int MODE>
__global__ __launch_bounds__(kHeurThreads) void k_heur_pairs(CnIndex x, int kind, HeurPairs p) {
  constexpr int kGroups = kHeurThreads / GL;
  __shared__ int heads[kGroups * kHeurHead];
  const int grp = threadIdx.x / GL, li = threadIdx.x % GL;
  const u64 *__restrict__ w = x.w[kind - 1];
  const long long stride = (long long)gridDim.x * kGroups;
  // (the trip count is the same for every thread of a workgroup: heur_pair holds barriers)
  for (long long base = (long long)blockIdx.x * kGroups; base < p.m; base += stride) {
    const long long e = base + grp;
    const bool live = e < p.m;
    int a = 0, v = 0, q = 0;
    if (MODE == 0) {
      if (live) {
        a = clamp_node(p.src[e], x.n);
        v = clamp_node(p.dst[e], x.n);
      }
    } else if (live) {
      // the query of filter entry e: the last q with filter_ptr[q] <= e
      int lo = 0, hi = p.n_queries;
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (p.filter_ptr[mid] <= e) lo = mid; else hi = mid;
      }
      q = lo;
      a = p.src[q];
      v = p.filter_idx[e];
    }
    const u64 s = heur_pair<GL>(x, w, live, a, v, li, heads + grp * kHeurHead);
    if (!live || li != 0) continue;
    if (MODE == 0) {
      if (p.fx) p.fx[e] = s;
      if (p.scores) p.scores[e] = heur_float(s, kind);
    } else {
      const u64 t = p.thr[q];
      if (s > t) atomicSub(p.greater + q, 1u);
      if (s == t) atomicSub(p.equal + q, 1u);
    }
  }
}

__global__ __launch_bounds__(kHeurSweepThreads) void k_heur_sweep(
    CnIndex x, int kind, const int *__restrict__ anchor, const int *__restrict__ target,
    const u64 *__restrict__ thr, int Q, unsigned *__restrict__ greater,
    unsigned *__restrict__ equal) {
  constexpr int kWaves = kHeurSweepThreads / kWave;
  __shared__ int s_cnt;
  __shared__ unsigned s_red[kWaves][3];
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const u64 *__restrict__ w = x.w[kind - 1];
  u64 *acc = x.acc + (size_t)blockIdx.x * x.n;
  int *touched = x.touched + (size_t)blockIdx.x * x.n;
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  for (int q = blockIdx.x; q < Q; q += gridDim.x) {
    const int a = anchor[q], t = target[q];
    const u64 T = thr[q];
    // phase A: acc[v] += w(z) over z in G(a), v in the reverse row of z
    for (int k = x.ptr[a] + wave; k < x.ptr[a + 1]; k += kWaves) {
      const int z = x.idx[k];
      const u64 wz = w[z];
      if (wz == 0) continue;
      for (int j = x.tptr[z] + lane; j < x.tptr[z + 1]; j += kWave) {
        const int v = x.tidx[j];
        if (atomicAdd(acc + v, wz) == 0) touched[atomicAdd(&s_cnt, 1)] = v;
      }
    }
    __syncthreads();
    // phase B: the touched nodes' scores against T; the row goes back to zero
    const int c = s_cnt;
    unsigned cg = 0u, ce = 0u, seen_t = 0u;
    for (int i = tid; i < c; i += kHeurSweepThreads) {
      const int v = touched[i];
      const u64 s = atomicExch(acc + v, 0ull);
      if (v == t) {
        seen_t = 1u;
      } else {
        cg += s > T ? 1u : 0u;
        ce += s == T ? 1u : 0u;
      }
    }
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      cg += __shfl_xor(cg, off, kWave);
      ce += __shfl_xor(ce, off, kWave);
      seen_t += __shfl_xor(seen_t, off, kWave);
    }
    if (lane == 0) {
      s_red[wave][0] = cg;
      s_red[wave][1] = ce;
      s_red[wave][2] = seen_t;
    }
    __syncthreads();
    if (tid == 0) {
      unsigned g = 0u, e = 0u, st = 0u;
      for (int k = 0; k < kWaves; k++) {
        g += s_red[k][0];
        e += s_red[k][1];
        st += s_red[k][2];
      }
      // the untouched nodes score 0: n - touched, less the target when it is one of them
      if (T == 0) e += (unsigned)(x.n - c) - (st ? 0u : 1u);
      greater[q] = g;
      equal[q] = e;
      s_cnt = 0;
    }
    __syncthreads();
  }
}

int heur_group(long long nnz, int n) {
  const long long mean = nnz / std::max(n, 1);
  return mean <= 16 ? 8 : mean <= 64 ? 16 : mean <= 256 ? 32 : 64;
}

int heur_workgroups(int n) {
  const long long per = (long long)std::max(n, 1) * (long long)(sizeof(u64) + sizeof(int));
  return (int)std::max<long long>(1, std::min<long long>(2 * kCUs, kHeurWorkspaceBudget / per));
}

namespace {
template <int MODE>
void launch_pairs(const CnIndex &x, int kind, const HeurPairs &p, hipStream_t s) {
  const int groups = kHeurThreads / x.group;
  const unsigned grid =
      (unsigned)std::min<long long>(ceil_div(p.m, groups), (long long)32 * kCUs);
#define HEUR_PAIRS(GL)                                                                      \
  PGCN_LAUNCH((k_heur_pairs<GL, MODE>), dim3(grid), dim3(kHeurThreads), 0, s, x, kind, p)
  switch (x.group) {
    case 8: HEUR_PAIRS(8); break;
    case 16: HEUR_PAIRS(16); break;
    case 32: HEUR_PAIRS(32); break;
    default: HEUR_PAIRS(64); break;
  }
#undef HEUR_PAIRS
}
}  // namespace

void launch_heur_score(const CnIndex &x, int kind, const int *src, const int *dst, long long m,
                       unsigned long long *fx, float *scores, hipStream_t s) {
  PGCN_CHECK(kind >= kHeurCN && kind <= kHeurRA && m >= 0 && (fx || scores), PGCN_E_INVALID,
             "link_heur_score: kind 1..3, fx or scores");
  if (m == 0) return;
  HeurPairs p;
  p.src = src;
  p.dst = dst;
  p.m = m;
  p.fx = fx;
  p.scores = scores;
  launch_pairs<0>(x, kind, p, s);
}

void launch_heur_rank(const CnIndex &x, int kind, const RankQueries &q, unsigned *greater,
                      unsigned *equal, hipStream_t s) {
  PGCN_CHECK(kind >= kHeurCN && kind <= kHeurRA && q.n == x.n && q.n_queries >= 0, PGCN_E_INVALID,
             "link_heur_rank: kind 1..3, a query set over the index's nodes");
  if (q.n_queries == 0) return;
  const int Q = q.n_queries;
  u64 *thr = q.thr_u64();
  HeurPairs p;
  p.src = q.anchor;
  p.dst = q.target;
  p.m = Q;
  p.fx = thr;
  launch_pairs<0>(x, kind, p, s);  // (the sweep stores both counts of every query: no zeroing)
  const unsigned grid = (unsigned)std::min(Q, x.workgroups);
  PGCN_LAUNCH(k_heur_sweep, dim3(grid), dim3(kHeurSweepThreads), 0, s, x, kind, q.anchor,
              q.target, thr, Q, greater, equal);
  if (q.filter_ptr && q.n_filter > 0) {
    HeurPairs f;
    f.src = q.anchor;
    f.m = q.n_filter;
    f.n_queries = Q;
    f.filter_ptr = q.filter_ptr;
    f.filter_idx = q.filter_idx;
    f.thr = thr;
    f.greater = greater;
    f.equal = equal;
    launch_pairs<1>(x, kind, f, s);
  }
}

}  // namespace pgcn
