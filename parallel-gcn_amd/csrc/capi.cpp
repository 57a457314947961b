// parallel-gcn_amd/csrc/capi.cpp -- the extern "C" boundary declared in include/pgcn.h.
#include <atomic>
#include <climits>
#include <cstring>
#include <memory>

#include "../../include/pgcn.h"
#include "common.hpp"
#include "host/checkpoint.hpp"
#include "host/comm.hpp"
#include "host/data.hpp"
#include "host/gcn.hpp"
#include "host/graph.hpp"
#include "kernels.hpp"
#include "knobs.hpp"
#include "rng.hpp"

#include <cmath>

using namespace pgcn;

namespace pgcn {
namespace {
std::atomic<long long> g_path_hits[KP_COUNT];
thread_local long long t_path_hits[KP_COUNT];  // the launching host thread's (loopback ranks)
const char *const kPathNames[KP_COUNT] = {"xs_nn_ring", "xs_tn_ring", "xs_nn",   "xs_tn",
                                          "gs_ring",    "gs_gather",  "out_xent", "gemm_nn",
                                          "gemm_tn",    "gemm_nn_w",  "gemm_tn_w", "gat_fwd",
                                          "gat_bwd",    "gat_heads",  "spmm_csr",
                                          "spmm_csr_dual", "spmm_csc_256", "spmm_csc_1024",
                                          "spmm_tree_256", "spmm_tree_1024", "launches",
                                          "link_fwd",   "link_bwd",   "rank_sweep",
                                          "rank_filter", "topk_sweep", "topk_merge"};
}  // namespace
void note_path(KernelPath p) {
  g_path_hits[p].fetch_add(1, std::memory_order_relaxed);
  t_path_hits[p]++;
}
}  // namespace pgcn

struct pgcn_graph {
  std::unique_ptr<DevGraph> g;
};
struct pgcn_links {
  std::unique_ptr<LinkIndexDev> l;
};
struct pgcn_rank_queries {
  std::unique_ptr<RankQueriesDev> q;
};
struct pgcn_topk_queries {
  std::unique_ptr<TopKQueriesDev> q;
};
struct pgcn_gcn {
  std::unique_ptr<GCN> g;
};
struct pgcn_dataset {
  GCNData d;
};
struct pgcn_loopback {
  std::shared_ptr<LoopbackGroup> g;
};

namespace {
void check_device() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    throw Error(PGCN_E_NODEVICE, "no HIP device visible: the engine has no CPU fallback");
}

// the edge-cut creators: attention (a row's softmax needs all its columns) and the SAGE
// aggregators run on one GPU only
void refuse_single_gpu_only(const pgcn_params *p) {
  PGCN_CHECK(!p->attention, PGCN_E_INVALID,
             "attention: single GPU only (edge-cut attention is not supported)");
  // (the mean is linear and could be partitioned; the max needs a max / arg exchange)
  PGCN_CHECK(!p->aggregator && !p->root_weight, PGCN_E_INVALID,
             "aggregator: single GPU only (edge-cut SAGE layers are not supported)");
  // (a graph's rows may lie on several ranks: its readout would need an exchange of its own)
  PGCN_CHECK(!p->readout, PGCN_E_INVALID,
             "readout: single GPU only (edge-cut graph classification is not supported)");
  // (a pair's endpoints may lie on two ranks: its score would need an exchange of its own)
  PGCN_CHECK(!p->link_decoder, PGCN_E_INVALID,
             "link_decoder: single GPU only (edge-cut link prediction is not supported)");
}

GCNParams to_params(const pgcn_params *p, const pgcn_data *d) {
  GCNParams q;
  q.num_nodes = d->num_nodes;
  q.input_dim = p->input_dim;
  q.output_dim = p->output_dim;
  q.n_layers = p->n_layers;
  q.hidden_dims.assign(p->hidden_dims, p->hidden_dims + std::max(0, p->n_layers - 1));
  q.dropouts.assign(p->dropouts, p->dropouts + std::max(0, p->n_layers));
  q.epochs = p->epochs;
  q.early_stopping = p->early_stopping;
  q.reassociate_last = p->reassociate_last != 0;
  q.seed = p->seed;
  q.residual = p->residual != 0;
  q.layer_norm = p->layer_norm != 0;
  q.multilabel = p->multilabel != 0;
  q.attention = p->attention != 0;
  q.attention_heads = p->attention_heads == 0 ? 1 : p->attention_heads;
  q.attention_dropout = p->attention_dropout;
  PGCN_CHECK(p->root_weight == 0 || p->root_weight == 1, PGCN_E_INVALID,
             "root_weight must be 0 or 1");
  q.aggregator = p->aggregator;
  q.root_weight = p->root_weight != 0;
  PGCN_CHECK(p->readout >= kReadoutNone && p->readout <= kReadoutMax, PGCN_E_INVALID,
             "readout must be 0 (none), 1 (sum), 2 (mean) or 3 (max)");
  PGCN_CHECK(!p->readout || !p->multilabel, PGCN_E_INVALID,
             "readout cannot be combined with multilabel");
  q.readout = p->readout;
  PGCN_CHECK(p->link_decoder == 0 || p->link_decoder == 1, PGCN_E_INVALID,
             "link_decoder must be 0 (none) or 1 (dot product)");
  PGCN_CHECK(!p->link_decoder || (!p->multilabel && !p->readout), PGCN_E_INVALID,
             "link_decoder cannot be combined with multilabel or readout");
  q.link_decoder = p->link_decoder;
  return q;
}
AdamParams to_adam(const pgcn_params *p) {
  AdamParams a;
  a.learning_rate = p->learning_rate;
  a.weight_decay = p->weight_decay;
  a.beta1 = p->beta1;
  a.beta2 = p->beta2;
  a.eps = p->eps;
  return a;
}
// GCNData view -> owned GCNData (the engine uploads from it once)
GCNData to_data(const pgcn_data *d, const pgcn_params *p) {
  GCNData g;
  const int n = d->num_nodes;
  g.num_nodes = n;
  g.input_dim = p->input_dim;
  g.output_dim = p->output_dim;
  g.graph.indptr.assign(d->graph_indptr, d->graph_indptr + n + 1);
  g.graph.indices.assign(d->graph_indices, d->graph_indices + d->graph_indptr[n]);
  g.feature_index.indptr.assign(d->feat_indptr, d->feat_indptr + n + 1);
  g.feature_index.indices.assign(d->feat_indices, d->feat_indices + d->feat_indptr[n]);
  g.feature_value.assign(d->feat_values, d->feat_values + d->feat_indptr[n]);
  g.label.assign(d->label, d->label + n);
  g.split.assign(d->split, d->split + n);
  if (p->multilabel) {  // (the two trailing members are read only then)
    PGCN_CHECK(d->label_bits, PGCN_E_INVALID, "multilabel: pgcn_data.label_bits is required");
    PGCN_CHECK(p->output_dim >= 1 && p->output_dim <= 128 &&
                   d->label_words == (p->output_dim + 31) / 32,
               PGCN_E_INVALID,
               "multilabel: 1 <= output_dim <= 128 and label_words = ceil(output_dim / 32)");
    g.label_words = d->label_words;
    g.label_bits.assign(d->label_bits, d->label_bits + (size_t)n * d->label_words);
  }
  if (p->readout) {  // (the graph members are read only then)
    PGCN_CHECK(d->num_graphs >= 1 && d->graph_ptr && d->graph_label && d->graph_split,
               PGCN_E_INVALID, "readout: pgcn_data has no graphs attached");
    PGCN_CHECK(graphs_valid(n, d->num_graphs, d->graph_ptr, d->graph_label, d->graph_split,
                            p->output_dim),
               PGCN_E_INVALID,
               "readout: graph_ptr from 0 to num_nodes, labels in [-1, output_dim), splits 0..3");
    const size_t G = (size_t)d->num_graphs;
    g.num_graphs = d->num_graphs;
    g.graph_ptr.assign(d->graph_ptr, d->graph_ptr + G + 1);
    g.graph_label.assign(d->graph_label, d->graph_label + G);
    g.graph_split.assign(d->graph_split, d->graph_split + G);
  }
  if (p->link_decoder) {  // (the pair members are read only then)
    PGCN_CHECK(d->num_pairs >= 1 && d->pair_src && d->pair_dst && d->pair_label && d->pair_split,
               PGCN_E_INVALID, "link_decoder: pgcn_data has no pairs attached");
    PGCN_CHECK(links_valid(n, d->num_pairs, d->pair_src, d->pair_dst, d->pair_label,
                           d->pair_split),
               PGCN_E_INVALID,
               "link_decoder: endpoints in [0, num_nodes), labels -1 / 0 / 1, splits 0..3");
    const size_t E = (size_t)d->num_pairs;
    g.pair_src.assign(d->pair_src, d->pair_src + E);
    g.pair_dst.assign(d->pair_dst, d->pair_dst + E);
    g.pair_label.assign(d->pair_label, d->pair_label + E);
    g.pair_split.assign(d->pair_split, d->pair_split + E);
  }
  return g;
}
}  // namespace

extern "C" {

const char *pgcn_status_string(int s) {
  switch (s) {
    case PGCN_OK: return "ok";
    case PGCN_E_INVALID: return "invalid argument";
    case PGCN_E_NOMEM: return "out of device memory";
    case PGCN_E_IO: return "cannot read input";
    case PGCN_E_COMM: return "RCCL error";
    case PGCN_E_NODEVICE: return "no HIP device";
    default: return s > 0 ? hipGetErrorString((hipError_t)s) : "unknown";
  }
}

int pgcn_version(void) { return 112; }

// ---------------------------------------------------------------- graph + kernels
int pgcn_graph_create(int n, const int *indptr, const int *indices, pgcn_graph **out) {
  return guarded([&] {
    PGCN_CHECK(n > 0 && indptr && indices && out, PGCN_E_INVALID, "graph_create args");
    check_device();
    std::vector<float> v = graph_coefs(n, indptr, indices);
    auto h = std::make_unique<pgcn_graph>();
    h->g = std::make_unique<DevGraph>(n, n, indptr, indices, v.data());
    std::vector<float> sc = degree_scales(n, indptr);
    h->g->set_scales(sc, sc);
    *out = h.release();
  });
}
int pgcn_graph_create_values(int n, const int *indptr, const int *indices, const float *values,
                             pgcn_graph **out) {
  return guarded([&] {
    PGCN_CHECK(n > 0 && indptr && indices && values && out, PGCN_E_INVALID,
               "graph_create_values args");
    PGCN_CHECK(indptr[0] == 0 && indptr[n] >= 0, PGCN_E_INVALID, "graph_create_values: indptr");
    for (int i = 0; i < n; i++)
      PGCN_CHECK(indptr[i + 1] >= indptr[i], PGCN_E_INVALID, "graph_create_values: indptr order");
    for (long long k = 0; k < indptr[n]; k++)
      PGCN_CHECK(indices[k] >= 0 && indices[k] < n, PGCN_E_INVALID,
                 "graph_create_values: column id out of range");
    check_device();
    auto h = std::make_unique<pgcn_graph>();
    h->g = std::make_unique<DevGraph>(n, n, indptr, indices, values);
    // the parser's coefficients exactly: the factorised LDS path applies
    const std::vector<float> coef = graph_coefs(n, indptr, indices);
    if (std::memcmp(coef.data(), values, coef.size() * sizeof(float)) == 0) {
      std::vector<float> sc = degree_scales(n, indptr);
      h->g->set_scales(sc, sc);
    }
    *out = h.release();
  });
}

int pgcn_debug_rank_graph(int n, const int *indptr, const int *indices, int world, int rank,
                          int chunks, int chunk, pgcn_graph **out, int *rows, int *cols) {
  return guarded([&] {
    PGCN_CHECK(n > 0 && indptr && indices && out && world >= 1 && rank >= 0 && rank < world &&
                   chunks >= 1 && chunk >= 0 && chunk < chunks,
               PGCN_E_INVALID, "rank_graph args");
    check_device();
    const Partition part = make_partition(n, indptr, world, rank, chunks);
    const std::vector<float> sg = degree_scales(n, indptr);
    const int h = part.chunk_rows();
    std::vector<int> sp, si;
    partition_subgraph_chunk(part, n, indptr, indices, chunk, &sp, &si);
    // the same values and scales as GCN::build's chunk graphs
    std::vector<float> rs((size_t)part.world * h, 0.0f), cs((size_t)part.local_rows()), sv(si.size());
    for (int c = 0; c < part.local_rows(); c++) cs[(size_t)c] = sg[(size_t)part.first() + c];
    for (int q = 0; q < part.world; q++)
      for (int j = 0; j < h; j++) {
        const int i = part.bounds[(size_t)q] + chunk * h + j;
        if (i >= part.bounds[(size_t)q + 1]) continue;
        const size_t r = (size_t)q * h + j;
        rs[r] = sg[(size_t)i];
        for (int t = sp[r]; t < sp[r + 1]; t++) {
          const int gj = part.first() + si[(size_t)t];
          sv[(size_t)t] = graph_coef(indptr[i + 1] - indptr[i], indptr[gj + 1] - indptr[gj]);
        }
      }
    auto g = std::make_unique<pgcn_graph>();
    g->g = std::make_unique<DevGraph>(part.world * h, part.local_rows(), sp.data(), si.data(),
                                      sv.data());
    g->g->set_scales(std::move(rs), cs);
    if (rows) *rows = part.world * h;
    if (cols) *cols = part.local_rows();
    *out = g.release();
  });
}

int pgcn_graph_destroy(pgcn_graph *g) {
  delete g;
  return PGCN_OK;
}
long long pgcn_graph_nnz(const pgcn_graph *g) { return g ? g->g->nnz() : -1; }

int pgcn_graphsum(const pgcn_graph *g, const float *in, int ld_in, float *out, int ld_out,
                  int dim, void *stream) {
  return guarded([&] {
    PGCN_CHECK(g && in && out && dim > 0, PGCN_E_INVALID, "graphsum args");
    g->g->graphsum(in, ld_in, out, ld_out, dim, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_gemm(int M, int N, int K, const float *A, int lda, const float *B, int ldb, int trans_b,
              float *C, int ldc, const uint64_t *a_mask, long long mask_base, long long mask_ld,
              float a_scale, void *stream) {
  return guarded([&] {
    PGCN_CHECK(A && B && C && M >= 0 && K > 0 && ldc >= N, PGCN_E_INVALID, "gemm args");
    launch_gemm_nn(M, N, K, A, lda, B, ldb, trans_b, C, ldc, a_mask, mask_base, mask_ld, a_scale,
                   as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

size_t pgcn_gemm_tn_workspace(int M, int N, int K) { return gemm_tn_workspace(M, N, K); }

int pgcn_gemm_tn(int M, int N, int K, const float *A, int lda, const float *G, int ldg, float *C,
                 int ldc, const uint64_t *a_mask, long long mask_base, long long mask_ld,
                 float a_scale, void *workspace, void *stream) {
  return guarded([&] {
    PGCN_CHECK(A && G && C && workspace && K > 0 && ldc >= N, PGCN_E_INVALID, "gemm_tn args");
    launch_gemm_tn(M, N, K, A, lda, G, ldg, C, ldc, a_mask, mask_base, mask_ld, a_scale,
                   workspace, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_mask_nibbles(const uint64_t *mask, long long mask_base, long long mask_ld, int M, int K,
                      uint64_t *out, void *stream) {
  return guarded([&] {
    PGCN_CHECK(mask && out && M >= 0 && K > 0, PGCN_E_INVALID, "mask_nibbles args");
    launch_mask_nibbles(mask, mask_base, mask_ld, M, K, out, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_gemm_xstream(int M, int N, int K, const float *A, int lda, const float *B, int ldb,
                      int trans_b, float *C, int ldc, const uint64_t *mask_nib, float a_scale,
                      void *stream) {
  return guarded([&] {
    PGCN_CHECK(A && B && C && M >= 0 && ldc >= N, PGCN_E_INVALID, "gemm_xstream args");
    launch_xstream_nn(M, N, K, A, lda, B, ldb, trans_b, C, ldc, mask_nib, a_scale,
                      as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_gemm_xstream_dual(int M, int N, int K, const float *A, int lda, const float *B, int ldb,
                           int trans_b, float *C, float *C2, int ldc, const uint64_t *mask_nib,
                           float a_scale, void *stream) {
  return guarded([&] {
    PGCN_CHECK(A && B && C && C2 && mask_nib && M >= 0 && ldc >= N, PGCN_E_INVALID,
               "gemm_xstream_dual args");
    launch_xstream_nn(M, N, K, A, lda, B, ldb, trans_b, C, ldc, mask_nib, a_scale,
                      as_stream(stream), C2);
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_gemm_tn_xstream(int M, int N, int K, const float *A, int lda, const float *G, int ldg,
                         float *C, int ldc, const uint64_t *mask_nib, float a_scale,
                         void *workspace, void *stream) {
  return guarded([&] {
    PGCN_CHECK(A && G && C && workspace && M >= 0 && ldc >= N, PGCN_E_INVALID,
               "gemm_tn_xstream args");
    launch_xstream_tn(M, N, K, A, lda, G, ldg, C, ldc, mask_nib, a_scale, workspace,
                      as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_gemm_xstream_flat(int M, int N, int K, const float *A, int lda, const float *B, int ldb,
                           int trans_b, float *C, float *C2, int ldc, const uint64_t *mask,
                           long long mask_base, long long mask_words, float a_scale,
                           void *stream) {
  return guarded([&] {
    PGCN_CHECK(A && B && C && mask && mask_words > 0 && mask_base >= 0 && M >= 0 && ldc >= N &&
                   xstream_ring_ok(K, lda),
               PGCN_E_INVALID, "gemm_xstream_flat args");
    const XsMask fm{mask, mask_base, K, mask_words};
    launch_xstream_nn(M, N, K, A, lda, B, ldb, trans_b, C, ldc, nullptr, a_scale,
                      as_stream(stream), C2, nullptr, &fm);
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_gemm_tn_xstream_flat(int M, int N, int K, const float *A, int lda, const float *G, int ldg,
                              float *C, int ldc, const uint64_t *mask, long long mask_base,
                              long long mask_words, float a_scale, void *workspace, void *stream) {
  return guarded([&] {
    PGCN_CHECK(A && G && C && workspace && mask && mask_words > 0 && mask_base >= 0 && M >= 0 &&
                   ldc >= N && xstream_ring_ok(K, lda),
               PGCN_E_INVALID, "gemm_tn_xstream_flat args");
    const XsMask fm{mask, mask_base, K, mask_words};
    launch_xstream_tn(M, N, K, A, lda, G, ldg, C, ldc, nullptr, a_scale, workspace,
                      as_stream(stream), &fm);
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_spmm_csr(int m, int p, const int *indptr, const int *indices, const float *a,
                  const uint64_t *a_mask, float a_scale, const float *b, float *c, void *stream) {
  return guarded([&] {
    launch_spmm_csr(m, p, p, indptr, indices, a, a_mask, 0, a_scale, b, c, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_spmm_csc_bwd(int nf, int p, const int *csc_ptr, const int *csc_row, const int *csc_pos,
                      const float *a, const uint64_t *a_mask, float a_scale, const float *cgrad,
                      float *bgrad, void *stream) {
  return guarded([&] {
    launch_spmm_csc_bwd(nf, p, p, csc_ptr, csc_row, csc_pos, a, a_mask, 0, a_scale, cgrad, bgrad,
                        as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_csr_transpose(int m, int n_cols, const int *indptr, const int *indices, int *csc_ptr,
                       int *csc_row, int *csc_pos) {
  return guarded([&] {
    std::memset(csc_ptr, 0, sizeof(int) * (size_t)(n_cols + 1));
    for (int k = 0; k < indptr[m]; k++) {
      PGCN_CHECK(indices[k] >= 0 && indices[k] < n_cols, PGCN_E_INVALID, "column id");
      csc_ptr[indices[k] + 1]++;
    }
    for (int f = 0; f < n_cols; f++) csc_ptr[f + 1] += csc_ptr[f];
    std::vector<int> fill(csc_ptr, csc_ptr + n_cols);
    for (int i = 0; i < m; i++)
      for (int k = indptr[i]; k < indptr[i + 1]; k++) {
        const int o = fill[(size_t)indices[k]]++;
        csc_row[o] = i;
        csc_pos[o] = k;
      }
  });
}

int pgcn_dropout_mask(uint64_t *chunk_states, long long n_chunks, long long n_elems,
                      long long elem0, float p, uint64_t *mask, const void *dev_jump_table,
                      void *stream) {
  return guarded([&] {
    launch_dropout_mask(chunk_states, n_chunks, elem0, n_elems, p, mask, dev_jump_table,
                        as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_dropout_apply(float *x, long long n, const uint64_t *mask, float scale, void *stream) {
  return guarded([&] {
    launch_dropout_apply_based(x, n, mask, 0, scale, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_relu_fwd(float *x, long long n, uint8_t *mask, int training, void *stream) {
  return guarded([&] { launch_relu_fwd(x, n, mask, training, as_stream(stream)); });
}
int pgcn_relu_bwd(float *g, long long n, const uint8_t *mask, void *stream) {
  return guarded([&] { launch_relu_bwd(g, n, mask, as_stream(stream)); });
}
int pgcn_residual_fwd(float *cur, const float *prev, long long n, void *stream) {
  return guarded([&] {
    PGCN_CHECK(n >= 0 && (n == 0 || (cur && prev)), PGCN_E_INVALID, "residual_fwd args");
    check_device();
    launch_residual_fwd(cur, prev, n, as_stream(stream));
  });
}
int pgcn_residual_bwd(float *prev_grad, const float *cur_grad, long long n, void *stream) {
  return guarded([&] {
    PGCN_CHECK(n >= 0 && (n == 0 || (prev_grad && cur_grad)), PGCN_E_INVALID,
               "residual_bwd args");
    check_device();
    launch_residual_bwd(prev_grad, cur_grad, n, as_stream(stream));
  });
}


namespace {
bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool ln_ld_ok(int ld, int d) { return ld >= d && ld % 4 == 0; }
void layernorm_fwd_checked(const float *x, int ld_x, float *y, int ld_y, int n, int d,
                           const float *gamma, const float *beta, float eps, float *xhat,
                           int ld_xhat, float *rstd, const GsEpilogue *epi, void *stream) {
  PGCN_CHECK(n >= 0 && d >= 1 && d <= kLayerNormMaxWidth && ln_ld_ok(ld_x, d) && ln_ld_ok(ld_y, d),
             PGCN_E_INVALID, "layernorm_fwd: 1 <= d <= 1024, ld % 4 == 0, ld >= d");
  PGCN_CHECK(eps >= 0.0f && (xhat != nullptr) == (rstd != nullptr) &&
                 (!xhat || ln_ld_ok(ld_xhat, d)),
             PGCN_E_INVALID, "layernorm_fwd: xhat and rstd together, ld_xhat % 4 == 0 >= d");
  PGCN_CHECK(n == 0 || (x && y && gamma && beta && aligned16(x) && aligned16(y) && aligned16(xhat)),
             PGCN_E_INVALID, "layernorm_fwd: null or misaligned argument");
  if (epi && epi->mode) {
    PGCN_CHECK(ld_y == d && ln_ld_ok(epi->relu_ld, d) && (!epi->res || ln_ld_ok(epi->res_ld, d)) &&
                   aligned16(epi->res) && (reinterpret_cast<uintptr_t>(epi->relu_mask) & 3) == 0 &&
                   epi->drop_base >= 0,
               PGCN_E_INVALID, "layernorm_fwd_tail: the tail needs ld_y == d and padded strides");
  }
  check_device();
  if (n == 0) return;
  launch_layernorm_fwd(x, ld_x, y, ld_y, n, d, gamma, beta, eps, xhat, ld_xhat, rstd, epi,
                       as_stream(stream));
  PGCN_HIP(hipGetLastError());
}
}  // namespace

int pgcn_layernorm_fwd(const float *x, int ld_x, float *y, int ld_y, int n, int d,
                       const float *gamma, const float *beta, float eps, float *xhat,
                       int ld_xhat, float *rstd, void *stream) {
  return guarded([&] {
    layernorm_fwd_checked(x, ld_x, y, ld_y, n, d, gamma, beta, eps, xhat, ld_xhat, rstd, nullptr,
                          stream);
  });
}

int pgcn_debug_layernorm_fwd_tail(const float *x, int ld_x, float *y, int ld_y, int n, int d,
                                  const float *gamma, const float *beta, float eps, float *xhat,
                                  int ld_xhat, float *rstd, uint8_t *relu_mask, int relu_ld,
                                  const float *res, int res_ld, const uint64_t *drop_mask,
                                  long long drop_base, float drop_scale, void *stream) {
  return guarded([&] {
    GsEpilogue e;
    e.mode = 1;
    e.relu_mask = relu_mask;
    e.relu_ld = relu_ld;
    e.res = const_cast<float *>(res);  // (mode 1 reads it)
    e.res_ld = res_ld;
    e.drop_mask = drop_mask;
    e.drop_base = drop_base;
    e.drop_cols = d;
    e.drop_scale = drop_scale;
    layernorm_fwd_checked(x, ld_x, y, ld_y, n, d, gamma, beta, eps, xhat, ld_xhat, rstd, &e,
                          stream);
  });
}

size_t pgcn_layernorm_bwd_workspace(int n, int d) {
  if (n < 0 || d < 1 || d > kLayerNormMaxWidth) return 0;
  return layernorm_bwd_workspace(n, d);
}

int pgcn_layernorm_bwd(const float *dy, int ld_dy, const float *xhat, int ld_xhat,
                       const float *rstd, const float *gamma, int n, int d, float *dx, int ld_dx,
                       float *dgamma, float *dbeta, void *workspace, void *stream) {
  return guarded([&] {
    PGCN_CHECK(n >= 0 && d >= 1 && d <= kLayerNormMaxWidth && ln_ld_ok(ld_dy, d) &&
                   ln_ld_ok(ld_xhat, d) && ln_ld_ok(ld_dx, d),
               PGCN_E_INVALID, "layernorm_bwd: 1 <= d <= 1024, ld % 4 == 0, ld >= d");
    PGCN_CHECK(n == 0 || (dy && xhat && rstd && gamma && dx && dgamma && dbeta && workspace &&
                          aligned16(dy) && aligned16(xhat) && aligned16(dx)),
               PGCN_E_INVALID, "layernorm_bwd: null or misaligned argument");
    check_device();
    if (n == 0) return;
    launch_layernorm_bwd(dy, ld_dy, xhat, ld_xhat, rstd, gamma, n, d, dx, ld_dx, dgamma, dbeta,
                         workspace, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

namespace {
void check_gat_dims(int n, int d, std::initializer_list<int> lds) {
  PGCN_CHECK(n >= 0 && d >= 1 && d <= kGatMaxWidth, PGCN_E_INVALID, "gat: 1 <= d <= 128");
  for (int ld : lds) PGCN_CHECK(ln_ld_ok(ld, d), PGCN_E_INVALID, "gat: ld % 4 == 0, ld >= d");
}
}  // namespace

int pgcn_gat_scores(const float *P, int ld_p, int n, int d, const float *a_dst,
                    const float *a_src, float *u, float *v, void *stream) {
  return guarded([&] {
    check_gat_dims(n, d, {ld_p});
    PGCN_CHECK(n == 0 || (P && a_dst && a_src && u && v && aligned16(P)), PGCN_E_INVALID,
               "gat_scores: null or misaligned argument");
    if (n == 0) return;
    check_device();
    launch_gat_scores(P, ld_p, n, d, 1, a_dst, a_src, u, v, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_gat_fwd(const pgcn_graph *g, const float *P, int ld_p, const float *u, const float *v,
                 float slope, float *Z, int ld_z, int d, float *alpha, void *stream) {
  return guarded([&] {
    check_gat_dims(0, d, {ld_p, ld_z});
    PGCN_CHECK(g && g->g && P && u && v && Z && aligned16(P) && aligned16(Z), PGCN_E_INVALID,
               "gat_fwd: null or misaligned argument");
    PGCN_CHECK(g->g->rows() == g->g->cols(), PGCN_E_INVALID, "gat_fwd: square pattern");
    check_device();
    launch_gat_fwd(g->g->gat_pattern(), P, ld_p, u, v, slope, Z, ld_z, d, 1, nullptr, 0, 1.0f,
                   alpha, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

size_t pgcn_gat_bwd_workspace(const pgcn_graph *g, int d) {
  if (!g || !g->g || d < 1 || d > kGatMaxWidth || g->g->rows() != g->g->cols()) return 0;
  size_t bytes = 0;
  (void)guarded([&] { bytes = gat_bwd_workspace(g->g->gat_pattern(), d, 1); });
  return bytes;
}

int pgcn_gat_bwd(const pgcn_graph *g, const float *P, int ld_p, const float *u, const float *v,
                 float slope, const float *alpha, const float *Z, int ld_z, const float *G,
                 int ld_g, const float *a_dst, const float *a_src, float *dP, int ld_dp, int d,
                 float *da, void *workspace, void *stream) {
  return guarded([&] {
    check_gat_dims(0, d, {ld_p, ld_z, ld_g, ld_dp});
    PGCN_CHECK(g && g->g && P && u && v && alpha && Z && G && a_dst && a_src && dP && da &&
                   workspace && aligned16(P) && aligned16(Z) && aligned16(G) && aligned16(dP) &&
                   aligned16(workspace),
               PGCN_E_INVALID, "gat_bwd: null or misaligned argument");
    PGCN_CHECK(g->g->rows() == g->g->cols(), PGCN_E_INVALID, "gat_bwd: square pattern");
    check_device();
    launch_gat_bwd(g->g->gat_pattern(), P, ld_p, u, v, slope, alpha, Z, ld_z, G, ld_g, a_dst,
                   a_src, dP, ld_dp, d, 1, nullptr, 0, 1.0f, da, workspace, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

namespace {
// the head rules of the _mh entries, after check_gat_dims
void check_gat_heads(int d, int heads) {
  PGCN_CHECK(heads >= 1 && heads <= kGatMaxHeads, PGCN_E_INVALID, "gat: 1 <= heads <= 32");
  PGCN_CHECK(gat_heads_ok(d, heads), PGCN_E_INVALID,
             "gat: heads must divide d into widths of 4, 8, 16, 32, 64 or 128");
}
}  // namespace

int pgcn_gat_scores_mh(const float *P, int ld_p, int n, int d, int heads, const float *a_dst,
                       const float *a_src, float *u, float *v, void *stream) {
  return guarded([&] {
    check_gat_dims(n, d, {ld_p});
    check_gat_heads(d, heads);
    PGCN_CHECK(n == 0 || (P && a_dst && a_src && u && v && aligned16(P)), PGCN_E_INVALID,
               "gat_scores: null or misaligned argument");
    if (n == 0) return;
    check_device();
    launch_gat_scores(P, ld_p, n, d, heads, a_dst, a_src, u, v, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_gat_fwd_mh(const pgcn_graph *g, const float *P, int ld_p, const float *u, const float *v,
                    float slope, float *Z, int ld_z, int d, int heads, const uint64_t *drop_mask,
                    long long drop_base, float drop_scale, float *alpha, void *stream) {
  return guarded([&] {
    check_gat_dims(0, d, {ld_p, ld_z});
    check_gat_heads(d, heads);
    PGCN_CHECK(!drop_mask || (alpha && drop_base >= 0), PGCN_E_INVALID,
               "gat_fwd: a mask needs alpha (a training forward) and drop_base >= 0");
    PGCN_CHECK(g && g->g && P && u && v && Z && aligned16(P) && aligned16(Z), PGCN_E_INVALID,
               "gat_fwd: null or misaligned argument");
    PGCN_CHECK(g->g->rows() == g->g->cols(), PGCN_E_INVALID, "gat_fwd: square pattern");
    check_device();
    launch_gat_fwd(g->g->gat_pattern(), P, ld_p, u, v, slope, Z, ld_z, d, heads, drop_mask,
                   drop_base, drop_scale, alpha, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

size_t pgcn_gat_bwd_workspace_mh(const pgcn_graph *g, int d, int heads) {
  if (!g || !g->g || heads > kGatMaxHeads || !gat_heads_ok(d, heads) ||
      g->g->rows() != g->g->cols())
    return 0;
  size_t bytes = 0;
  (void)guarded([&] { bytes = gat_bwd_workspace(g->g->gat_pattern(), d, heads); });
  return bytes;
}

int pgcn_gat_bwd_mh(const pgcn_graph *g, const float *P, int ld_p, const float *u, const float *v,
                    float slope, const float *alpha, const float *Z, int ld_z, const float *G,
                    int ld_g, const float *a_dst, const float *a_src, float *dP, int ld_dp, int d,
                    int heads, const uint64_t *drop_mask, long long drop_base, float drop_scale,
                    float *da, void *workspace, void *stream) {
  return guarded([&] {
    check_gat_dims(0, d, {ld_p, ld_z, ld_g, ld_dp});
    check_gat_heads(d, heads);
    PGCN_CHECK(!drop_mask || drop_base >= 0, PGCN_E_INVALID, "gat_bwd: drop_base >= 0");
    PGCN_CHECK(g && g->g && P && u && v && alpha && Z && G && a_dst && a_src && dP && da &&
                   workspace && aligned16(P) && aligned16(Z) && aligned16(G) && aligned16(dP) &&
                   aligned16(workspace),
               PGCN_E_INVALID, "gat_bwd: null or misaligned argument");
    PGCN_CHECK(g->g->rows() == g->g->cols(), PGCN_E_INVALID, "gat_bwd: square pattern");
    check_device();
    launch_gat_bwd(g->g->gat_pattern(), P, ld_p, u, v, slope, alpha, Z, ld_z, G, ld_g, a_dst,
                   a_src, dP, ld_dp, d, heads, drop_mask, drop_base, drop_scale, da, workspace,
                   as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_graph_create_mean(int n, const int *indptr, const int *indices, int transpose,
                           pgcn_graph **out) {
  return guarded([&] {
    PGCN_CHECK(n > 0 && indptr && indices && out && (transpose == 0 || transpose == 1),
               PGCN_E_INVALID, "graph_create_mean args");
    PGCN_CHECK(indptr[0] == 0 && indptr[n] >= 0, PGCN_E_INVALID, "graph_create_mean: indptr");
    for (int i = 0; i < n; i++)
      PGCN_CHECK(indptr[i + 1] >= indptr[i], PGCN_E_INVALID, "graph_create_mean: indptr order");
    const int nnz = indptr[n];
    for (int k = 0; k < nnz; k++)
      PGCN_CHECK(indices[k] >= 0 && indices[k] < n, PGCN_E_INVALID,
                 "graph_create_mean: column id out of range");
    check_device();
    auto h = std::make_unique<pgcn_graph>();
    h->g = make_mean_graph(n, indptr, indices, transpose != 0);
    *out = h.release();
  });
}

namespace {
void check_sage_dims(int d, std::initializer_list<int> lds) {
  PGCN_CHECK(d >= 1 && d <= kSageMaxWidth, PGCN_E_INVALID, "agg_max: 1 <= d <= 128");
  for (int ld : lds) PGCN_CHECK(ln_ld_ok(ld, d), PGCN_E_INVALID, "agg_max: ld % 4 == 0, ld >= d");
}
}  // namespace

int pgcn_agg_max_fwd(const pgcn_graph *g, const float *in, int ld_in, int d, const float *add,
                     int ld_add, float *out, int ld_out, int *arg, int ld_arg, void *stream) {
  return guarded([&] {
    check_sage_dims(d, {ld_in, ld_out});
    if (add) check_sage_dims(d, {ld_add});
    if (arg) check_sage_dims(d, {ld_arg});
    PGCN_CHECK(g && g->g && in && out && aligned16(in) && aligned16(out) && aligned16(add) &&
                   aligned16(arg),
               PGCN_E_INVALID, "agg_max_fwd: null or misaligned argument");
    PGCN_CHECK(g->g->rows() == g->g->cols() && g->g->nnz() <= INT_MAX, PGCN_E_INVALID,
               "agg_max_fwd: square pattern, nnz within an int");
    check_device();
    const GatPattern &p = g->g->gat_pattern();
    launch_agg_max_fwd(p, g->g->sage_ws(), in, ld_in, d, add, ld_add, out, ld_out, arg, ld_arg,
                       as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_agg_max_bwd(const pgcn_graph *g, const float *G, int ld_g, const int *arg, int ld_arg,
                     int d, float *din, int ld_din, void *stream) {
  return guarded([&] {
    check_sage_dims(d, {ld_g, ld_arg, ld_din});
    PGCN_CHECK(g && g->g && G && arg && din && aligned16(G) && aligned16(arg) && aligned16(din),
               PGCN_E_INVALID, "agg_max_bwd: null or misaligned argument");
    PGCN_CHECK(g->g->rows() == g->g->cols() && g->g->nnz() <= INT_MAX, PGCN_E_INVALID,
               "agg_max_bwd: square pattern, nnz within an int");
    check_device();
    const GatPattern &p = g->g->gat_pattern();
    launch_agg_max_bwd(p, g->g->sage_ws(), G, ld_g, arg, ld_arg, d, din, ld_din,
                       as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

namespace {
void check_readout_dims(int d, int mode, int G, int n, std::initializer_list<int> lds) {
  PGCN_CHECK(d >= 1 && d <= kReadoutMaxWidth, PGCN_E_INVALID, "readout: 1 <= d <= 128");
  PGCN_CHECK(mode >= kReadoutSum && mode <= kReadoutMax, PGCN_E_INVALID,
             "readout: mode 1 (sum), 2 (mean) or 3 (max)");
  PGCN_CHECK(G >= 0 && n >= 0, PGCN_E_INVALID, "readout: G >= 0, n >= 0");
  for (int ld : lds) PGCN_CHECK(ln_ld_ok(ld, d), PGCN_E_INVALID, "readout: ld % 4 == 0, ld >= d");
}
}  // namespace

int pgcn_readout_chunk_rows(void) { return kReadoutChunk; }

size_t pgcn_readout_workspace(int n) { return readout_workspace(n); }

int pgcn_readout_fwd(const float *in, int ld_in, const int *graph_ptr, int G, int n, int d,
                     int mode, int max_len, float *out, int ld_out, int *arg, int ld_arg,
                     void *workspace, void *stream) {
  return guarded([&] {
    check_readout_dims(d, mode, G, n, {ld_in, ld_out});
    if (arg) check_readout_dims(d, mode, G, n, {ld_arg});
    PGCN_CHECK(max_len >= 0, PGCN_E_INVALID, "readout_fwd: max_len >= 0");
    PGCN_CHECK((in || n == 0) && graph_ptr && out && aligned16(in) && aligned16(out) &&
                   aligned16(arg),
               PGCN_E_INVALID, "readout_fwd: null or misaligned argument");
    PGCN_CHECK(max_len <= kReadoutChunk || n <= kReadoutChunk ||
                   (workspace && aligned16(workspace)),
               PGCN_E_INVALID, "readout_fwd: ranges above the chunk length need the workspace");
    check_device();
    launch_readout_fwd(in, ld_in, graph_ptr, G, n, d, mode, max_len, out, ld_out, arg, ld_arg,
                       workspace, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_readout_bwd(const float *G_out, int ld_g, const int *graph_ptr, const int *node_graph,
                     const int *arg, int ld_arg, int G, int n, int d, int mode, float *din,
                     int ld_din, void *stream) {
  return guarded([&] {
    check_readout_dims(d, mode, G, n, {ld_g, ld_din});
    if (mode == kReadoutMax) check_readout_dims(d, mode, G, n, {ld_arg});
    PGCN_CHECK(G_out && graph_ptr && node_graph && din && (mode != kReadoutMax || arg) &&
                   aligned16(G_out) && aligned16(din) && aligned16(arg),
               PGCN_E_INVALID, "readout_bwd: null or misaligned argument");
    check_device();
    launch_readout_bwd(G_out, ld_g, graph_ptr, node_graph, arg, ld_arg, G, n, d, mode, din, ld_din,
                       as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

namespace {
// widths and strides of the pair-score entries: `wide` strides span d columns, `one` strides one
void check_link_dims(int d, std::initializer_list<int> wide, std::initializer_list<int> one) {
  PGCN_CHECK(d >= 1 && d <= kLinkMaxWidth, PGCN_E_INVALID, "link_score: 1 <= d <= 128");
  for (int ld : wide) PGCN_CHECK(ln_ld_ok(ld, d), PGCN_E_INVALID, "link_score: ld % 4 == 0, ld >= d");
  for (int ld : one) PGCN_CHECK(ln_ld_ok(ld, 1), PGCN_E_INVALID, "link_score: ld % 4 == 0, ld >= 1");
}
}  // namespace

int pgcn_links_create(int n_nodes, long long n_pairs, const int *src, const int *dst,
                      const int *select, pgcn_links **out) {
  return guarded([&] {
    PGCN_CHECK(out, PGCN_E_INVALID, "links_create args");
    validate_pairs(n_nodes, n_pairs, src, dst);
    check_device();
    auto h = std::make_unique<pgcn_links>();
    h->l = std::make_unique<LinkIndexDev>(n_nodes, n_pairs, src, dst, select);
    *out = h.release();
  });
}

int pgcn_links_destroy(pgcn_links *l) {
  delete l;
  return PGCN_OK;
}

int pgcn_link_segment_slots(void) { return kGatSeg; }

long long pgcn_links_slots(const pgcn_links *l) {
  return l && l->l ? l->l->slots() : (long long)PGCN_E_INVALID;
}

int pgcn_link_score_fwd(const pgcn_links *l, const float *H, int ld_h, int d, float *scores,
                        int ld_s, void *stream) {
  return guarded([&] {
    check_link_dims(d, {ld_h}, {ld_s});
    PGCN_CHECK(l && l->l && H && scores && aligned16(H) && aligned16(scores), PGCN_E_INVALID,
               "link_score_fwd: null or misaligned argument");
    check_device();
    launch_link_score_fwd(l->l->index(), H, ld_h, d, scores, ld_s, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_link_score_bwd(const pgcn_links *l, const float *H, int ld_h, int d, const float *G,
                        int ld_g, float *dH, int ld_dh, void *stream) {
  return guarded([&] {
    check_link_dims(d, {ld_h, ld_dh}, {ld_g});
    PGCN_CHECK(l && l->l && H && G && dH && aligned16(H) && aligned16(G) && aligned16(dH),
               PGCN_E_INVALID, "link_score_bwd: null or misaligned argument");
    check_device();
    launch_link_score_bwd(l->l->index(), H, ld_h, d, G, ld_g, dH, ld_dh, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_debug_links_incidence(int n_nodes, long long n_pairs, const int *src, const int *dst,
                               const int *select, int *ptr, int *pair, int *other) {
  return guarded([&] {
    PGCN_CHECK(ptr, PGCN_E_INVALID, "debug_links_incidence: ptr [n_nodes + 1] is required");
    std::vector<int> p, e, o;
    validate_pairs(n_nodes, n_pairs, src, dst);
    build_incidence(n_nodes, n_pairs, src, dst, select, &p, &e, &o);
    std::memcpy(ptr, p.data(), p.size() * sizeof(int));
    if (pair && !e.empty()) std::memcpy(pair, e.data(), e.size() * sizeof(int));
    if (other && !o.empty()) std::memcpy(other, o.data(), o.size() * sizeof(int));
  });
}

int pgcn_rank_queries_create(int n_nodes, long long n_queries, const int *anchor, const int *target,
                             const long long *filter_ptr, const int *filter_idx,
                             pgcn_rank_queries **out) {
  return guarded([&] {
    PGCN_CHECK(out, PGCN_E_INVALID, "rank_queries_create args");
    validate_rank_queries(n_nodes, n_queries, anchor, target, filter_ptr, filter_idx);
    check_device();
    auto h = std::make_unique<pgcn_rank_queries>();
    h->q = std::make_unique<RankQueriesDev>(n_nodes, n_queries, anchor, target, filter_ptr,
                                            filter_idx);
    *out = h.release();
  });
}

int pgcn_rank_queries_destroy(pgcn_rank_queries *q) {
  delete q;
  return PGCN_OK;
}

void pgcn_link_rank_tile(int *queries_per_block, int *candidates_per_tile) {
  if (queries_per_block) *queries_per_block = kRankTQ;
  if (candidates_per_tile) *candidates_per_tile = kRankTC;
}

int pgcn_link_rank_scores(const int *src, const int *dst, long long m, const float *H, int ld_h,
                          int d, float *scores, void *stream) {
  return guarded([&] {
    check_link_dims(d, {ld_h}, {});
    PGCN_CHECK(m >= 0 && H && aligned16(H) && (m == 0 || (src && dst && scores)), PGCN_E_INVALID,
               "link_rank_scores: null or misaligned argument");
    check_device();
    launch_rank_scores(src, dst, m, H, ld_h, d, scores, nullptr, nullptr, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_link_rank(const pgcn_rank_queries *q, const float *H, int ld_h, int d,
                   unsigned int *greater, unsigned int *equal, void *stream) {
  return guarded([&] {
    check_link_dims(d, {ld_h}, {});
    PGCN_CHECK(q && q->q && H && aligned16(H), PGCN_E_INVALID,
               "link_rank: null or misaligned argument");
    PGCN_CHECK(q->q->queries().n_queries == 0 || (greater && equal), PGCN_E_INVALID,
               "link_rank: greater and equal [n_queries]");
    check_device();
    launch_link_rank(q->q->queries(), H, ld_h, d, greater, equal, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

long long pgcn_debug_rank_filter(int n_nodes, const int *indptr, const int *indices,
                                 long long n_pairs, const int *pair_src, const int *pair_dst,
                                 const int *pair_label, const int *pair_split, int split, int side,
                                 int filtered, long long *n_filter, int *anchor, int *target,
                                 long long *ptr, int *idx) {
  long long n = -1;
  const int st = guarded([&] {
    const RankFilterHost f = build_rank_filter(n_nodes, indptr, indices, n_pairs, pair_src,
                                               pair_dst, pair_label, pair_split, split, side,
                                               filtered);
    n = (long long)f.anchor.size();
    if (n_filter) *n_filter = (long long)f.idx.size();
    if (anchor && n) std::memcpy(anchor, f.anchor.data(), f.anchor.size() * sizeof(int));
    if (target && n) std::memcpy(target, f.target.data(), f.target.size() * sizeof(int));
    if (ptr) std::memcpy(ptr, f.ptr.data(), f.ptr.size() * sizeof(long long));
    if (idx && !f.idx.empty()) std::memcpy(idx, f.idx.data(), f.idx.size() * sizeof(int));
  });
  return st == PGCN_OK ? n : st;
}

int pgcn_topk_queries_create(int n_nodes, long long n_queries, const int *anchor,
                             const long long *exclude_ptr, const int *exclude_idx, int k,
                             pgcn_topk_queries **out) {
  return guarded([&] {
    PGCN_CHECK(out, PGCN_E_INVALID, "topk_queries_create args");
    validate_topk_queries(n_nodes, n_queries, anchor, exclude_ptr, exclude_idx, k);
    check_device();
    auto h = std::make_unique<pgcn_topk_queries>();
    h->q = std::make_unique<TopKQueriesDev>(n_nodes, n_queries, anchor, exclude_ptr, exclude_idx, k);
    *out = h.release();
  });
}

int pgcn_topk_queries_destroy(pgcn_topk_queries *q) {
  delete q;
  return PGCN_OK;
}

long long pgcn_topk_queries_workspace(const pgcn_topk_queries *q) {
  return q && q->q ? q->q->workspace() : (long long)PGCN_E_INVALID;
}

void pgcn_link_topk_tile(int *queries_per_block, int *candidates_per_tile, int *k_max) {
  if (queries_per_block) *queries_per_block = kRankTQ;
  if (candidates_per_tile) *candidates_per_tile = kRankTC;
  if (k_max) *k_max = kTopKMax;
}

int pgcn_link_topk_splits(long long n_queries, int n_nodes) {
  return topk_splits(n_queries, n_nodes);
}

int pgcn_link_topk_chunk(void) { return kTopKChunk; }

int pgcn_link_topk(const pgcn_topk_queries *q, const float *H, int ld_h, int d, int *idx,
                   float *score, void *stream) {
  return guarded([&] {
    check_link_dims(d, {ld_h}, {});
    PGCN_CHECK(q && q->q && H && aligned16(H), PGCN_E_INVALID,
               "link_topk: null or misaligned argument");
    PGCN_CHECK(q->q->queries().n_queries == 0 || (idx && score), PGCN_E_INVALID,
               "link_topk: idx and score [n_queries][k]");
    check_device();
    launch_link_topk(q->q->queries(), H, ld_h, d, idx, score, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

long long pgcn_debug_topk_filter(int n_nodes, const int *indptr, const int *indices,
                                 long long n_pairs, const int *pair_src, const int *pair_dst,
                                 const int *pair_label, const int *pair_split, long long m,
                                 const int *nodes, int side, int filtered, long long *n_exclude,
                                 long long *ptr, int *idx) {
  const int st = guarded([&] {
    const TopKFilterHost f = build_topk_filter(n_nodes, indptr, indices, n_pairs, pair_src,
                                               pair_dst, pair_label, pair_split, m, nodes, side,
                                               filtered);
    if (n_exclude) *n_exclude = (long long)f.idx.size();
    if (ptr) std::memcpy(ptr, f.ptr.data(), f.ptr.size() * sizeof(long long));
    if (idx && !f.idx.empty()) std::memcpy(idx, f.idx.data(), f.idx.size() * sizeof(int));
  });
  return st == PGCN_OK ? m : st;
}

int pgcn_xent_blocks(int n) { return xent_blocks(n); }

int pgcn_xent_fwd(float *logits, int ld, float *grad, const int *truth, int n, int c, int count,
                  int training, float *partials, void *stream) {
  return guarded([&] {
    launch_xent_fwd(logits, ld, grad, truth, n, c, count, training, partials, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_finalize(const float *partials, int n_blocks, int count, const float *w_l2,
                  long long n_l2, float weight_decay, float *out4, void *stream) {
  return guarded([&] {
    // out4[0..1] = {loss, acc}; out4[2..3] hold the raw sums (loss_sum, wrong); one launch
    launch_reduce_scalars(partials, n_blocks, w_l2, n_l2, out4 + 2, as_stream(stream), count,
                          weight_decay, out4);
  });
}

int pgcn_predict_rows(const float *logits, int ld, int n, int c, int *cls, float *conf,
                      float *probs, int ld_probs, void *stream) {
  return guarded([&] {
    check_device();
    launch_predict_rows(logits, ld, n, c, cls, conf, probs, ld_probs, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_confusion(const int *cls, const int *truth, int n, int c, unsigned int *counts,
                   void *stream) {
  return guarded([&] {
    check_device();
    launch_confusion(cls, truth, n, c, counts, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_bce_fwd(const float *logits, int ld, float *grad, const int *truth,
                 const uint32_t *label_bits, int words, int n, int c, int count, int training,
                 float *partials, void *stream) {
  return guarded([&] {
    check_bce_args(ld, words, n, c, count);
    if (n == 0) return;
    check_device();
    launch_bce_fwd(logits, ld, grad, truth, label_bits, words, n, c, count, training, partials,
                   as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_predict_multilabel_rows(const float *logits, int ld, int n, int c, uint32_t *bits,
                                 int words, float *probs, int ld_probs, void *stream) {
  return guarded([&] {
    check_predict_multilabel_args(ld, n, c, words, probs != nullptr, ld_probs);
    if (n == 0) return;
    check_device();
    launch_predict_multilabel(logits, ld, n, c, bits, words, probs, ld_probs, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_multilabel_counts(const uint32_t *pred_bits, const uint32_t *label_bits,
                           const int *truth, int n, int c, int words, unsigned int *counts,
                           void *stream) {
  return guarded([&] {
    check_multilabel_counts_args(n, c, words);
    check_device();
    launch_multilabel_counts(pred_bits, label_bits, truth, n, c, words, counts,
                             as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_adam(float *w, const float *g, float *m, float *v, long long n, float step_size,
              float beta1, float beta2, float eps, float weight_decay, int decay, void *stream) {
  return guarded([&] {
    launch_adam(w, g, m, v, n, step_size, beta1, beta2, eps, weight_decay, decay,
                as_stream(stream));
  });
}

float pgcn_adam_step_size(float lr, float beta1, float beta2, int t) {
  return lr * sqrtf(1.0f - powf(beta2, (float)t)) / (1.0f - powf(beta1, (float)t));
}

// ---------------------------------------------------------------- engine
void pgcn_params_default(pgcn_params *p) {
  std::memset(p, 0, sizeof *p);
  p->n_layers = 2;
  p->hidden_dims[0] = 16;
  p->dropouts[0] = 0.5f;
  p->dropouts[1] = 0.5f;
  p->aggregator = 0;
  p->root_weight = 0;
  p->epochs = 100;
  p->readout = 0;
  p->link_decoder = 0;
  p->early_stopping = 0;
  p->attention_heads = 1;
  p->attention_dropout = 0.0f;
  p->learning_rate = 0.01f;
  p->weight_decay = 5e-4f;
  p->beta1 = 0.9f;
  p->beta2 = 0.999f;
  p->eps = 1e-8f;
  p->attention = 0;
  p->reassociate_last = 1;
  p->multilabel = 0;
  p->seed = 0;
  p->layer_norm = 0;
  p->residual = 0;
}

int pgcn_gcn_create(const pgcn_params *p, const pgcn_data *d, int device, pgcn_gcn **out) {
  return guarded([&] {
    PGCN_CHECK(p && d && out, PGCN_E_INVALID, "gcn_create args");
    check_device();
    GCNData data = to_data(d, p);
    auto h = std::make_unique<pgcn_gcn>();
    h->g = std::make_unique<GCN>(to_params(p, d), to_adam(p), data, device, nullptr);
    *out = h.release();
  });
}

int pgcn_comm_unique_id(void *uid) {
  return guarded([&] { Comm::unique_id(uid); });
}

int pgcn_gcn_create_dist(const pgcn_params *p, const pgcn_data *d, int device, int rank,
                         int world, const void *uid, pgcn_gcn **out) {
  return guarded([&] {
    PGCN_CHECK(p && d && out && uid, PGCN_E_INVALID, "gcn_create_dist args");
    refuse_single_gpu_only(p);
    check_device();
    GCNData data = to_data(d, p);
    DistSpec ds;
    ds.rank = rank;
    ds.world = world;
    ds.unique_id = uid;
    auto h = std::make_unique<pgcn_gcn>();
    h->g = std::make_unique<GCN>(to_params(p, d), to_adam(p), data, device, &ds);
    *out = h.release();
  });
}

int pgcn_gcn_create_peer(const pgcn_params *p, const pgcn_data *d, int device, int rank,
                         int world, pgcn_allgather_fn allgather, void *user, pgcn_gcn **out) {
  return guarded([&] {
    PGCN_CHECK(p && d && out && allgather && world >= 1 && world <= kPeerMaxRanks && rank >= 0 &&
                   rank < world,
               PGCN_E_INVALID, "gcn_create_peer args");
    refuse_single_gpu_only(p);
    check_device();
    GCNData data = to_data(d, p);
    DistSpec ds;
    ds.rank = rank;
    ds.world = world;
    ds.allgather = [allgather, user](const void *mine, size_t bytes, void *all) {
      if (allgather(mine, bytes, all, user) != 0)
        throw Error(PGCN_E_COMM, "peer comm: the caller's all-gather failed");
    };
    auto h = std::make_unique<pgcn_gcn>();
    h->g = std::make_unique<GCN>(to_params(p, d), to_adam(p), data, device, &ds);
    *out = h.release();
  });
}

int pgcn_debug_gcn_create_solo(const pgcn_params *p, const pgcn_data *d, int device, int rank,
                               int world, pgcn_gcn **out) {
  return guarded([&] {
    PGCN_CHECK(p && d && out && world >= 1 && rank >= 0 && rank < world, PGCN_E_INVALID,
               "gcn_create_solo args");
    refuse_single_gpu_only(p);
    check_device();
    GCNData data = to_data(d, p);
    DistSpec ds;
    ds.rank = rank;
    ds.world = world;
    ds.solo = true;
    auto h = std::make_unique<pgcn_gcn>();
    h->g = std::make_unique<GCN>(to_params(p, d), to_adam(p), data, device, &ds);
    *out = h.release();
  });
}

int pgcn_loopback_create(int world, pgcn_loopback **out) {
  return guarded([&] {
    PGCN_CHECK(out, PGCN_E_INVALID, "loopback_create args");
    auto h = std::make_unique<pgcn_loopback>();
    h->g = std::make_shared<LoopbackGroup>(world);
    *out = h.release();
  });
}

int pgcn_loopback_destroy(pgcn_loopback *g) {
  delete g;  // engines keep the group alive until they are destroyed
  return PGCN_OK;
}

int pgcn_gcn_create_loopback(const pgcn_params *p, const pgcn_data *d, int device, int rank,
                             pgcn_loopback *group, pgcn_gcn **out) {
  return guarded([&] {
    PGCN_CHECK(p && d && out && group && group->g, PGCN_E_INVALID, "gcn_create_loopback args");
    refuse_single_gpu_only(p);
    check_device();
    GCNData data = to_data(d, p);
    DistSpec ds;
    ds.rank = rank;
    ds.world = group->g->world();
    ds.loopback = group->g;
    auto h = std::make_unique<pgcn_gcn>();
    h->g = std::make_unique<GCN>(to_params(p, d), to_adam(p), data, device, &ds);
    *out = h.release();
  });
}

long long pgcn_gcn_query(pgcn_gcn *g, const char *key) {
  if (!g || !key) return PGCN_E_INVALID;
  const GCN &e = *g->g;
  const Comm *c = e.communicator();
  if (!std::strncmp(key, "knob.", 5)) {  // the engine's snapshot, whatever was set since
    const KnobRow *row = find_knob(key + 5);
    return row ? e.knobs().*row->field : PGCN_E_INVALID;
  }
  if (!std::strcmp(key, "world")) return c ? c->world() : 1;
  if (!std::strcmp(key, "rank")) return c ? c->rank() : 0;
  if (!std::strcmp(key, "comm"))
    return c ? (!std::strcmp(c->kind(), "rccl")       ? 1
                : !std::strcmp(c->kind(), "loopback") ? 2
                : !std::strcmp(c->kind(), "solo")     ? 3
                                                      : 4)
             : 0;
  if (!std::strcmp(key, "comm_calls")) return c ? c->calls : 0;
  if (!std::strcmp(key, "peer_uncached")) {  // the peer exchange's slots are uncached memory
    const auto *pc = dynamic_cast<const pgcn::PeerComm *>(c);
    return pc && pc->slots_uncached() ? 1 : 0;
  }
  if (!std::strcmp(key, "comm_bytes")) return c ? (long long)c->bytes : 0;
  if (!std::strcmp(key, "reassociated")) return e.reassociated() ? 1 : 0;
  if (!std::strcmp(key, "fused_tails")) return e.fused_tails();
  if (!std::strcmp(key, "residual_layers")) return e.residual_layers();
  if (!std::strcmp(key, "fused_residuals")) return e.fused_residuals();
  if (!std::strcmp(key, "norm_padding_nonzero")) {
    long long n = PGCN_E_INVALID;
    const int st = guarded([&] { n = g->g->norm_padding_nonzero(); });
    return st == PGCN_OK ? n : st;
  }
  if (!std::strcmp(key, "norm_layers")) return e.norm_layers();
  if (!std::strcmp(key, "attention_layers")) return e.attention_layers();
  if (!std::strcmp(key, "attention_heads")) return e.attention_heads();
  if (!std::strcmp(key, "attention_dropout_layers")) return e.attention_dropout_layers();
  if (!std::strcmp(key, "aggregator")) return e.aggregator();
  if (!std::strcmp(key, "root_weight")) return e.root_weight() ? 1 : 0;
  if (!std::strcmp(key, "multilabel")) return e.get_params().multilabel ? 1 : 0;
  if (!std::strcmp(key, "readout")) return e.get_params().readout;
  if (!std::strcmp(key, "num_graphs")) return e.num_graphs();
  if (!std::strcmp(key, "link_decoder")) return e.get_params().link_decoder;
  if (!std::strcmp(key, "num_pairs")) return e.num_pairs();
  if (!std::strcmp(key, "fused_norm_tails")) return e.fused_norm_tails();
  if (!std::strcmp(key, "graph_symmetric")) return e.symmetric() ? 1 : 0;
  if (!std::strcmp(key, "graphsum_lds")) return e.graphsum_lds() ? 1 : 0;
  if (!std::strcmp(key, "epochs")) return e.epochs_run();
  if (!std::strcmp(key, "adam_steps")) return e.adam_steps();
  if (!std::strcmp(key, "eval_ax_us")) return (long long)(e.eval_ax_build_ms() * 1000.0f);
  return PGCN_E_INVALID;
}

int pgcn_gcn_destroy(pgcn_gcn *g) {
  delete g;
  return PGCN_OK;
}

int pgcn_gcn_train_epoch(pgcn_gcn *g, float out2[2]) {
  return guarded([&] {
    auto r = g->g->train_epoch();
    out2[0] = r.first;
    out2[1] = r.second;
  });
}

int pgcn_gcn_eval(pgcn_gcn *g, int split, float out2[2]) {
  return guarded([&] {
    auto r = g->g->eval(split);
    out2[0] = r.first;
    out2[1] = r.second;
  });
}

int pgcn_gcn_epoch_async(pgcn_gcn *g) {
  return guarded([&] { g->g->epoch_async(); });
}
int pgcn_gcn_sync(pgcn_gcn *g) {
  return guarded([&] { g->g->sync(); });
}
int pgcn_gcn_results(pgcn_gcn *g, int n, float *host_out) {
  int rows = 0;
  const int st = guarded([&] {
    PGCN_CHECK(n >= 0 && (n == 0 || host_out), PGCN_E_INVALID, "gcn_results args");
    auto r = g->g->results(n);
    std::memcpy(host_out, r.data(), r.size() * sizeof(float));
    rows = (int)(r.size() / 4);
  });
  return st == PGCN_OK ? rows : st;
}
int pgcn_gcn_run(pgcn_gcn *g, int verbose) {
  return guarded([&] { g->g->run(verbose != 0); });
}
long long pgcn_gcn_get_var(pgcn_gcn *g, int idx, int which, float *dst) {
  long long n = -1;
  const int st = guarded([&] {
    auto v = g->g->get_var(idx, which);
    if (dst && !v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(float));
    n = (long long)v.size();
  });
  return st == PGCN_OK ? n : st;
}
int pgcn_gcn_num_vars(pgcn_gcn *g) { return g->g->num_vars(); }
int pgcn_gcn_set_var(pgcn_gcn *g, int idx, int which, const float *src, long long count) {
  return guarded([&] {
    PGCN_CHECK(g, PGCN_E_INVALID, "gcn_set_var: null engine");
    g->g->set_var(idx, which, src, count);
  });
}
int pgcn_gcn_save(pgcn_gcn *g, const char *path) {
  return guarded([&] {
    PGCN_CHECK(g && path, PGCN_E_INVALID, "gcn_save args");
    g->g->save(path);
  });
}
int pgcn_gcn_load(pgcn_gcn *g, const char *path, int flags) {
  return guarded([&] {
    PGCN_CHECK(g && path, PGCN_E_INVALID, "gcn_load args");
    g->g->load(path, flags);
  });
}
int pgcn_checkpoint_info(const char *path, long long info[8]) {
  return guarded([&] {
    PGCN_CHECK(path && info, PGCN_E_INVALID, "checkpoint_info args");
    const Checkpoint ck = read_checkpoint(path);
    info[0] = ck.version;
    info[1] = ck.n_layers;
    info[2] = ck.num_nodes;
    info[3] = ck.dims.front();
    info[4] = ck.dims.back();
    info[5] = ck.adam_steps;
    info[6] = ck.epochs;
    info[7] = (long long)ck.w.size();
  });
}
int pgcn_checkpoint_flags(const char *path) {
  int flags = 0;
  const int st = guarded([&] {
    PGCN_CHECK(path, PGCN_E_INVALID, "checkpoint_flags args");
    flags = (int)read_checkpoint(path).flags;
  });
  return st == PGCN_OK ? flags : st;
}
int pgcn_checkpoint_attention(const char *path, int *heads, float *dropout) {
  return guarded([&] {
    PGCN_CHECK(path && heads && dropout, PGCN_E_INVALID, "checkpoint_attention args");
    const Checkpoint ck = read_checkpoint(path);
    *heads = ck.heads;
    *dropout = ck.attention_dropout;
  });
}
int pgcn_checkpoint_sage(const char *path, int *aggregator, int *root_weight) {
  return guarded([&] {
    PGCN_CHECK(path && aggregator && root_weight, PGCN_E_INVALID, "checkpoint_sage args");
    const Checkpoint ck = read_checkpoint(path);
    *aggregator = ck.aggregator;
    *root_weight = ck.root_weight;
  });
}
int pgcn_checkpoint_readout(const char *path, int *mode, int *num_graphs) {
  return guarded([&] {
    PGCN_CHECK(path && mode && num_graphs, PGCN_E_INVALID, "checkpoint_readout args");
    const Checkpoint ck = read_checkpoint(path);
    *mode = ck.readout;
    *num_graphs = ck.num_graphs;
  });
}
int pgcn_checkpoint_links(const char *path, int *decoder, long long *num_pairs) {
  return guarded([&] {
    PGCN_CHECK(path && decoder && num_pairs, PGCN_E_INVALID, "checkpoint_links args");
    const Checkpoint ck = read_checkpoint(path);
    *decoder = ck.link_decoder;
    *num_pairs = ck.num_pairs;
  });
}
int pgcn_params_sizeof(void) { return (int)sizeof(pgcn_params); }
long long pgcn_gcn_predict(pgcn_gcn *g, int *cls, float *conf, float *probs) {
  long long n = -1;
  const int st = guarded([&] {
    PGCN_CHECK(g, PGCN_E_INVALID, "gcn_predict: null engine");
    n = g->g->predict(cls, conf, probs);
  });
  return st == PGCN_OK ? n : st;
}
int pgcn_gcn_confusion(pgcn_gcn *g, int split, long long *counts) {
  return guarded([&] {
    PGCN_CHECK(g, PGCN_E_INVALID, "gcn_confusion: null engine");
    g->g->confusion(split, counts);
  });
}
long long pgcn_gcn_predict_multilabel(pgcn_gcn *g, uint32_t *bits, float *probs) {
  long long n = -1;
  const int st = guarded([&] {
    PGCN_CHECK(g, PGCN_E_INVALID, "gcn_predict_multilabel: null engine");
    n = g->g->predict_multilabel(bits, probs);
  });
  return st == PGCN_OK ? n : st;
}
int pgcn_gcn_multilabel_counts(pgcn_gcn *g, int split, long long *counts) {
  return guarded([&] {
    PGCN_CHECK(g && counts, PGCN_E_INVALID, "gcn_multilabel_counts args");
    g->g->multilabel_counts(split, counts);
  });
}
long long pgcn_gcn_predict_links(pgcn_gcn *g, float *scores, float *probs) {
  long long n = -1;
  const int st = guarded([&] {
    PGCN_CHECK(g, PGCN_E_INVALID, "gcn_predict_links: null engine");
    n = g->g->predict_links(scores, probs);
  });
  return st == PGCN_OK ? n : st;
}
int pgcn_gcn_link_counts(pgcn_gcn *g, int split, long long *counts) {
  return guarded([&] {
    PGCN_CHECK(g && counts, PGCN_E_INVALID, "gcn_link_counts args");
    g->g->link_counts(split, counts);
  });
}
long long pgcn_gcn_link_ranks(pgcn_gcn *g, int split, int side, int filtered, long long *greater,
                              long long *equal) {
  long long n = -1;
  const int st = guarded([&] {
    PGCN_CHECK(g, PGCN_E_INVALID, "gcn_link_ranks: null engine");
    n = g->g->link_ranks(split, side, filtered, greater, equal);
  });
  return st == PGCN_OK ? n : st;
}
long long pgcn_gcn_top_links(pgcn_gcn *g, const int *nodes, long long m, int k, int side,
                             int filtered, int *idx, float *score) {
  const int st = guarded([&] {
    PGCN_CHECK(g, PGCN_E_INVALID, "gcn_top_links: null engine");
    g->g->top_links(nodes, m, k, side, filtered, idx, score);
  });
  return st == PGCN_OK ? m : st;
}
int pgcn_gcn_score_pairs(pgcn_gcn *g, const int *src, const int *dst, long long m,
                         float *scores) {
  return guarded([&] {
    PGCN_CHECK(g, PGCN_E_INVALID, "gcn_score_pairs: null engine");
    g->g->score_pairs(src, dst, m, scores);
  });
}
int pgcn_gcn_profile(pgcn_gcn *g, int enable) {
  return guarded([&] { g->g->set_profile(enable != 0); });
}
int pgcn_gcn_profile_read(pgcn_gcn *g, double *ms, long long *calls, double *bytes) {
  return guarded([&] { g->g->profile_read(ms, calls, bytes); });
}
int pgcn_gcn_profile_read_mm(pgcn_gcn *g, double *ms, long long *calls, double *flops) {
  return guarded([&] { g->g->profile_read_mm(ms, calls, flops); });
}
int pgcn_gcn_node_range(pgcn_gcn *g, int *first, int *last) {
  *first = g->g->partition().first();
  *last = g->g->partition().last();
  return PGCN_OK;
}

// ---------------------------------------------------------------- data
int pgcn_dataset_load(const char *root, const char *name, pgcn_dataset **out) {
  return guarded([&] {
    auto h = std::make_unique<pgcn_dataset>();
    Parser parser(&h->d, name, root ? root : ".");
    if (!parser.parse()) throw Error(PGCN_E_IO, std::string("Cannot read input: ") + name);
    *out = h.release();
  });
}

int pgcn_dataset_load_cached(const char *root, const char *name, pgcn_dataset **out,
                             int *from_cache) {
  return guarded([&] {
    auto h = std::make_unique<pgcn_dataset>();
    bool hit = false;
    if (!load_dataset_cached(&h->d, root ? root : ".", name, &hit))
      throw Error(PGCN_E_IO, std::string("Cannot read input: ") + name);
    if (from_cache) *from_cache = hit ? 1 : 0;
    *out = h.release();
  });
}

int pgcn_dataset_save(const pgcn_dataset *ds, const char *path) {
  return guarded([&] {
    PGCN_CHECK(ds && path, PGCN_E_INVALID, "dataset_save: null argument");
    PGCN_CHECK(ds->d.label_bits.empty(), PGCN_E_INVALID,
               "dataset_save: the cache format holds no multi-label data");
    if (!save_binary(ds->d, path, nullptr))
      throw Error(PGCN_E_IO, std::string("cannot write ") + path);
  });
}

int pgcn_dataset_binarize(pgcn_dataset *ds) {
  if (!ds) return PGCN_E_INVALID;
  std::fill(ds->d.feature_value.begin(), ds->d.feature_value.end(), 1.0f);
  return PGCN_OK;
}

int pgcn_dataset_load_binary(const char *path, pgcn_dataset **out) {
  return guarded([&] {
    PGCN_CHECK(path && out, PGCN_E_INVALID, "dataset_load_binary: null argument");
    auto h = std::make_unique<pgcn_dataset>();
    if (!load_binary(&h->d, path, nullptr))
      throw Error(PGCN_E_IO, std::string("not a valid dataset cache: ") + path);
    *out = h.release();
  });
}

int pgcn_dataset_synthetic(int n, int f, int c, long long undirected_edges, uint64_t seed,
                           pgcn_dataset **out) {
  return guarded([&] {
    PGCN_CHECK(n > 1 && f > 0 && c > 0 && undirected_edges >= 0, PGCN_E_INVALID, "synthetic args");
    auto h = std::make_unique<pgcn_dataset>();
    make_synthetic(&h->d, n, f, c, undirected_edges, seed);
    *out = h.release();
  });
}

int pgcn_dataset_view(const pgcn_dataset *ds, pgcn_data *v, int *input_dim, int *output_dim) {
  if (!ds || !v) return PGCN_E_INVALID;
  v->num_nodes = ds->d.num_nodes;
  v->graph_indptr = ds->d.graph.indptr.data();
  v->graph_indices = ds->d.graph.indices.data();
  v->feat_indptr = ds->d.feature_index.indptr.data();
  v->feat_indices = ds->d.feature_index.indices.data();
  v->feat_values = ds->d.feature_value.data();
  v->label = ds->d.label.data();
  v->split = ds->d.split.data();
  v->label_bits = ds->d.label_bits.empty() ? nullptr : ds->d.label_bits.data();
  v->label_words = ds->d.label_bits.empty() ? 0 : ds->d.label_words;
  const bool graphs = ds->d.num_graphs > 0;
  v->num_graphs = graphs ? ds->d.num_graphs : 0;
  v->graph_ptr = graphs ? ds->d.graph_ptr.data() : nullptr;
  v->graph_label = graphs ? ds->d.graph_label.data() : nullptr;
  v->graph_split = graphs ? ds->d.graph_split.data() : nullptr;
  const bool pairs = !ds->d.pair_src.empty();
  v->num_pairs = (int)ds->d.pair_src.size();
  v->pair_src = pairs ? ds->d.pair_src.data() : nullptr;
  v->pair_dst = pairs ? ds->d.pair_dst.data() : nullptr;
  v->pair_label = pairs ? ds->d.pair_label.data() : nullptr;
  v->pair_split = pairs ? ds->d.pair_split.data() : nullptr;
  if (input_dim) *input_dim = ds->d.input_dim;
  if (output_dim) *output_dim = ds->d.output_dim;
  return PGCN_OK;
}

int pgcn_dataset_set_multilabel(pgcn_dataset *ds, const uint32_t *bits, int words, int c) {
  return guarded([&] {
    PGCN_CHECK(ds && bits && c >= 1 && c <= 128 && words == (c + 31) / 32, PGCN_E_INVALID,
               "dataset_set_multilabel: 1 <= c <= 128, words = ceil(c / 32)");
    const size_t n = (size_t)ds->d.num_nodes;
    if (c % 32) {
      const uint32_t past = ~((1u << (c % 32)) - 1u);
      for (size_t i = 0; i < n; i++)
        PGCN_CHECK(!(bits[i * words + words - 1] & past), PGCN_E_INVALID,
                   "dataset_set_multilabel: bits at positions >= c must be zero");
    }
    ds->d.label_bits.assign(bits, bits + n * words);
    ds->d.label_words = words;
    ds->d.output_dim = c;
  });
}

int pgcn_dataset_load_labels(pgcn_dataset *ds, const char *path, int num_classes) {
  return guarded([&] {
    PGCN_CHECK(ds && path && num_classes >= 0 && num_classes <= 128, PGCN_E_INVALID,
               "dataset_load_labels: 0 <= num_classes <= 128");
    std::vector<uint32_t> bits;
    int words = 0, c = 0;
    std::string why;
    if (!read_labels_file(path, ds->d.num_nodes, num_classes, &bits, &words, &c, &why))
      throw Error(PGCN_E_IO, why);
    ds->d.label_bits = std::move(bits);
    ds->d.label_words = words;
    ds->d.output_dim = c;
    for (int &l : ds->d.label) l = std::max(l, 0);  // every line is a labelled node
  });
}

int pgcn_dataset_set_graphs(pgcn_dataset *ds, const int *graph_ptr, const int *label,
                            const int *split, int G, int num_classes) {
  return guarded([&] {
    PGCN_CHECK(ds && graph_ptr && label && split && G >= 1 && num_classes >= 0 &&
                   num_classes <= 128,
               PGCN_E_INVALID, "dataset_set_graphs: G >= 1, 0 <= num_classes <= 128");
    int c = num_classes;
    if (c == 0)
      for (int g = 0; g < G; g++) c = std::max(c, label[g] + 1);
    PGCN_CHECK(c >= 1 && c <= 128, PGCN_E_INVALID, "dataset_set_graphs: 1 <= classes <= 128");
    PGCN_CHECK(graphs_valid(ds->d.num_nodes, G, graph_ptr, label, split, c), PGCN_E_INVALID,
               "dataset_set_graphs: graph_ptr from 0 to num_nodes, non-decreasing; labels in "
               "[-1, classes); splits 0..3");
    ds->d.num_graphs = G;
    ds->d.graph_ptr.assign(graph_ptr, graph_ptr + G + 1);
    ds->d.graph_label.assign(label, label + G);
    ds->d.graph_split.assign(split, split + G);
    ds->d.output_dim = c;
  });
}

int pgcn_dataset_load_graphs(pgcn_dataset *ds, const char *path, int num_classes) {
  return guarded([&] {
    PGCN_CHECK(ds && path && num_classes >= 0 && num_classes <= 128, PGCN_E_INVALID,
               "dataset_load_graphs: 0 <= num_classes <= 128");
    std::vector<int> ptr, label, split;
    int c = 0;
    std::string why;
    if (!read_graphs_file(path, ds->d.num_nodes, num_classes, &ptr, &label, &split, &c, &why))
      throw Error(PGCN_E_IO, why);
    ds->d.num_graphs = (int)label.size();
    ds->d.graph_ptr = std::move(ptr);
    ds->d.graph_label = std::move(label);
    ds->d.graph_split = std::move(split);
    ds->d.output_dim = c;
  });
}

int pgcn_dataset_set_links(pgcn_dataset *ds, const int *src, const int *dst, const int *label,
                           const int *split, long long E, int embed_dim) {
  return guarded([&] {
    PGCN_CHECK(ds && embed_dim >= 1 && embed_dim <= kLinkMaxWidth, PGCN_E_INVALID,
               "dataset_set_links: 1 <= embed_dim <= 128");
    PGCN_CHECK(links_valid(ds->d.num_nodes, E, src, dst, label, split), PGCN_E_INVALID,
               "dataset_set_links: E >= 1 pairs, endpoints in [0, num_nodes), labels -1 / 0 / 1, "
               "splits 0..3");
    ds->d.pair_src.assign(src, src + E);
    ds->d.pair_dst.assign(dst, dst + E);
    ds->d.pair_label.assign(label, label + E);
    ds->d.pair_split.assign(split, split + E);
    ds->d.output_dim = embed_dim;
  });
}

int pgcn_dataset_load_links(pgcn_dataset *ds, const char *path, int embed_dim) {
  return guarded([&] {
    PGCN_CHECK(ds && path && embed_dim >= 1 && embed_dim <= kLinkMaxWidth, PGCN_E_INVALID,
               "dataset_load_links: 1 <= embed_dim <= 128");
    std::vector<int> src, dst, label, split;
    std::string why;
    if (!read_links_file(path, ds->d.num_nodes, &src, &dst, &label, &split, &why))
      throw Error(PGCN_E_IO, why);
    ds->d.pair_src = std::move(src);
    ds->d.pair_dst = std::move(dst);
    ds->d.pair_label = std::move(label);
    ds->d.pair_split = std::move(split);
    ds->d.output_dim = embed_dim;
  });
}

int pgcn_dataset_free(pgcn_dataset *ds) {
  delete ds;
  return PGCN_OK;
}

// ---------------------------------------------------------------- diagnostics
int pgcn_debug_set(const char *key, int value) {
  // every key's value range is checked: an out-of-range value is refused, never reinterpreted
  const KnobRow *row = key ? find_knob(key) : nullptr;
  if (!row || !row->accepts(value)) return PGCN_E_INVALID;
  process_knobs().*row->field = value;
  return PGCN_OK;
}

int pgcn_debug_knob(int index, const char **name, int *default_value) {
  if (index < 0 || index >= kKnobCount) return PGCN_E_INVALID;
  if (name) *name = kKnobTable[index].name;
  if (default_value) *default_value = Knobs{}.*kKnobTable[index].field;
  return PGCN_OK;
}

// the ring schedule a graph of this pattern created now would build (process_knobs())
static LdsHost debug_ring_host(int n_rows, int n_cols, const std::vector<int> &ip,
                               const std::vector<int> &ix) {
  const Knobs &k = process_knobs();
  const std::vector<int> cut = ring_cuts(n_cols, ix, lds_blocks(n_rows, n_cols, k));
  return build_ring_host(
      n_rows, n_cols, ip, ix, cut, lds_slots(n_rows, n_cols), k.ring_pair != 0,
      ring_window_for(n_rows, n_cols, (long long)ix.size(), (int)cut.size() - 1, k));
}

// CPU check of the d = 16 ring schedule of a CSR pattern: builds it, walks it as the kernel
// does over a seeded input and reports the max relative error of the sums against a direct CSR
// sum, and the number of entry blocks.  No device needed.  (window: kRingWindow, the only
// schedule.)  Diagnostics: the schedule's step counts [wg][t_max][LDS_CW][LDS_SLOTS] (uint16)
// and its shape {n_batches, t_max, LDS_CW, LDS_SLOTS, window} (balance analysis on the host).
long long pgcn_debug_lds_counts(int n_rows, int n_cols, const int *indptr, const int *indices,
                                int window, unsigned short *dst, long long cap, int *shape5) {
  long long n = -1;
  const int st = guarded([&] {
    PGCN_CHECK(n_rows > 0 && n_cols > 0 && indptr && indices && window == kRingWindow,
               PGCN_E_INVALID, "lds_counts args");
    std::vector<int> ip(indptr, indptr + n_rows + 1), ix(indices, indices + indptr[n_rows]);
    const LdsHost h = debug_ring_host(n_rows, n_cols, ip, ix);
    n = (long long)h.counts.size();
    if (dst) std::copy(h.counts.begin(), h.counts.begin() + std::min(n, cap), dst);
    if (shape5) {
      shape5[0] = h.n_batches;
      shape5[1] = h.t_max;
      shape5[2] = LDS_CW;
      shape5[3] = h.ns;
      shape5[4] = kRingWindow;
    }
  });
  return st == PGCN_OK ? n : -1;
}

int pgcn_debug_lds_check(int n_rows, int n_cols, const int *indptr, const int *indices,
                         int window, double *max_rel_err, long long *n_blocks) {
  return guarded([&] {
    PGCN_CHECK(n_rows > 0 && n_cols > 0 && indptr && indices && window == kRingWindow,
               PGCN_E_INVALID, "lds_check args");
    std::vector<int> ip(indptr, indptr + n_rows + 1), ix(indices, indices + indptr[n_rows]);
    const LdsHost h = debug_ring_host(n_rows, n_cols, ip, ix);
    std::vector<float> in((size_t)n_cols);
    uint64_t st[2] = {12345, 67890};
    for (auto &x : in) x = (float)((double)(xs_next(st) & 0xffffff) / (double)0x1000000 - 0.5);
    std::vector<double> out((size_t)n_rows, 0.0);
    ring_emulate(h, n_rows, in.data(), out.data());
    double err = 0;
    for (int r = 0; r < n_rows; r++) {
      double ref = 0, mag = 0;
      for (int k = ip[(size_t)r]; k < ip[(size_t)r + 1]; k++) {
        ref += in[(size_t)ix[(size_t)k]];
        mag += std::fabs(in[(size_t)ix[(size_t)k]]);
      }
      err = std::max(err, std::fabs(out[(size_t)r] - ref) / (mag + 1e-30));
    }
    if (max_rel_err) *max_rel_err = err;
    if (n_blocks) *n_blocks = h.wave_off.back();
  });
}

int pgcn_debug_empty_launches(int n, void *stream) {
  return guarded([&] {
    PGCN_CHECK(n >= 0, PGCN_E_INVALID, "empty_launches: n >= 0");
    launch_empty(n, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_debug_exp_check(const float *x, long long n, float *mine, float *lib, void *stream) {
  return guarded([&] {
    PGCN_CHECK(n >= 0 && (n == 0 || (x && mine && lib)), PGCN_E_INVALID, "exp_check args");
    launch_exp_check(x, n, mine, lib, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_debug_div_check(const float *a, const float *b, long long n, float *q, void *stream) {
  return guarded([&] {
    PGCN_CHECK(n >= 0 && (n == 0 || (a && b && q)), PGCN_E_INVALID, "div_check args");
    launch_div_check(a, b, n, q, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

// ---------------------------------------------------------------- loss kernel family (tests)
}  // extern "C"

namespace {
// the C mirror of XentFinal, checked as the launchers check theirs (and ring_cap, n_w)
void check_final(const pgcn_xent_final *f, const char *what) {
  if (!f) return;
  PGCN_CHECK(f->ticket && f->part4 && f->out2, PGCN_E_INVALID, what);
  PGCN_CHECK(f->group >= 0 && (f->group == 0 || (f->gticket && f->gpart4)), PGCN_E_INVALID, what);
  PGCN_CHECK(f->n_w >= 0 && (f->n_w == 0 || f->w) && (!f->ctr || f->ring_cap >= 1),
             PGCN_E_INVALID, what);
}
XentFinal to_final(const pgcn_xent_final &f) {
  XentFinal x;
  x.w = f.w;
  x.n_w = f.n_w;
  x.wd = f.wd;
  x.out2 = f.out2;
  x.ctr = f.ctr;
  x.ring_cap = f.ctr ? f.ring_cap : 1;
  x.sums = f.sums;
  x.ticket = f.ticket;
  x.part4 = static_cast<float4 *>(f.part4);
  x.group = f.group;
  x.gticket = f.gticket;
  x.gpart4 = static_cast<float4 *>(f.gpart4);
  return x;
}
}  // namespace

extern "C" {

int pgcn_debug_ring_slice_rows(void) { return RING_SR; }

int pgcn_debug_xent_fwd(float *logits, int ld, float *grad, const int *truth, int n, int c,
                        int count, int training, float *partials, int write_back,
                        const pgcn_xent_final *fin, void *stream) {
  return guarded([&] {
    PGCN_CHECK(n >= 0 && c >= 1 && c <= ld && ld <= 124 && ld % 4 == 0 && count >= 0,
               PGCN_E_INVALID, "debug_xent_fwd: 1 <= c <= ld <= 124, ld % 4 == 0");
    PGCN_CHECK(n == 0 || (logits && truth && partials && (grad || !training)), PGCN_E_INVALID,
               "debug_xent_fwd: null argument");
    check_final(fin, "debug_xent_fwd: the finish needs its ticket, partials and output");
    if (n == 0) return;
    XentFinal xf;
    if (fin) xf = to_final(*fin);
    launch_xent_fwd(logits, ld, grad, truth, n, c, count, training, partials, as_stream(stream),
                    write_back != 0, fin ? &xf : nullptr);
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_debug_out_xent(const float *H, int ldh, int kh, const float *W, int ldw, float *logits,
                        int ld, float *grad, const int *truth, int n, int c, int count,
                        int training, float *partials, float *dH, int lddh, float *dWp,
                        float *table, const float *scale, const int *pos, int table_rows,
                        const pgcn_xent_final *fin, void *stream) {
  return guarded([&] {
    PGCN_CHECK(n >= 0 && kh >= 1 && kh <= 16 && ldh >= kh, PGCN_E_INVALID,
               "debug_out_xent: 1 <= kh <= 16, ldh >= kh");
    PGCN_CHECK(c >= 1 && c <= ld && ld <= 116 && ld % 4 == 0 && ldw >= c && count >= 0,
               PGCN_E_INVALID, "debug_out_xent: 1 <= c <= ld <= 116, ld % 4 == 0, ldw >= c");
    PGCN_CHECK(!dH || lddh >= kh, PGCN_E_INVALID, "debug_out_xent: lddh >= kh");
    PGCN_CHECK(!dWp || ld <= 48, PGCN_E_INVALID,
               "debug_out_xent: the weight-grad partial needs <= 48 classes");
    PGCN_CHECK(!table || (kh == 16 && scale && dH && (pos || table_rows >= 0)), PGCN_E_INVALID,
               "debug_out_xent: a prescaled table of a 16-column dH");
    PGCN_CHECK(n == 0 || (H && W && logits && truth && partials && (grad || !training)),
               PGCN_E_INVALID, "debug_out_xent: null argument");
    check_final(fin, "debug_out_xent: the finish needs its ticket, partials and output");
    if (n == 0) return;
    XentFinal xf;
    if (fin) xf = to_final(*fin);
    XentTable tb;
    tb.table = table;
    tb.scale = scale;
    tb.pos = pos;
    tb.rows = table_rows;
    launch_out_xent(H, ldh, kh, W, ldw, logits, ld, grad, truth, n, c, count, training, partials,
                    as_stream(stream), dH, lddh, dWp, table ? &tb : nullptr,
                    fin ? &xf : nullptr);
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_debug_finalize_ring(const float *partials, int n_blocks, int count, const float *w_l2,
                             long long n_l2, float weight_decay, float *out2, const int *ctr,
                             int ring_cap, float *sums, void *stream) {
  return guarded([&] {
    PGCN_CHECK(n_blocks >= 0 && n_l2 >= 0 && (n_l2 == 0 || w_l2) && (!ctr || ring_cap >= 1),
               PGCN_E_INVALID, "debug_finalize_ring args");
    PGCN_CHECK(n_blocks == 0 || (partials && out2), PGCN_E_INVALID,
               "debug_finalize_ring: null argument");
    if (n_blocks == 0) return;
    launch_reduce_scalars(partials, n_blocks, w_l2, n_l2, sums, as_stream(stream), count,
                          weight_decay, out2, ctr, ctr ? ring_cap : 1);
    PGCN_HIP(hipGetLastError());
  });
}

size_t pgcn_debug_tn_reduce_blocks_workspace(int n_blocks, int K, int ldp) {
  if (n_blocks < 0 || K < 1 || ldp < 1) return 0;
  return tn_reduce_blocks_workspace(n_blocks, K, ldp);
}

int pgcn_debug_tn_reduce_blocks(float *partial, int n_blocks, int K, int N, int ldp, float *C,
                                int ldc, void *stream) {
  return guarded([&] {
    PGCN_CHECK(n_blocks >= 0 && K >= 1 && N >= 1 && N <= ldc && ldc <= ldp, PGCN_E_INVALID,
               "debug_tn_reduce_blocks: K >= 1, 1 <= N <= ldc <= ldp");
    PGCN_CHECK(n_blocks == 0 || (partial && C), PGCN_E_INVALID,
               "debug_tn_reduce_blocks: null argument");
    if (n_blocks == 0) return;
    launch_tn_reduce_blocks(partial, n_blocks, K, N, ldp, C, ldc, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_debug_tn_reduce_one_pass(const float *partial, int n, int K, int N, int ldp, float *C,
                                  int ldc, void *stream) {
  return guarded([&] {
    PGCN_CHECK(n >= 0 && K >= 1 && N >= 1 && N <= ldc && ldc <= ldp, PGCN_E_INVALID,
               "debug_tn_reduce_one_pass: K >= 1, 1 <= N <= ldc <= ldp");
    PGCN_CHECK(n == 0 || (partial && C), PGCN_E_INVALID,
               "debug_tn_reduce_one_pass: null argument");
    if (n == 0) return;
    launch_tn_reduce_one_pass(partial, n, K, N, ldp, C, ldc, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_debug_gemm_nib(int M, int N, int K, const float *A, int lda, const float *B, int ldb,
                        int trans_b, float *C, int ldc, const uint64_t *a_mask,
                        long long mask_base, long long mask_ld, float a_scale,
                        const uint64_t *mask_nib, void *stream) {
  return guarded([&] {
    PGCN_CHECK(A && B && C && M >= 0 && K > 0 && ldc >= N, PGCN_E_INVALID, "debug_gemm_nib args");
    launch_gemm_nn(M, N, K, A, lda, B, ldb, trans_b, C, ldc, a_mask, mask_base, mask_ld, a_scale,
                   as_stream(stream), mask_nib);
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_debug_gemm_tn_nib(int M, int N, int K, const float *A, int lda, const float *G, int ldg,
                           float *C, int ldc, const uint64_t *a_mask, long long mask_base,
                           long long mask_ld, float a_scale, const uint64_t *mask_nib,
                           void *workspace, void *stream) {
  return guarded([&] {
    PGCN_CHECK(A && G && C && workspace && K > 0 && ldc >= N, PGCN_E_INVALID,
               "debug_gemm_tn_nib args");
    launch_gemm_tn(M, N, K, A, lda, G, ldg, C, ldc, a_mask, mask_base, mask_ld, a_scale,
                   workspace, as_stream(stream), mask_nib);
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_debug_spmm_csr(int m, int p, int ldc, const int *indptr, const int *indices,
                        const float *a, const uint64_t *mask, long long mask_base, float scale,
                        const float *b, float *c, float *c2, void *stream) {
  return guarded([&] {
    PGCN_CHECK(m >= 0 && p >= 1 && ldc >= p && mask_base >= 0, PGCN_E_INVALID,
               "debug_spmm_csr: m >= 0, 1 <= p <= ldc, mask_base >= 0");
    PGCN_CHECK(m == 0 || (indptr && indices && a && b && c), PGCN_E_INVALID,
               "debug_spmm_csr: null argument");
    if (c2)
      launch_spmm_csr_dual(m, p, ldc, indptr, indices, a, mask, mask_base, scale, b, c, c2,
                           as_stream(stream));
    else
      launch_spmm_csr(m, p, ldc, indptr, indices, a, mask, mask_base, scale, b, c,
                      as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_debug_spmm_csc_bwd(int nf, int p, int ldg, const int *csc_ptr, const int *csc_row,
                            const int *csc_pos, const float *a, const uint64_t *mask,
                            long long mask_base, float scale, const float *cgrad, float *bgrad,
                            long long nnz, const int *order, int tree, void *stream) {
  return guarded([&] {
    PGCN_CHECK(nf >= 0 && p >= 1 && ldg >= p && mask_base >= 0 && nnz >= 0, PGCN_E_INVALID,
               "debug_spmm_csc_bwd: nf >= 0, 1 <= p <= ldg, mask_base >= 0, nnz >= 0");
    PGCN_CHECK(nf == 0 || (csc_ptr && csc_row && csc_pos && a && cgrad && bgrad), PGCN_E_INVALID,
               "debug_spmm_csc_bwd: null argument");
    launch_spmm_csc_bwd(nf, p, ldg, csc_ptr, csc_row, csc_pos, a, mask, mask_base, scale, cgrad,
                        bgrad, as_stream(stream), nnz, order, tree != 0);
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_debug_dropout_mask(uint64_t *states, long long n_chunks, long long elem0,
                            long long elem_end, float p, uint64_t *mask, const void *table,
                            int per, int max_blocks, void *stream) {
  return guarded([&] {
    PGCN_CHECK(n_chunks >= 0 && max_blocks >= 0 && (n_chunks == 0 || (states && mask && table)),
               PGCN_E_INVALID, "debug_dropout_mask args");
    launch_dropout_mask(states, n_chunks, elem0, elem_end, p, mask, table, as_stream(stream),
                        max_blocks, per);
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_debug_dropout_mask2(uint64_t *states0, long long n_chunks0, long long elem0_0,
                             long long elem_end0, float p0, uint64_t *mask0, int per0,
                             uint64_t *states1, long long n_chunks1, long long elem0_1,
                             long long elem_end1, float p1, uint64_t *mask1, int per1,
                             const void *table, void *stream) {
  return guarded([&] {
    PGCN_CHECK(n_chunks0 >= 0 && n_chunks1 >= 0 && (n_chunks0 == 0 || (states0 && mask0)) &&
                   (n_chunks1 == 0 || (states1 && mask1)) &&
                   (n_chunks0 + n_chunks1 == 0 || table),
               PGCN_E_INVALID, "debug_dropout_mask2 args");
    const MaskDraw d0{states0, n_chunks0, elem0_0, elem_end0, p0, mask0, per0};
    const MaskDraw d1{states1, n_chunks1, elem0_1, elem_end1, p1, mask1, per1};
    launch_dropout_mask2(d0, d1, table, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

int pgcn_debug_dropout_apply(float *x, long long n, const uint64_t *mask, long long base,
                             float scale, void *stream) {
  return guarded([&] {
    PGCN_CHECK(n >= 0 && base >= 0 && (n == 0 || (x && mask)), PGCN_E_INVALID,
               "debug_dropout_apply args");
    launch_dropout_apply_based(x, n, mask, base, scale, as_stream(stream));
    PGCN_HIP(hipGetLastError());
  });
}

long long pgcn_debug_path_count(const char *name, int reset) {
  const bool thread = (reset & 2) != 0, zero = (reset & 1) != 0;
  if (reset & ~3) return PGCN_E_INVALID;
  if (!name) {
    if (!zero) return PGCN_E_INVALID;
    for (int p = 0; p < KP_COUNT; p++) {
      if (thread) pgcn::t_path_hits[p] = 0;
      else pgcn::g_path_hits[p].store(0);
    }
    return 0;
  }
  for (int p = 0; p < KP_COUNT; p++)
    if (!std::strcmp(name, pgcn::kPathNames[p])) {
      if (thread) {
        const long long n = pgcn::t_path_hits[p];
        if (zero) pgcn::t_path_hits[p] = 0;
        return n;
      }
      return zero ? pgcn::g_path_hits[p].exchange(0) : pgcn::g_path_hits[p].load();
    }
  return PGCN_E_INVALID;
}

// ---------------------------------------------------------------- partition (host only)
int pgcn_partition_bounds(int n, const int *indptr, int world, int *bounds_out, int *maxrows) {
  return guarded([&] {
    Partition p = make_partition(n, indptr, world, 0);
    std::memcpy(bounds_out, p.bounds.data(), sizeof(int) * (size_t)(world + 1));
    if (maxrows) *maxrows = p.maxrows;
  });
}

// Rank `rank`'s column block in the padded row layout (sizes: call with null arrays first
// to get nnz; indptr needs world*maxrows+1 entries).
long long pgcn_partition_subgraph(int n, const int *indptr, const int *indices, int world,
                                  int rank, int *sub_indptr, int *sub_indices, float *sub_vals) {
  long long nnz = -1;
  const int st = guarded([&] {
    Partition p = make_partition(n, indptr, world, rank);
    std::vector<int> sp, si;
    std::vector<float> sv;
    partition_subgraph(p, n, indptr, indices, &sp, &si, &sv);
    nnz = (long long)si.size();
    if (sub_indptr) std::memcpy(sub_indptr, sp.data(), sp.size() * sizeof(int));
    if (sub_indices) std::memcpy(sub_indices, si.data(), si.size() * sizeof(int));
    if (sub_vals) std::memcpy(sub_vals, sv.data(), sv.size() * sizeof(float));
  });
  return st == PGCN_OK ? nnz : st;
}

}  // extern "C"
