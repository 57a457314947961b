/* include/pgcn.h -- the drop-in C ABI of the MI355X GCN engine (libpgcn.so).
 *
 * Two layers, both plain C: caller-owned device pointers, sizes, a hipStream_t passed as
 * `void *`, int status returns (0 = OK, >0 = hipError_t, <0 = PGCN_E_*). Kernel entry
 * points never allocate (workspace is passed in or owned by a handle created beforehand),
 * are asynchronous on the given stream and are safe to capture into a hipGraph.
 *
 *  (1) Kernel ABI -- one entry per reference kernel family it replaces
 *      (reference: src/module.cu, src/optim.cu, src/gcn.cu of parallel-GCN).
 *  (2) Engine ABI -- the GCN object of include/gcn.cuh (ctor + train_epoch/eval/run),
 *      plus the edge-cut multi-GPU variant (new: the reference is single-GPU).
 *
 * The reference's C++ classes (Module and its subclasses, Variable, Adam, GCN, Parser) with
 * their constructor shapes are published in include/pgcn.hpp (namespace pgcn::api, the same
 * library); INTEGRATION.md shows the bindings a reference maintainer would add.
 */
#ifndef PGCN_H
#define PGCN_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGCN_OK 0
#define PGCN_E_INVALID (-1)   /* bad argument / shape */
#define PGCN_E_NOMEM (-2)     /* device allocation failed */
#define PGCN_E_IO (-3)        /* dataset could not be read (Parser::parse() == false) */
#define PGCN_E_COMM (-4)      /* RCCL error */
#define PGCN_E_NODEVICE (-5)  /* no HIP device: the product has no CPU fallback */

const char *pgcn_status_string(int status);
int pgcn_version(void);

/* ===================================================================================== */
/* (1) Kernel ABI                                                                          */
/* ===================================================================================== */

/* --- xorshift128+ (hpdga-spring23/src/rand.cpp:17-28), host helpers ------------------- */
/* Default seed state of hpdga init_rand_state() (rand.cpp:6-14). */
void pgcn_rng_seed(uint64_t state[2]);
/* the same two draws after srand(seed), on a private glibc random_r state */
void pgcn_rng_seed_glibc(unsigned int seed, uint64_t state[2]);
/* state <- state advanced by `k` draws (GF(2) jump-ahead; exact). */
void pgcn_rng_jump(uint64_t state[2], uint64_t k);

/* --- Graph (DevSparseIndex + precomputed Â values; include/sparse.cuh:21-29,
 *     src/parser.cpp:164-181) ------------------------------------------------------------ */
typedef struct pgcn_graph pgcn_graph;
/* Uploads a CSR adjacency (implicit self loops already present, as the hpdga Parser builds
 * it), computes coef = 1/sqrtf(deg_src*deg_dst) bit-exactly as hpdga module.cpp:88-90 and
 * builds the wavefront work schedule. Host pointers. */
int pgcn_graph_create(int n_nodes, const int *indptr, const int *indices, pgcn_graph **out);
/* The reference's full GraphSum contract (include/module.cuh:82, the dev_graph_value array of
 * src/gcn.cu:30-43): any per-slot values, aligned with `indices` (host pointers).  Values equal
 * to the parser's coefficients (as pgcn_graph_create computes them) take the LDS ring path;
 * any other values take the per-edge gather kernels.  The pattern need not be symmetric (the
 * call is out = A in for the given A; the engine's backward identity needs A = A^T). */
int pgcn_graph_create_values(int n_nodes, const int *indptr, const int *indices,
                             const float *values, pgcn_graph **out);
int pgcn_graph_destroy(pgcn_graph *g);
long long pgcn_graph_nnz(const pgcn_graph *g);
/* out[i, 0:dim] = sum_j coef_ij * in[j, 0:dim]  (GraphSum::forward/backward,
 * src/module.cu:172-210; the backward is the same gather on grads because Â is symmetric).
 * Row-major, leading dims ld_in/ld_out (multiples of 4, >= dim). Device pointers. */
int pgcn_graphsum(const pgcn_graph *g, const float *in, int ld_in, float *out, int ld_out,
                  int dim, void *stream);

/* --- dense GEMMs on fp32 MFMA (Matmul, src/module.cu:274-472; dense X * W1) ------------- */
/* C[M,N] = A[M,K] * op(B)   (op(B) = B[K,N] if trans_b == 0 else B^T with B stored [N,K]).
 * Optional dropout on A: element (m,k) is kept iff bit (mask_base + m*mask_ld + k) of
 * `a_mask` is set, kept values scaled by `a_scale` (a_mask NULL: no dropout). */
int pgcn_gemm(int M, int N, int K, const float *A, int lda, const float *B, int ldb, int trans_b,
              float *C, int ldc, const uint64_t *a_mask, long long mask_base, long long mask_ld,
              float a_scale, void *stream);
/* C[K,N] = A[M,K]^T * G[M,N], reduced over M deterministically (split-M slabs + ordered
 * reduction; replaces the atomicAdd kernels matmul_kernel_backward_2 and
 * sparse_matmul_kernel_backward). `workspace` >= pgcn_gemm_tn_workspace(M,N,K) bytes. */
size_t pgcn_gemm_tn_workspace(int M, int N, int K);
int pgcn_gemm_tn(int M, int N, int K, const float *A, int lda, const float *G, int ldg,
                 float *C, int ldc, const uint64_t *a_mask, long long mask_base,
                 long long mask_ld, float a_scale, void *workspace, void *stream);

/* X-stream forms of the two contractions over the dense feature matrix (N <= 16, K <= 640;
 * SparseMatmul::forward/backward on dense X, src/module.cu:104-163), with the dropout keep
 * bits in the "nibble" layout: mask_nib[m][j] (16 words per row) holds in nibble c the bits of
 * A[m][64c + 4j .. 64c + 4j + 3].  pgcn_mask_nibbles builds it from the flat bitmap of
 * pgcn_gemm (bit mask_base + m*mask_ld + k).  mask_nib NULL: no dropout.  The TN form needs
 * pgcn_gemm_tn_workspace(M, N, K) bytes of workspace.  Same results as pgcn_gemm /
 * pgcn_gemm_tn up to fp32 summation order. */
int pgcn_mask_nibbles(const uint64_t *mask, long long mask_base, long long mask_ld, int M, int K,
                      uint64_t *mask_nib, void *stream);
int pgcn_gemm_xstream(int M, int N, int K, const float *A, int lda, const float *B, int ldb,
                      int trans_b, float *C, int ldc, const uint64_t *mask_nib, float a_scale,
                      void *stream);
/* Both first-layer products from one pass over A: C = A B (no dropout) and C2 = drop(A) B,
 * C2 bit-identical to pgcn_gemm_xstream with the same mask.  The engine uses it for eval's
 * forward together with the next training forward (same weights: no optimizer step between),
 * replacing the reference's two separate SparseMatmul::forward passes (src/module.cu:104-126,
 * called by src/gcn.cu:293-343). */
int pgcn_gemm_xstream_dual(int M, int N, int K, const float *A, int lda, const float *B, int ldb,
                           int trans_b, float *C, float *C2, int ldc, const uint64_t *mask_nib,
                           float a_scale, void *stream);
int pgcn_gemm_tn_xstream(int M, int N, int K, const float *A, int lda, const float *G, int ldg,
                         float *C, int ldc, const uint64_t *mask_nib, float a_scale,
                         void *workspace, void *stream);
/* The same products with the flat bitmap itself (keep bit of A[m][k] at mask_base + m*K + k;
 * mask_words uint64 words at mask, an even count), which the engine passes on the shapes the
 * loader-wave kernels take (K in 577..640, lda = K rounded up to 4; others: PGCN_E_INVALID):
 * their loader waves stage each 16-row group's bits beside its rows, no pgcn_mask_nibbles
 * pass.  C2 NULL: the single product.  Bit-identical to the nibble forms with the nibbles of
 * the same bitmap. */
int pgcn_gemm_xstream_flat(int M, int N, int K, const float *A, int lda, const float *B, int ldb,
                           int trans_b, float *C, float *C2, int ldc, const uint64_t *mask,
                           long long mask_base, long long mask_words, float a_scale, void *stream);
int pgcn_gemm_tn_xstream_flat(int M, int N, int K, const float *A, int lda, const float *G, int ldg,
                              float *C, int ldc, const uint64_t *mask, long long mask_base,
                              long long mask_words, float a_scale, void *workspace, void *stream);

/* --- sparse X (SparseMatmul, src/module.cu:104-163) ----------------------------------- */
/* c[i,:] = sum_jj drop(a[jj]) * b[indices[jj], :], CSR order (bit-exact vs hpdga). */
int pgcn_spmm_csr(int m, int p, const int *indptr, const int *indices, const float *a,
                  const uint64_t *a_mask, float a_scale, const float *b, float *c, void *stream);
/* bgrad[f,:] = sum over (i,jj) with indices[jj]==f, in CSR order: drop(a[jj]) * cgrad[i,:],
 * using the transposed index (csc_ptr/csc_row/csc_pos) built by pgcn_csr_transpose. */
int pgcn_spmm_csc_bwd(int n_features, int p, const int *csc_ptr, const int *csc_row,
                      const int *csc_pos, const float *a, const uint64_t *a_mask, float a_scale,
                      const float *cgrad, float *bgrad, void *stream);
/* host helper: CSR (m rows, nnz, column ids < n_cols) -> CSC with original positions */
int pgcn_csr_transpose(int m, int n_cols, const int *indptr, const int *indices, int *csc_ptr,
                       int *csc_row, int *csc_pos);

/* --- dropout (Dropout, src/module.cu:16-99; hpdga module.cpp:208-228) ------------------ */
/* Bit-exact hpdga masks: chunk c holds the xorshift128+ state at the draw that element
 * 64*c of the variable consumes.  One call generates words [c0, c0+n_chunks) and advances
 * every chunk state by `period` draws via the byte tables built by pgcn_rng_jump_table. */
int pgcn_rng_jump_table(uint64_t period, void *host_table /* 16*256*16 bytes */);
int pgcn_dropout_mask(uint64_t *chunk_states, long long n_chunks, long long n_elems,
                      long long elem0, float p, uint64_t *mask, const void *dev_jump_table,
                      void *stream);
/* x[i] *= bit(i) ? scale : 0 for i in [0,n) (also the backward on grads). */
int pgcn_dropout_apply(float *x, long long n, const uint64_t *mask, float scale, void *stream);

/* --- ReLU (src/module.cu:215-265) ------------------------------------------------------- */
int pgcn_relu_fwd(float *x, long long n, uint8_t *mask, int training, void *stream);
int pgcn_relu_bwd(float *g, long long n, const uint8_t *mask, void *stream);

/* --- ResidualConnection (src/module.cu:566-593) ------------------------------------------
 * forward: cur[i] += prev[i]; backward (empty in the reference): prev_grad[i] += cur_grad[i].
 * One fp32 add per element, any alignment; the arrays must not overlap. */
int pgcn_residual_fwd(float *cur, const float *prev, long long n, void *stream);
int pgcn_residual_bwd(float *prev_grad, const float *cur_grad, long long n, void *stream);

/* --- LayerNorm over the columns of a node variable (new: the reference has no such module) -
 * forward: y [n][ld_y] = gamma * xhat + beta with xhat = (x - mean_row(x)) * rstd and rstd =
 * 1 / sqrtf(var_row(x) + eps), the biased variance over the d columns, mean and variance in two
 * passes over the row.  1 <= d <= 1024; every ld a multiple of 4 and >= d; every row 16-byte
 * aligned; gamma, beta [d].  The float4s covering columns [0, round_up4(d)) of y are written,
 * zero from column d on; columns beyond them are left alone.  Padding columns of x are never
 * read into the result.  x == y (in place) is allowed.  xhat [n][ld_xhat] and rstd [n] (both or
 * neither; a training forward) receive the normalised rows and the row scales the backward
 * reads.
 * backward: dx = rstd * (g - mean_row(g) - xhat * mean_row(g * xhat)) with g = dy * gamma (dx
 * == dy allowed); dgamma[c] = sum over the rows of dy * xhat, dbeta[c] = sum of dy.  The column
 * sums go through per-workgroup partials in `workspace` (pgcn_layernorm_bwd_workspace(n, d)
 * bytes) and one reducing launch, in an order that depends on (n, d) only: two calls give the
 * same bits.  No float atomics.
 * PGCN_E_INVALID for bad arguments (nothing is launched); n == 0 launches nothing; the calls are
 * asynchronous on `stream`, allocate nothing and may be captured. */
int pgcn_layernorm_fwd(const float *x, int ld_x, float *y, int ld_y, int n, int d,
                       const float *gamma, const float *beta, float eps, float *xhat,
                       int ld_xhat, float *rstd, void *stream);
size_t pgcn_layernorm_bwd_workspace(int n, int d);
int pgcn_layernorm_bwd(const float *dy, int ld_dy, const float *xhat, int ld_xhat,
                       const float *rstd, const float *gamma, int n, int d, float *dx, int ld_dx,
                       float *dgamma, float *dbeta, void *workspace, void *stream);
/* The forward with the engine's fused tail in its final write (kernel tests): after the
 * LayerNorm, pgcn_relu_fwd (relu_mask [n][relu_ld] bytes, NULL: no mask kept), pgcn_residual_fwd
 * (res [n][res_ld], NULL: none) and pgcn_dropout_apply (keep bit drop_base + r * d + c of
 * drop_mask, NULL: none), bit for bit.  Needs ld_y == d, relu_ld and res_ld multiples of 4 and
 * >= d. */
int pgcn_debug_layernorm_fwd_tail(const float *x, int ld_x, float *y, int ld_y, int n, int d,
                                  const float *gamma, const float *beta, float eps, float *xhat,
                                  int ld_xhat, float *rstd, uint8_t *relu_mask, int relu_ld,
                                  const float *res, int res_ld, const uint64_t *drop_mask,
                                  long long drop_base, float drop_scale, void *stream);

/* --- graph attention over a node variable (new: the reference has one aggregation) ---------
 * Single head, additive (GAT).  `g` comes from pgcn_graph_create with a square pattern; its
 * values are not used.  Every CSR slot s = (i, j) counts as the pattern has it (self loops, a
 * duplicated edge twice).  With P [n][ld_p] and the attention vectors a_dst, a_src [d]:
 *   pgcn_gat_scores: u[i] = P_i . a_dst, v[i] = P_i . a_src (one pass over P).
 *   pgcn_gat_fwd:    e_s = x > 0 ? x : slope x with x = u[i] + v[j] (strict >), alpha_s = exp(e_s -
 *     max_row) / sum_row exp(e - max_row), Z_i = sum over row i's slots of alpha_s P_j.  A row
 *     without a slot gives Z_i = 0.  alpha [nnz] (may be NULL; a training forward) receives the
 *     slot weights the backward reads.
 *   pgcn_gat_bwd:    with G [n][ld_g] = dLoss/dZ and the forward's u, v, alpha, Z: dx_s = alpha_s
 *     (G_i . P_j - G_i . Z_i) (x_s > 0 ? 1 : slope), du_i / dv_j its sums over row i / over the
 *     slots into column j; dP_j = sum over the slots into j of alpha_s G_i + du_j a_dst + dv_j
 *     a_src; da [2][d] = {sum du_i P_i, sum dv_j P_j} (a_dst's gradient, then a_src's).
 *     `workspace`: pgcn_gat_bwd_workspace(g, d) bytes, 16-byte aligned (dx per slot, du, dv and
 *     the partial sums): the value of pgcn_gat_bwd_workspace_mh(g, d, 1), whose long columns'
 *     segment partials are 192 floats each.  d is passed (after ld_dp): the widths cannot be
 *     told from the strides.
 * These three entries are the _mh entries below at heads = 1 without a mask, behind their own
 * argument checks: one set of kernels serves both.
 * 1 <= d <= 128; every ld a multiple of 4 and >= d; every row 16-byte aligned.  The float4s
 * covering columns [0, round_up4(d)) of Z and dP are written, zero from column d on; columns
 * beyond them are left alone.  Padding columns of P, Z and G are never read into the result.
 * The sums into a column walk the transposed index in CSR order (a store pass per slot, then a
 * sum pass per destination); rows and columns longer than 512 slots are cut into 512-slot
 * segments summed by separate waves and merged in segment order; da goes through per-workgroup
 * partials and one reducing launch.  Every order depends on the pattern and d only: two calls
 * give the same bits.  No float atomics.
 * PGCN_E_INVALID (before anything touches the device) for d outside [1, 128], an ld that is not
 * a multiple of 4 or below d, a null required pointer; n == 0 launches nothing.  Asynchronous on
 * `stream`, allocate nothing and may be captured -- after the graph's first attention call,
 * which builds and uploads the transposed index (pgcn_gat_bwd_workspace does it too).  The
 * forward keeps its long rows' partial sums in the graph: two forwards on one graph must not
 * run side by side. */
int pgcn_gat_scores(const float *P, int ld_p, int n, int d, const float *a_dst,
                    const float *a_src, float *u, float *v, void *stream);
int pgcn_gat_fwd(const pgcn_graph *g, const float *P, int ld_p, const float *u, const float *v,
                 float slope, float *Z, int ld_z, int d, float *alpha /* [nnz] or NULL */,
                 void *stream);
size_t pgcn_gat_bwd_workspace(const pgcn_graph *g, int d);
int pgcn_gat_bwd(const pgcn_graph *g, const float *P, int ld_p, const float *u, const float *v,
                 float slope, const float *alpha, const float *Z, int ld_z, const float *G,
                 int ld_g, const float *a_dst, const float *a_src, float *dP, int ld_dp, int d,
                 float *da /* [2][d]: dst, src */, void *workspace, void *stream);

/* Several heads, and dropout on the attention weights.  Head h of `heads` owns columns [h dh,
 * (h + 1) dh) of P, Z, G, dP, a_dst and a_src, dh = d / heads, and runs the formulas above on its
 * slice with a softmax of its own: u, v are [n][heads], alpha [nnz][heads] (slot-major), the
 * concatenated heads fill the d columns of Z.  With a mask (a training forward and its backward):
 *   m'_s^h = bit (drop_base + s heads + h) of drop_mask ? drop_scale : 0
 *   Z_i[h] = sum_row alpha_s^h m'_s^h P_j[h]
 *   dx_s^h = alpha_s^h (m'_s^h G_i[h] . P_j[h] - G_i[h] . Z_i[h]) (x_s^h > 0 ? 1 : slope)
 *   dP_j[h] = sum into column j of alpha_s^h m'_s^h G_i[h] + du_j^h a_dst[h] + dv_j^h a_src[h]
 * drop_mask is a device bit array (bit b = word b / 64, bit b % 64: the triple the fused GraphSum
 * entries take) or NULL for no dropout; alpha receives the weights BEFORE dropout (each head's
 * sum to 1 per row) and is required with a mask.
 * heads == 1: any d in 1..128; without a mask this is what pgcn_gat_scores / _fwd / _bwd run
 * (the same kernels, the same bits); one head under an all-ones mask of scale 1 gives those bits
 * too.
 * heads > 1: heads divides d and dh is 4, 8, 16, 32, 64 or 128 -- a lane's float4 then belongs to
 * one head and a head is an aligned power-of-two group of lanes; anything else is
 * PGCN_E_INVALID before anything touches the device, like the checks of the entries above.
 * Every head shares one pass over a row's or column's index and one load of each neighbour row:
 * a call launches as many kernels as the single-head call on the same graph.  No float atomics;
 * every summation order depends on the pattern, d and heads only.
 * `workspace`: pgcn_gat_bwd_workspace_mh(g, d, heads) bytes (dx [nnz][heads], du, dv
 * [n][heads], the partial sums); it does not depend on whether a mask is passed. */
int pgcn_gat_scores_mh(const float *P, int ld_p, int n, int d, int heads, const float *a_dst,
                       const float *a_src, float *u /* [n][heads] */, float *v, void *stream);
int pgcn_gat_fwd_mh(const pgcn_graph *g, const float *P, int ld_p, const float *u, const float *v,
                    float slope, float *Z, int ld_z, int d, int heads, const uint64_t *drop_mask,
                    long long drop_base, float drop_scale,
                    float *alpha /* [nnz][heads]; NULL only without a mask */, void *stream);
size_t pgcn_gat_bwd_workspace_mh(const pgcn_graph *g, int d, int heads);
int pgcn_gat_bwd_mh(const pgcn_graph *g, const float *P, int ld_p, const float *u, const float *v,
                    float slope, const float *alpha, const float *Z, int ld_z, const float *G,
                    int ld_g, const float *a_dst, const float *a_src, float *dP, int ld_dp, int d,
                    int heads, const uint64_t *drop_mask, long long drop_base, float drop_scale,
                    float *da /* [2][d]: dst, src */, void *workspace, void *stream);

/* --- GraphSAGE aggregators over the CSR slots of a square pattern (k_sage.hip) ---------------
 * Max (new kernels).  `g` comes from pgcn_graph_create* with a square pattern; its values are
 * not used, and nnz must fit an int.  Slot s = (i, j) is global position s of `indices`.
 *   pgcn_agg_max_fwd: out_i[c] = add_i[c] + max over row i's slots of in_j[c] -- the maximum is
 *     exact and the add is one fp32 add (add == NULL: the maximum itself).  arg_i[c] (arg may be
 *     NULL: an inference call) is the slot whose in_j[c] is that maximum.  A candidate replaces
 *     the incumbent only when strictly greater (the project's tie rule), so among equal values --
 *     -0.0 and +0.0 are equal -- the LOWEST slot wins, however the slots are dealt to lanes.  A row
 *     without a slot: out_i = add_i (or 0), arg_i = -1.  Inputs are taken as finite.
 *   pgcn_agg_max_bwd: with G [n][ld_g] = dLoss/dout and the forward's arg, din_j[c] = sum over
 *     the slots s = (i, j) into column j with arg_i[c] == s of G_i[c]: every gradient element
 *     goes to the one slot that won.  The sum walks the transposed index in CSR order (the
 *     pattern need not be symmetric); a column without incoming slots gives a zero row.  The
 *     gradient of `add` is G itself.
 * 1 <= d <= 128; every ld a multiple of 4 and >= d, rows 16-byte aligned.  The float4s / int4s
 * covering [0, round_up4(d)) of out, arg and din are written -- 0 (arg: -1) from column d on --
 * and columns beyond them are left alone; padding columns of in, add, G and arg may hold
 * anything and never reach a result.  Anything else is PGCN_E_INVALID before anything touches
 * the device.  The calls are asynchronous and allocate nothing -- a graph's first call builds
 * and uploads its transposed index and segment lists and allocates the segment partials of its
 * rows / columns longer than 512 slots, which live in the graph, so two calls on one graph must
 * not overlap -- and may be captured after it.  No float atomics: every order depends on the
 * pattern and d only, so two calls give the same bits.
 * Mean (no new kernel): pgcn_graph_create_mean builds the graph whose pgcn_graphsum is the mean
 * forward (transpose = 0: the pattern with 1 / len_i on every slot of row i, out_i = (1 / len_i)
 * sum in_j) or backward (transpose = 1: the transposed pattern, host side as
 * pgcn_csr_transpose orders it, whose slot (j, i) carries 1 / len_i: out_j = sum over the slots
 * into column j of in_i / len_i).  1 / len_i is one 1.0f / (float)len_i, len_i the CSR row
 * length as given.  The values factor into (row scale, column scale) = (1 / len, 1) resp.
 * (1, 1 / len), so pgcn_graphsum takes whatever kernel the width and size select, the LDS ring
 * schedule included. */
int pgcn_graph_create_mean(int n_nodes, const int *indptr, const int *indices, int transpose,
                           pgcn_graph **out);
int pgcn_agg_max_fwd(const pgcn_graph *g, const float *in, int ld_in, int d,
                     const float *add /* [n][ld_add] or NULL */, int ld_add, float *out,
                     int ld_out, int *arg /* [n][ld_arg] or NULL */, int ld_arg, void *stream);
int pgcn_agg_max_bwd(const pgcn_graph *g, const float *G, int ld_g, const int *arg, int ld_arg,
                     int d, float *din, int ld_din, void *stream);

/* --- graph-level readout over contiguous row ranges (k_readout.hip; new: the reference has
 *     no graph-level model) -------------------------------------------------------------------
 * A batch of G graphs is one node variable whose rows [graph_ptr[g], graph_ptr[g + 1]) belong to
 * graph g: graph_ptr [G + 1] (a DEVICE array), non-decreasing, graph_ptr[0] = 0, graph_ptr[G] = n;
 * len_g is the range's length.  The adjacency pattern is not looked at.
 *   pgcn_readout_fwd, mode PGCN_READOUT_SUM: out_g = sum of in_i over the range; _MEAN: that sum
 *     times one 1.0f / (float)len_g (the mean aggregator's form); _MAX: the exact maximum per
 *     column, arg_g[c] (arg may be NULL: an inference call) the row that holds it -- a candidate
 *     replaces the incumbent only when strictly greater (pgcn_agg_max_fwd's rule), so among equal
 *     values, -0.0 and +0.0 included, the LOWEST row wins.  An empty range: a zero row, arg -1.
 *     arg is written by every mode that is given one (-1 for sum and mean).
 *     max_len (a host value): the longest range's length, or any upper bound of it (n when
 *     unknown).  Up to pgcn_readout_chunk_rows() = T the call is ONE kernel launch, a wave per
 *     range, four ranges per workgroup step.  Above T the ranges longer than T take two more
 *     launches: they are cut where the row index is a multiple of T, a 256-thread workgroup per
 *     T-row block reduces the block's piece of the (at most two) long ranges that meet it into
 *     `workspace` (pgcn_readout_workspace(n) bytes, 16-byte aligned; may be NULL when max_len <=
 *     T), and a workgroup per long range reduces its pieces in order.  A max_len below the truth
 *     costs time, never correctness: the one-launch form handles any length.
 *   pgcn_readout_bwd: with G_out [G][ld_g] = dLoss/dout, node_graph [n] (device; the range of
 *     every row) and the forward's arg: din_i = g_{graph(i)} (sum), g * (1.0f / (float)len) (mean),
 *     g[c] where arg[graph(i)][c] == i and 0 elsewhere (max; arg is required then).  Every row of
 *     din is written (a row whose node_graph is outside [0, G): zero).
 * 1 <= d <= 128; every ld a multiple of 4 and >= d, rows 16-byte aligned.  The float4s / int4s
 * covering [0, round_up4(d)) of out, arg and din are written -- 0 (arg: -1) from column d on --
 * and columns beyond them are left alone; padding columns of in, G_out and arg may hold anything,
 * NaN included, and never reach a result.  Inputs are taken as finite.  Anything else is
 * PGCN_E_INVALID before anything touches the device.  The calls are asynchronous, allocate
 * nothing and may be captured.  No float atomics: every summation order depends on graph_ptr and
 * d only (and on whether max_len exceeds T), so two calls give the same bits. */
#define PGCN_READOUT_NONE 0
#define PGCN_READOUT_SUM 1
#define PGCN_READOUT_MEAN 2
#define PGCN_READOUT_MAX 3
int pgcn_readout_chunk_rows(void);
size_t pgcn_readout_workspace(int n);
int pgcn_readout_fwd(const float *in, int ld_in, const int *graph_ptr, int G, int n, int d,
                     int mode, int max_len, float *out, int ld_out,
                     int *arg /* [G][ld_arg] or NULL */, int ld_arg, void *workspace,
                     void *stream);
int pgcn_readout_bwd(const float *G_out, int ld_g, const int *graph_ptr, const int *node_graph,
                     const int *arg /* max only */, int ld_arg, int G, int n, int d, int mode,
                     float *din, int ld_din, void *stream);

/* --- link prediction: pair scores over a node variable (k_link.hip; new: the reference has no
 *     pair-level model) ------------------------------------------------------------------------
 * pgcn_links is an opaque pair index, in the manner of pgcn_graph: n_pairs pairs (src_e, dst_e) of
 * nodes in [0, n_nodes), all host arrays.  Every pair enters the forward; a pair enters the
 * backward iff select == NULL or select[e] >= 0.  pgcn_links_create uploads src / dst and builds
 * the INCIDENCE INDEX on the host: each node's list of (pair e, other endpoint) over the selected
 * pairs that touch it, in ascending e, the entry of a pair's src role before that of its dst role
 * -- a self pair (i, i) gives two consecutive entries in node i's list, a duplicated pair counts
 * as often as it is listed.  Lists longer than pgcn_link_segment_slots() = T entries are cut into
 * T-entry segments.  pgcn_links_slots: the incidence entries, 2 x the selected pairs.
 * PGCN_E_INVALID: an endpoint outside [0, n_nodes), 2^30 or more selected pairs (the entries are
 * indexed by int), n_pairs beyond an int.  The segment partials of the backward live in the
 * handle: two backward calls on one handle must not overlap (the pgcn_agg_max_* contract).
 *   pgcn_link_score_fwd, ONE launch: scores[e][0] = sum_c H[src_e][c] * H[dst_e][c] over c < d; the
 *     float4 at scores[e][0..3] is written as {s, 0, 0, 0}, columns behind it are left alone.  GL
 *     lanes take one pair (GL by width as for the attention kernels), each lane multiplies its
 *     float4 of the two rows and the lanes of a group are summed by xor butterflies over the
 *     offsets 1 .. GL / 2: a fixed order.
 *   pgcn_link_score_bwd, one launch, two when any list exceeds T: with G[e][0] = dLoss/dscore_e,
 *     dH_i[c] = sum over node i's incidence entries (e, o) of G[e][0] * H[o][c].  EVERY row of dH
 *     is written: the float4s covering [0, round_up4(d)), zero from column d on and for a node
 *     without entries; columns beyond are left alone.  G of an unselected pair is never read.
 * 1 <= d <= 128; every ld a multiple of 4 and >= d (>= 1 for scores and G), rows 16-byte aligned;
 * padding columns of H may hold anything, NaN included, and never reach a result.  Anything else
 * is PGCN_E_INVALID before anything touches the device.  n_pairs == 0 launches nothing.  The
 * calls are asynchronous, allocate nothing and may be captured.  No float atomics: every
 * summation order depends on the pair list and d only, so two calls give the same bits. */
typedef struct pgcn_links pgcn_links;
int pgcn_links_create(int n_nodes, long long n_pairs, const int *src, const int *dst,
                      const int *select /* [n_pairs] or NULL */, pgcn_links **out);
int pgcn_links_destroy(pgcn_links *l);
int pgcn_link_segment_slots(void);
long long pgcn_links_slots(const pgcn_links *l);
int pgcn_link_score_fwd(const pgcn_links *l, const float *H, int ld_h, int d, float *scores,
                        int ld_s, void *stream);
int pgcn_link_score_bwd(const pgcn_links *l, const float *H, int ld_h, int d, const float *G,
                        int ld_g /* dLoss/dscore = G[e][0] */, float *dH, int ld_dh,
                        void *stream);
/* host-only (no device): the incidence index pgcn_links_create would build -- ptr [n_nodes + 1],
 * pair and other [ptr[n_nodes]] (either may be NULL: call once for ptr, then again) */
int pgcn_debug_links_incidence(int n_nodes, long long n_pairs, const int *src, const int *dst,
                               const int *select, int *ptr, int *pair, int *other);

/* --- link prediction: 1-vs-all ranking counts (k_rank.hip; new: the reference has no pair-level
 * model).  For a held-out link (anchor a, target t) ranking metrics ask where t stands among all
 * candidates v for a.  The rank score over an embedding H [n][ld_h] of logical width d is the
 * k-ordered fp32 fused chain
 *     r(a, v) = s_d,  s_0 = 0,  s_{c+1} = fmaf(H[a][c], H[v][c], s_c)  for c = 0 .. d - 1
 * -- deliberately NOT pgcn_link_score_fwd's order (float4 partials met in xor butterflies): a chain
 * is what the f32 MFMA computes bit for bit, so every kernel below produces the same bits for the
 * same (a, v) and scores are compared with > and == exactly.  Columns >= d are never read into a
 * result (the padding may hold NaN); inputs are taken as finite.
 *
 * pgcn_rank_queries is an opaque query set built from host arrays: anchors, targets and optionally
 * per query e a list F_e = filter_idx[filter_ptr[e] .. filter_ptr[e + 1]) of candidates to leave
 * out.  Creation validates on the host, before a device is looked for -- PGCN_E_INVALID for an
 * endpoint outside [0, n_nodes), a list that is not strictly ascending (so deduplicated) or has
 * an entry out of range, a list holding its query's target, n_queries beyond an int.  The handle
 * owns the thresholds r(a_e, t_e) a call writes: pgcn_link_rank allocates nothing (it can be
 * captured), and two calls on one handle must not overlap.
 *
 * pgcn_link_rank_scores: scores[e] = r(src_e, dst_e) of m explicit pairs (src, dst: device
 * arrays), a lane per pair with an fmaf loop: the definition itself.
 * pgcn_link_rank: for every query e (greater, equal: device, [n_queries])
 *     greater[e] = #{ v in [0, n) : v != t_e, v not in F_e, r(a_e, v) >  r(a_e, t_e) }
 *     equal[e]   = #{ v in [0, n) : v != t_e, v not in F_e, r(a_e, v) == r(a_e, t_e) }
 * so the optimistic rank is greater + 1 and the pessimistic one greater + equal + 1.  At most
 * three launches: the thresholds (which also zero the counts), the sweep -- workgroups of
 * pgcn_link_rank_tile's queries_per_block queries over candidates_per_tile-candidate tiles of H on
 * the f32 MFMA, a grid of query blocks x candidate splits, the splits a function of (n_queries, n)
 * only, counts added with unsigned integer atomics -- and with lists the filter correction (a wave
 * per query).  Asynchronous, no float atomics; integer sums do not depend on their order, so two
 * calls give the same bits.  1 <= d <= 128, ld_h a multiple of 4 and >= d, H 16-byte aligned:
 * anything else is PGCN_E_INVALID before the device is touched; n_queries == 0 launches nothing.
 * pgcn_debug_rank_filter: host-only, the query set pgcn_gcn_link_ranks builds (see there) from a
 * CSR pattern and a pair list: returns the query count (or a status < 0), *n_filter = the filter
 * entries; anchor, target [queries], ptr [queries + 1], idx [*n_filter] are optional: call once for
 * the sizes, then again for the data. */
typedef struct pgcn_rank_queries pgcn_rank_queries;
int pgcn_rank_queries_create(int n_nodes, long long n_queries, const int *anchor, const int *target,
                             const long long *filter_ptr /* [n_queries + 1] or NULL */,
                             const int *filter_idx, pgcn_rank_queries **out);
int pgcn_rank_queries_destroy(pgcn_rank_queries *q);
void pgcn_link_rank_tile(int *queries_per_block, int *candidates_per_tile);
int pgcn_link_rank_scores(const int *src, const int *dst, long long m, const float *H, int ld_h,
                          int d, float *scores /* [m] */, void *stream);
int pgcn_link_rank(const pgcn_rank_queries *q, const float *H, int ld_h, int d,
                   unsigned int *greater, unsigned int *equal, void *stream);
long long pgcn_debug_rank_filter(int n_nodes, const int *indptr, const int *indices,
                                 long long n_pairs, const int *pair_src, const int *pair_dst,
                                 const int *pair_label, const int *pair_split, int split, int side,
                                 int filtered, long long *n_filter, int *anchor, int *target,
                                 long long *ptr, int *idx);

/* --- link prediction: 1-vs-all top-K retrieval (k_topk.hip; new: the reference has no pair-level
 * model).  "For this node, which nodes should it be linked to?": per query the k best candidates
 * by the rank score, never forming the [n_queries][n] score matrix.
 *
 * Score.  r(a, v) is the rank score above, unchanged: the fused chain over columns 0 .. d - 1,
 * columns >= d never read from memory.
 * Candidates of query e with anchor a_e: every v in [0, n) that is not in the query's exclude list
 * X_e = exclude_idx[exclude_ptr[e] .. exclude_ptr[e + 1]).  There is no target.
 * Order.  Candidate v precedes candidate w when r(a, v) > r(a, w), or when r(a, v) == r(a, w) and
 * v < w, by float comparison, so -0.0 == +0.0 (a chain may end in a zero of either sign; it is
 * canonicalised before any selection key is formed).  This is a total order on candidates, so the
 * answer is unique:
 *     idx[e][j], score[e][j], j < k: the j-th candidate in that order and its score;
 *     the positions from min(k, candidates) on hold idx = -1 and score = -inf.
 * Limits: 1 <= k <= 128 (pgcn_link_topk_tile's k_max, which covers Hits@100), 1 <= d <= 128, ld_h a
 * multiple of 4 and >= d, H 16-byte aligned, inputs finite.
 *
 * pgcn_topk_queries is an opaque query set built from host arrays.  Creation validates on the host,
 * before a device is looked for -- PGCN_E_INVALID for an anchor or a list entry outside
 * [0, n_nodes), a list that is not strictly ascending, k outside [1, 128], n_queries beyond an int.
 * A list may hold the anchor; nothing else about the lists is assumed.  The handle owns every byte
 * of workspace a call needs, pgcn_topk_queries_workspace =
 *     n_queries * pgcn_link_topk_splits(n_queries, n_nodes) * cap(k) * 8 bytes,
 *     cap(k) = 128 for k <= 64 and 256 above
 * (per query and candidate split an append buffer of cap 64-bit keys), so pgcn_link_topk allocates
 * nothing and can be captured; two calls on one handle must not overlap.
 *
 * pgcn_link_topk (idx, score: device, [n_queries][k]): exactly TWO launches whatever (n_queries, n,
 * k) and the data are, none when n_queries == 0 --
 *   the sweep: k_rank.hip's workgroups (pgcn_link_topk_tile's queries_per_block queries over
 *     candidates_per_tile-candidate tiles on the f32 MFMA), a grid of query blocks x
 *     pgcn_link_topk_splits -- a function of (n_queries, n_nodes) only, and the function the
 *     launcher uses -- whose epilogue selects: per query a threshold that only rises, an append
 *     buffer pruned to its k best whenever it could overflow; it leaves k keys per (query, split);
 *   the merge: a wave per query takes the k best of its splits' keys and writes idx and score
 *     with the padding.
 * No atomics and no data-dependent order: two calls on equal inputs give the same bits.  Argument
 * errors are PGCN_E_INVALID before the device is touched.
 * pgcn_link_topk_chunk: the queries pgcn_gcn_top_links hands to one pgcn_link_topk call.
 * pgcn_debug_topk_filter: host-only, the exclude lists pgcn_gcn_top_links builds for m anchor
 * nodes (see there) from a CSR pattern and a pair list: returns m (or a status < 0), *n_exclude =
 * the entries; ptr [m + 1] and idx [*n_exclude] are optional: call once for the sizes, then again
 * for the data. */
typedef struct pgcn_topk_queries pgcn_topk_queries;
int pgcn_topk_queries_create(int n_nodes, long long n_queries, const int *anchor,
                             const long long *exclude_ptr /* [n_queries + 1] or NULL */,
                             const int *exclude_idx, int k, pgcn_topk_queries **out);
int pgcn_topk_queries_destroy(pgcn_topk_queries *q);
long long pgcn_topk_queries_workspace(const pgcn_topk_queries *q); /* device bytes it owns */
void pgcn_link_topk_tile(int *queries_per_block, int *candidates_per_tile, int *k_max);
int pgcn_link_topk_splits(long long n_queries, int n_nodes); /* host only, pure */
int pgcn_link_topk_chunk(void);
int pgcn_link_topk(const pgcn_topk_queries *q, const float *H, int ld_h, int d,
                   int *idx /* dev [n_queries][k] */, float *score /* dev [n_queries][k] */,
                   void *stream);
long long pgcn_debug_topk_filter(int n_nodes, const int *indptr, const int *indices,
                                 long long n_pairs, const int *pair_src, const int *pair_dst,
                                 const int *pair_label, const int *pair_split, long long m,
                                 const int *nodes, int side, int filtered, long long *n_exclude,
                                 long long *ptr, int *idx);

/* --- cross entropy + accuracy (src/module.cu:484-541, src/gcn.cu:264-289) -------------- */
/* Rows with truth >= 0: logits max-shifted in place; if training grad = (softmax - 1[t])
 * / count, zero elsewhere.  Writes per-block partial sums (loss, wrong) to `partials`
 * (>= 2*pgcn_xent_blocks(n) floats); pgcn_finalize reduces them. */
int pgcn_xent_blocks(int n);
int pgcn_xent_fwd(float *logits, int ld, float *grad, const int *truth, int n, int c,
                  int count, int training, float *partials, void *stream);
/* out4[0] = loss/count + wd*sum(w^2)/2, out4[1] = (count-wrong)/count   (device) */
int pgcn_finalize(const float *partials, int n_blocks, int count, const float *w_l2,
                  long long n_l2, float weight_decay, float *out4, void *stream);

/* --- per-row prediction and confusion matrix (new: the reference keeps nothing per node) - */
/* cls[i] = lowest index of the row's maximum over columns [0,c); conf[i] = its softmax
 * probability; probs (may be NULL) [n][ld_probs] = the whole softmax row (columns
 * [c, round_up4(c)) are written as zero, further padding is left alone).  The softmax is
 * made of pgcn_xent_fwd's pieces (max shift, exp, summation order, rounded quotient) with the
 * shift's rounding corrected: within (c + 3) 2^-24 relative of the exact one.  Columns >= c of logits are never read into the result (they
 * may hold anything, NaN included).  logits is not modified.  1 <= c <= 128, ld and ld_probs
 * multiples of 4 and >= c.  cls/conf may be NULL.  PGCN_PREDICT_ROWS rows per workgroup. */
#define PGCN_PREDICT_ROWS 64
int pgcn_predict_rows(const float *logits, int ld, int n, int c, int *cls, float *conf,
                      float *probs, int ld_probs, void *stream);
/* counts[t*c + p] = rows with truth[i] == t >= 0 and cls[i] == p (truth < 0: skipped, the
 * pgcn_xent_fwd convention; labels or classes outside [0,c) are skipped too).  The call zeroes
 * counts first.  Integer adds only: the result does not depend on the order. */
int pgcn_confusion(const int *cls, const int *truth, int n, int c, unsigned int *counts,
                   void *stream);

/* --- multi-label classification (new: the reference has one class per node) ---------------
 * Labels are a bit matrix label_bits [n][words] of uint32_t, words = ceil(c / 32), bit j % 32 of
 * word j / 32 set iff row i has class j; 1 <= c <= 128.  Rows with truth >= 0 are labelled.
 * pgcn_bce_fwd: pgcn_xent_fwd's contract for the per-class sigmoid with binary cross-entropy.
 * With x the logits and y the target bits of the labelled rows, columns < c:
 *   partials[2 b]     = sum over block b's rows of max(x, 0) - x y + log1p(exp(-|x|))
 *   partials[2 b + 1] = #{(x > 0) != y}                     (pgcn_xent_blocks(n) blocks)
 *   training: grad [n][ld] = (sigmoid(x) - y) / count, zero on unlabelled rows and in columns
 *   [c, ld); !training: grad is not touched (may be NULL).
 * pgcn_finalize then gives loss / count and the Hamming accuracy (count - wrong) / count for
 * count = labelled rows * c.  logits is never written; its columns [c, ld) are never read into
 * the result.  No float atomics, a fixed summation order: two calls give the same bits.
 * PGCN_E_INVALID (before anything touches the device) for c outside [1, 128], ld < c or ld % 4,
 * words != ceil(c / 32), count < 1; n == 0 launches nothing.  Asynchronous, allocates nothing,
 * capturable. */
int pgcn_bce_fwd(const float *logits, int ld, float *grad, const int *truth,
                 const uint32_t *label_bits, int words, int n, int c, int count, int training,
                 float *partials, void *stream);
/* bits [n][words]: bit j of word w set iff logits[i][32 w + j] > 0 (strict, the project's tie
 * rule), bits from c on zero.  probs (may be NULL) [n][ld_probs]: the sigmoid row, columns
 * [c, round_up4(c)) zero, further padding left alone.  Same argument rules as pgcn_bce_fwd. */
int pgcn_predict_multilabel_rows(const float *logits, int ld, int n, int c, uint32_t *bits,
                                 int words, float *probs, int ld_probs, void *stream);
/* counts [3][c] = per class tp, fp, fn over the rows with truth >= 0.  The call zeroes counts
 * first.  Integer adds only, as pgcn_confusion. */
int pgcn_multilabel_counts(const uint32_t *pred_bits, const uint32_t *label_bits,
                           const int *truth, int n, int c, int words, unsigned int *counts,
                           void *stream);

/* --- Adam (src/optim.cu:42-95; hpdga optim.cpp:23-35) ---------------------------------- */
int pgcn_adam(float *w, const float *g, float *m, float *v, long long n, float step_size,
              float beta1, float beta2, float eps, float weight_decay, int decay, void *stream);
/* host: lr*sqrtf(1-powf(b2,t))/(1-powf(b1,t)) exactly as hpdga optim.cpp:24 */
float pgcn_adam_step_size(float lr, float beta1, float beta2, int t);

/* ===================================================================================== */
/* (2) Engine ABI                                                                          */
/* ===================================================================================== */

#define PGCN_MAX_LAYERS 16

/* GCNParams + AdamParams (include/gcn.cuh:40-47, include/optim.cuh:16-19) */
typedef struct {
  int num_nodes, input_dim, output_dim; /* filled by the loader */
  int n_layers;                          /* >= 2 */
  /* Link prediction.  0: none (the engine as it was, bit for bit); 1: dot product.  The output
   * layer's node variable out [N][D], D = output_dim <= 128, is an EMBEDDING; behind it a
   * LinkDecoder (pgcn_link_score_fwd / _bwd) scores the pgcn_data.num_pairs pairs (required then)
   * into scores [E][4], and the sigmoid binary cross-entropy (pgcn_bce_fwd with one class) runs on
   * the scores with bit 0 = pair_label == 1, the truth of a split built from pair_label /
   * pair_split and count = the split's labelled pairs.  Loss, accuracy ((score > 0) == label), the
   * results ring and early stopping are then per pair.  The backward's pair index holds the
   * TRAINING split's labelled pairs.  Every layer family runs unchanged (attention with heads,
   * aggregator / root_weight, residual, layer_norm).  Every node row carries gradient, so the
   * fused output / loss kernel, the output-row restriction with its compact buffers, the
   * column-subset backward and the reassociated output layer are off.  The decoder draws nothing
   * from the dropout stream and has no weights.  The message-passing adjacency is the dataset's
   * graph as loaded: keeping validation and test positives out of it is the caller's job.  Not
   * with multilabel or readout, single GPU only (the edge-cut creators return PGCN_E_INVALID); a
   * split whose labelled pairs exceed 2^24 is refused (the sums travel as floats).  The engine has
   * one more variable, the last (index pgcn_gcn_num_vars - 1): scores [E][1]. */
  int link_decoder;
  int hidden_dims[PGCN_MAX_LAYERS];      /* n_layers - 1 */
  float dropouts[PGCN_MAX_LAYERS];       /* n_layers */
  /* GraphSAGE layers.  aggregator: 0 = GCN's Â (the engine as it was, bit for bit), 1 = mean,
   * 2 = max; root_weight: 0 / 1, 1 only with aggregator != 0.  With H the layer's input as it
   * reads it (after its Dropout in training) and d_l its output width:
   *   root_weight 1: W_l is [d_in][2 d_l]; P = H W_l; R = P[:, 0:d_l], Q = P[:, d_l:2 d_l]
   *   root_weight 0: W_l is [d_in][d_l] as before; Q = H W_l, R absent
   *   mean: Z_i = R_i + (1 / len_i) sum over row i's slots of Q_j   (pgcn_graph_create_mean)
   *   max:  Z_i[c] = R_i[c] + max over row i's slots of Q_j[c]      (pgcn_agg_max_fwd)
   * on the adjacency pattern as loaded -- directed patterns included, len_i the CSR row length
   * with the self loop and duplicated edges as the pattern has them; the Â coefficients are not
   * used.  A row without a slot gives Z_i = R_i (or 0).  Behind Z a hidden layer goes on as
   * before ([LayerNorm] -> ReLU -> [Residual] -> Dropout) and the output layer is Z itself.  The
   * wider weight is drawn like any weight of its shape (Glorot with fan-out 2 d_l, one draw per
   * element, the dropout streams after the last draw); variable var1 of a layer is then
   * [rows][2 d_l], root half first.  No reassociated output layer, no Â X precompute, no
   * output-row restriction, the loss unfused.  Hidden widths and output_dim up to 128; not with
   * attention; single GPU only (the edge-cut creators return PGCN_E_INVALID: the mean could be
   * partitioned, the max needs a max / arg exchange). */
  int aggregator, root_weight;
  int epochs;
  /* Graph classification.  0: node-level losses (the engine as it was, bit for bit); 1 = sum,
   * 2 = mean, 3 = max: the nodes are a batch of pgcn_data.num_graphs graphs (contiguous row ranges
   * pgcn_data.graph_ptr, required then), and behind the output layer's node logits out [N][C] a
   * Readout (pgcn_readout_fwd) writes pooled [G][C]; the softmax cross-entropy runs on pooled
   * with the truth of a split built from graph_label / graph_split and count = the split's
   * labelled graphs.  Loss, accuracy, the results ring, early stopping, pgcn_gcn_predict (G rows)
   * and pgcn_gcn_confusion are then per graph.  Every layer family runs unchanged on the batch
   * (attention with heads, aggregator / root_weight, residual, layer_norm).  Every node row
   * carries gradient, so whatever relies on only a split's labelled rows mattering is off: the
   * fused output / loss kernel, the output-row restriction with its compact buffers, the
   * column-subset backward and the reassociated output layer.  The readout draws nothing from the
   * dropout stream.  Not with multilabel, single GPU only (the edge-cut creators return
   * PGCN_E_INVALID). */
  int readout;
  int early_stopping;
  /* attention != 0 only (anything but 1 / 0 without it is PGCN_E_INVALID).  attention_heads = K
   * (0 counts as 1): every HIDDEN attention layer runs K heads concatenated inside its width d_l
   * -- head h owns columns [h dh, (h + 1) dh), dh = d_l / K, reads its own slice of a_dst / a_src
   * and takes a softmax of its own (pgcn_gat_fwd_mh); no tensor changes shape.  K must divide
   * every hidden width into dh of 4, 8, 16, 32, 64 or 128.  The output layer stays single-head.
   * attention_dropout = p in [0, 1): in training, every attention layer (the output layer too)
   * drops each normalised weight alpha_s^h with probability p and scales the kept ones by
   * 1 / (1 - p) (kept iff draw >= int(p * RAND_MAX), the product in float, as every mask here).
   * The draws come from the engine's xorshift stream: inside an epoch's block of draws they stand
   * behind every existing Dropout's, layer by layer, nnz * K_l each (K_l = 1 on the output
   * layer), element s * K_l + h for slot s (CSR order), head h -- so the other masks keep their
   * offsets inside the epoch and only the period grows.  p == 0 draws nothing: heads 1 with p 0
   * is the single-head attention engine bit for bit. */
  int attention_heads;
  float attention_dropout;
  float learning_rate, weight_decay, beta1, beta2, eps;
  /* != 0: graph attention layers -- every layer's GraphSum is replaced by a single-head additive
   * attention over the node's neighbours (pgcn_gat_fwd, LeakyReLU slope 0.2) on the adjacency
   * pattern as loaded, directed patterns included; the Â coefficients are not used.  Hidden layers
   * go on as before ([LayerNorm] -> ReLU -> [Residual] -> Dropout); the output layer is Z itself.
   * The attention vectors, per layer a_dst[d_l] then a_src[d_l], are one more trainable tensor
   * (Glorot-uniform, limit sqrt(6 / (d_l + 1)) per vector, drawn after the last layer weight: the
   * dropout streams start after those draws; Adam without weight decay).  No reassociated output
   * layer, no Â X precompute, no output-row restriction, the loss unfused.  Hidden widths and
   * output_dim up to 128; single GPU only (the edge-cut creators return PGCN_E_INVALID: a row's
   * softmax needs all its columns).  0: the GCN engine, bit for bit. */
  int attention;
  /* 1: compute the output layer as (Â H) W instead of Â (H W) when hidden < classes, so its
   * GraphSum gathers hidden-width rows.  Exact algebra when Â is symmetric (checked at engine
   * build: a non-symmetric pattern keeps the reference's order); only the fp32 rounding order
   * differs from the reference.  0: the reference's module order. */
  int reassociate_last;
  /* != 0: multi-label node classification -- a node carries any subset of the output_dim <= 128
   * classes (pgcn_data.label_bits, required then), the loss is the per-class sigmoid with binary
   * cross-entropy, mean over (labelled rows of the split) x classes (pgcn_bce_fwd), and the
   * accuracy column is the Hamming accuracy.  The output layer's Matmul runs unfused.  Engine
   * build refuses (PGCN_E_INVALID) data where the labelled rows of any split x classes exceed
   * 2^24: the loss / wrong sums and their count travel as floats.  0: the single-label engine,
   * bit for bit. */
  int multilabel;
  /* PART2 `seed` (src/parser.cpp:234): 0 = hpdga's unseeded glibc rand() (init_rand_state,
   * hpdga rand.cpp:6-14); else the xorshift state is the first two rand() values after
   * srand(seed).  Glorot init and every dropout mask follow from it. */
  unsigned int seed;
  /* != 0: every hidden layer 0 <= l <= n_layers - 2 gets a LayerNorm between its
   * GraphSum and its ReLU: H_l = relu(gamma_l * xhat + beta_l) [+ A], xhat the row-normalised
   * Â (A W_l) (pgcn_layernorm_fwd, eps 1e-5).  gamma = 1 and beta = 0 at the start (no RNG
   * draw: weights and dropout masks equal the plain engine's); Adam updates them without weight
   * decay.  Hidden widths up to 1024.  0: the plain engine, bit for bit. */
  int layer_norm;
  /* (the struct's last member) != 0: every middle layer 1 <= l <= n_layers - 2 whose width equals the layer before it
   * (hidden_dims[l] == hidden_dims[l-1]) gets the reference's ResidualConnection after its ReLU
   * (include/module.cuh:149-161): H_l = relu(Â (A W_l)) + A, with A the layer's input as it
   * read it (in training, after that layer's Dropout), and a real backward (the reference's is
   * empty).  No projection for unequal widths; none qualifying (n_layers == 2): the plain
   * engine, bit for bit. */
  int residual;
} pgcn_params;

/* hpdga defaults: 2 layers, hidden 16, dropout .5/.5, 100 epochs, Adam lr .01, wd 5e-4,
 * reassociate_last = 1 */
void pgcn_params_default(pgcn_params *p);

/* GCNData in host memory (include/gcn.cuh:51-58): CSRs as the hpdga Parser builds them. */
typedef struct {
  int num_nodes;
  const int *graph_indptr, *graph_indices;            /* n+1, nnz */
  const int *feat_indptr, *feat_indices;              /* n+1, nnz_x */
  const float *feat_values;                           /* nnz_x */
  const int *label, *split;                           /* n, n */
  /* read only when pgcn_params.link_decoder != 0: num_pairs >= 1 node pairs (pair_src[e],
   * pair_dst[e]) in [0, num_nodes), pair_label [num_pairs] 1 (a link), 0 (none) or -1
   * (unlabelled), pair_split [num_pairs] in 0..3 as the node splits.  Self pairs and repeated
   * pairs are allowed.  0 / NULL: none. */
  int num_pairs;
  const int *pair_src, *pair_dst, *pair_label, *pair_split;
  /* read only when pgcn_params.multilabel != 0: the label bit matrix [n][label_words], bit j % 32
   * of word j / 32 set iff node i has class j, bits from output_dim on zero; label_words =
   * ceil(output_dim / 32).  A node is labelled iff label[i] >= 0 (the value is not used). */
  const uint32_t *label_bits;
  int label_words;
  /* read only when pgcn_params.readout != 0: the nodes are num_graphs >= 1 graphs, graph g owning
   * rows [graph_ptr[g], graph_ptr[g + 1]) (graph_ptr [num_graphs + 1], non-decreasing, from 0 to
   * num_nodes); graph_label [num_graphs] in [0, output_dim) or -1 (unlabelled), graph_split
   * [num_graphs] in 0..3 as the node splits.  0 / NULL: none. */
  int num_graphs;
  const int *graph_ptr, *graph_label, *graph_split;
} pgcn_data;

typedef struct pgcn_gcn pgcn_gcn;

/* GCN::GCN (include/gcn.cuh:79) on HIP device `device`. */
int pgcn_gcn_create(const pgcn_params *p, const pgcn_data *d, int device, pgcn_gcn **out);
/* Edge-cut variant: this process is rank `rank` of `world` (one process per GPU); the
 * graph is partitioned into contiguous nnz-balanced node ranges; GraphSum partials are
 * combined with RCCL reduce-scatter, weight grads and scalars with all-reduce.
 * `unique_id` = 128 bytes from pgcn_comm_unique_id on rank 0, shared by the caller. */
int pgcn_comm_unique_id(void *unique_id_128);
int pgcn_gcn_create_dist(const pgcn_params *p, const pgcn_data *d, int device, int rank,
                         int world, const void *unique_id_128, pgcn_gcn **out);
/* Edge-cut variant over peer-mapped memory instead of RCCL (one process per GPU, DESIGN.md
 * §6): every rank's receive slots are mapped into every other rank with hipIpc handles, and a
 * GraphSum's partial sums travel as one-sided stores over xGMI straight from the kernel that
 * forms them into their owner's slot, summed there in rank order (deterministic).  `allgather`
 * is the caller's host channel (MPI_Allgather, torch.distributed, ...): the engine calls it
 * with every rank in the same order -- at creation (the handles; all ranks fail together with
 * PGCN_E_COMM if any cannot map its peers) and at destruction (a barrier before the regions are
 * unmapped and freed) -- and it must fill all[q * bytes, (q + 1) * bytes) with rank q's `mine`
 * and return 0.  A peer that never signals fails the next sync with PGCN_E_COMM after 20 s. */
typedef int (*pgcn_allgather_fn)(const void *mine, size_t bytes, void *all, void *user);
int pgcn_gcn_create_peer(const pgcn_params *p, const pgcn_data *d, int device, int rank,
                         int world, pgcn_allgather_fn allgather, void *user, pgcn_gcn **out);
/* In-process ranks ("fake RCCL"): `world` edge-cut engines in ONE process on
 * one device, each created and driven by its own host thread (creation and destruction
 * rendezvous with the peers' same call).  Their collectives are pgcn_gcn_create_peer's
 * kernels over raw device pointers (the same pushes, flags and rank-order sums), so the
 * multi-rank engine (partition, peer exchange, global dropout offsets, weight all-reduce)
 * runs unchanged without RCCL.  The group may be destroyed after the engines are created
 * (they keep it alive). */
typedef struct pgcn_loopback pgcn_loopback;
int pgcn_loopback_create(int world, pgcn_loopback **out);
int pgcn_loopback_destroy(pgcn_loopback *group);
int pgcn_gcn_create_loopback(const pgcn_params *p, const pgcn_data *d, int device, int rank,
                             pgcn_loopback *group, pgcn_gcn **out);
/* Diagnostics (timing only, tools/rank_epoch.py): rank `rank` of a `world`-rank edge-cut
 * engine with no peers -- its kernels and stream order, collectives reduced to this rank's
 * share ("comm" 3).  Its results are not the model's. */
int pgcn_debug_gcn_create_solo(const pgcn_params *p, const pgcn_data *d, int device, int rank,
                               int world, pgcn_gcn **out);
int pgcn_gcn_destroy(pgcn_gcn *g);
/* Engine facts: "world", "rank", "comm" (0 none, 1 RCCL, 2 loopback, 3 solo, 4 peer), "comm_calls" /
 * "comm_bytes" (collectives enqueued since creation and the bytes this rank sends in them,
 * ring algorithm: a reduce-scatter (W-1)/W of its send buffer, an all-reduce twice that), "reassociated",
 * "graph_symmetric", "graphsum_lds" (width-16 GraphSums take the LDS kernel), "epochs",
 * "adam_steps" (optimizer steps taken; 0 again after a weights-only load),
 * "eval_ax_us" (device time of the Â X precompute at engine build, µs; 0 when not used),
 * "residual_layers" (layers with a ResidualConnection, pgcn_params.residual) and
 * "fused_residuals" (how many of them the last training forward added inside a GraphSum's
 * final write instead of a launch of their own), "norm_layers" (layers with a LayerNorm,
 * pgcn_params.layer_norm), "multilabel" (1: a multi-label engine, pgcn_params.multilabel), "readout" (the readout
 * mode, pgcn_params.readout) and "num_graphs" (its graph count; 0 without a readout),
 * "link_decoder" (pgcn_params.link_decoder) and "num_pairs" (its pair count; 0 without), and
 * "fused_norm_tails" (how many of them ran the ReLU / residual add /
 * Dropout behind them inside the LayerNorm kernel in the last training forward);
 * "norm_padding_nonzero" (diagnostics, syncs: non-zero elements in the edge-cut padding rows of
 * the normalised variables -- always 0); "attention_layers" (layers whose aggregation is graph
 * attention, pgcn_params.attention: n_layers or 0; on such an engine "reassociated", "eval_ax_us"
 * and "graphsum_lds" are 0); "attention_heads" (the heads of its hidden attention layers,
 * pgcn_params.attention_heads; 1 without attention) and "attention_dropout_layers" (layers that
 * drop attention weights in training: n_layers with attention_dropout > 0, else 0); "knob.<key>" (the value of that pgcn_debug_set key the engine was
 * built with).
 * Returns the value (>= 0) or PGCN_E_INVALID for an unknown key. */
long long pgcn_gcn_query(pgcn_gcn *g, const char *key);
/* GCN::train_epoch / GCN::eval (src/gcn.cu:293-343): out2 = {loss, accuracy} */
int pgcn_gcn_train_epoch(pgcn_gcn *g, float out2[2]);
int pgcn_gcn_eval(pgcn_gcn *g, int split, float out2[2]);
/* One "epoch" as the reference times it (train_epoch + eval(2)) without a host sync;
 * results land in an on-device ring read by pgcn_gcn_results. */
int pgcn_gcn_epoch_async(pgcn_gcn *g);
int pgcn_gcn_sync(pgcn_gcn *g);
/* copies the last min(n, epochs run, 1024) epoch results {train_loss, train_acc, val_loss,
 * val_acc}, oldest first; returns the number of rows copied (>= 0) or a status (< 0) */
int pgcn_gcn_results(pgcn_gcn *g, int n, float *host_out);
/* GCN::run (src/gcn.cu:347-436): prints the reference's epoch lines when verbose */
int pgcn_gcn_run(pgcn_gcn *g, int verbose);
/* Variables in reference order (input, then per layer var1, weight, var2; see
 * include/gcn.cuh:85). which: 0 data, 1 grad. Returns element count (>= 0) or status. For
 * the edge-cut engine node-sized variables cover this rank's rows only.  PGCN_E_INVALID for
 * the output layer's node variables after a forward with the diagnostic row restriction
 * ("split_rows" on): their rows outside the split are stale.
 * Residual layers (pgcn_params.residual): var2 of layer l holds relu(Z_l) + A_{l-1}, and its
 * grad (which = 1) is G = dLoss/dH_l, the gradient of that sum after the next layer's Dropout
 * backward, NOT masked by the layer's ReLU: the masked gradient G * [Z_l > 0] that the
 * GraphSum backward reads is kept in a buffer of the engine's own, so that G can be added to
 * the grad of var2 of layer l-1 when the layer's Matmul backward writes it.
 * LayerNorm engines (pgcn_params.layer_norm) have one more variable, index 3 * n_layers + 1: the
 * scale / shift tensor, per hidden layer gamma_l[d_l] then beta_l[d_l], layers in order (which =
 * 1: its gradient); pgcn_gcn_num_vars is 3 * n_layers + 2 for them.  pgcn_gcn_set_var accepts
 * it.  The LayerNorm backward transforms in place the buffer the layer's GraphSum backward
 * reads: after a training epoch the grad of var2 of such a layer is dLoss/dZ, the gradient with
 * respect to the GraphSum's output (on a residual layer that buffer is the engine's own masked
 * one, and var2's grad stays G as above).
 * Attention engines (pgcn_params.attention) have one more variable behind all others, index
 * pgcn_gcn_num_vars - 1 (3 * n_layers + 1, or 3 * n_layers + 2 with LayerNorm): the attention
 * tensor, per layer a_dst[d_l] then a_src[d_l], layers in order (which = 1: its gradient).
 * pgcn_gcn_set_var accepts it. */
long long pgcn_gcn_get_var(pgcn_gcn *g, int idx, int which, float *host_dst);
int pgcn_gcn_num_vars(pgcn_gcn *g);
/* Weights only (idx must be a weight variable, which == 0), in get_var's layout and count;
 * anything else PGCN_E_INVALID.  Invalidates every product computed ahead from the old
 * weights.  Edge-cut: the caller sets the same values on every rank. */
int pgcn_gcn_set_var(pgcn_gcn *g, int idx, int which, const float *host_src, long long count);
/* Whole training state to one file: weights, Adam m/v and step count, epoch count, dropout
 * stream position, the results history that pgcn_gcn_results would return, and what
 * identifies the model (layer dims, num_nodes, seed, dropouts).  Syncs first.  Written to
 * path + ".tmp" and renamed.  Every rank of an edge-cut engine writes the same bytes; one of
 * them saving is enough.  Format: INTEGRATION.md. */
int pgcn_gcn_save(pgcn_gcn *g, const char *path);
#define PGCN_LOAD_WEIGHTS_ONLY 1
/* flags 0: resume -- after it the engine continues exactly as the engine that saved would
 * have (same masks, same Adam steps, same results rows), whether `g` is fresh or has trained
 * past or short of the save point, on one GPU or as edge-cut ranks (every rank loads).
 * PGCN_LOAD_WEIGHTS_ONLY: weights from the file, Adam m/v and step count reset to zero, epoch
 * count, results and dropout position kept.
 * PGCN_E_INVALID: the file is for another model (dims, num_nodes; for flags 0 also seed,
 * dropouts and whether the model is residual -- a weights-only load ignores that flag, the
 * tensors having the same shapes, so a plain model's weights can warm-start a residual one;
 * for flags 0 also whether the model has LayerNorm -- a weights-only load crosses that too: from
 * a file without the scale / shift tensor the engine's gamma / beta keep their values, from a
 * file with it a plain engine ignores it).  PGCN_E_IO: missing, truncated, corrupted or unknown version.  On any error
 * the engine is untouched. */
int pgcn_gcn_load(pgcn_gcn *g, const char *path, int flags);
/* Host-only look at a checkpoint file (no device, no engine): validates it as pgcn_gcn_load
 * does and fills info[8] = {version, n_layers, num_nodes, input_dim, output_dim, adam_steps,
 * epochs, weight count}.  PGCN_E_IO as pgcn_gcn_load. */
int pgcn_checkpoint_info(const char *path, long long info[8]);
/* Host-only: the file's header flags (>= 0; bit 0: saved by a residual engine; bit 1: by a
 * LayerNorm engine; bit 2: by a multi-label engine; bit 3: by an attention engine), validated as
 * pgcn_checkpoint_info does, or a status < 0 (PGCN_E_IO also for flag bits this library does
 * not know). */
int pgcn_checkpoint_flags(const char *path);
#define PGCN_CKPT_RESIDUAL 1
/* bit 1: saved by a LayerNorm engine -- a version-2 file, whose weight count and w / m / v
 * payloads include the scale / shift tensor after the layer weights (version-1 files never
 * carry it: there the bit is unknown) */
#define PGCN_CKPT_LAYERNORM 2
/* bit 2: saved by a multi-label engine (pgcn_params.multilabel).  No payload or version change;
 * a flags-0 load refuses a file whose bit differs from the engine's, a weights-only load
 * crosses it.  (In a version-2 file the bit stays unknown, as it was before it had a meaning: a
 * multi-label engine with LayerNorm writes version 3, version 2's layout with bits 1 and 2.) */
#define PGCN_CKPT_MULTILABEL 4
/* bit 3: saved by an attention engine (pgcn_params.attention) -- a version-4 file: the existing
 * layout, the weight count and the w / m / v payloads carrying the attention tensor last (after
 * the scale / shift tensor when bit 1 is set); bits 0-3 are all known there.  In files of
 * versions 1-3 the bit stays unknown.  A flags-0 load refuses a file whose bit differs from the
 * engine's; a weights-only load crosses it as it crosses bit 1 (a file without the tensor leaves
 * the engine's alone, a plain engine ignores a file's). */
#define PGCN_CKPT_ATTENTION 8
/* Host-only: the heads and the attention dropout of the engine that saved the file.  An attention
 * engine with attention_heads > 1 or attention_dropout > 0 writes a version-5 file: the
 * version-4 header and flags (bit 3 set), then 16 bytes {u32 heads; f32 attention_dropout; u64 0}
 * between the header and the payload, under the checksum; the payload is version 4's (no tensor
 * changes shape).  Files of versions 1-4 give 1 and 0.  A flags-0 load refuses a file whose heads
 * or dropout differ from the engine's -- a version-4 file into such an engine and the reverse
 * included; a weights-only load crosses it.  pgcn_checkpoint_info and pgcn_checkpoint_flags
 * accept version 5.  Validates as pgcn_checkpoint_info does. */
int pgcn_checkpoint_attention(const char *path, int *heads, float *dropout);
/* flags bit 4: saved by a GraphSAGE engine (pgcn_params.aggregator != 0).  Such an engine writes
 * a version-6 file: the header with bit 4 set (bits 0-2 known, bit 3 never: no attention), then
 * 16 bytes {u32 aggregator; u32 root_weight; u64 0} where version 5 has its block, under the
 * checksum, then the payload.  With root_weight 1 every layer weight is [d_in][2 d_l], so
 * n_weights and the w / m / v tensors are that much longer; the scale / shift tensor follows as in
 * version 2.  Every other engine keeps writing versions 1-5 byte for byte.
 * pgcn_checkpoint_sage is host-only and validates as pgcn_checkpoint_info does: the aggregator
 * and the root weight of the engine that saved the file; versions 1-5 give 0 and 0.  A flags-0
 * load refuses a file whose aggregator or root weight differs from the engine's; a weights-only
 * load crosses the aggregator whenever the tensor shapes agree (the same root_weight) and refuses
 * otherwise.  pgcn_checkpoint_info and pgcn_checkpoint_flags accept version 6. */
#define PGCN_CKPT_SAGE 16
int pgcn_checkpoint_sage(const char *path, int *aggregator, int *root_weight);
/* flags bit 5: saved by a graph-classification engine (pgcn_params.readout != 0).  Such an engine
 * writes a version-7 file: the header with bit 5 set and bits 0-4 all known, then three 16-byte
 * blocks under the checksum -- version 5's {u32 heads; f32 attention_dropout; u64 0} (1 and 0
 * without attention), version 6's {u32 aggregator; u32 root_weight; u64 0} (0 and 0 without
 * SAGE layers) and {u32 readout; u32 num_graphs; u64 0} -- then the payload as the flags say
 * (the scale / shift tensor with bit 1, the attention tensor with bit 3, doubled layer weights
 * with root_weight).  Every other engine keeps writing versions 1-6 byte for byte.
 * pgcn_checkpoint_readout is host-only and validates as pgcn_checkpoint_info does: the readout
 * mode and the graph count of the engine that saved the file; versions 1-6 give 0 and 0.  Any
 * load (resume or weights only) refuses a file whose mode or graph count differs from the
 * engine's.  pgcn_checkpoint_info, _flags, _attention and _sage accept version 7. */
#define PGCN_CKPT_READOUT 32
int pgcn_checkpoint_readout(const char *path, int *mode, int *num_graphs);
/* flags bit 6: saved by a link-prediction engine (pgcn_params.link_decoder != 0).  Such an engine
 * writes a version-8 file: the header with bit 6 set, then version 7's three 16-byte blocks (the
 * third all zero: a link engine has no readout) and a fourth {u32 link_decoder; u32 0; u64
 * num_pairs}, all under the checksum, then the payload as the flags say -- unchanged: the decoder
 * has no weights.  Every other engine keeps writing versions 1-7 byte for byte.
 * pgcn_checkpoint_links is host-only and validates as pgcn_checkpoint_info does: the decoder and
 * the pair count of the engine that saved the file; versions 1-7 give 0 and 0.  A resuming load
 * (flags 0) refuses a file whose decoder or pair count differs from the engine's; a weights-only
 * load crosses both -- the tensors are the same, so a node-classification model can warm-start a
 * link model of equal dims, and the reverse.  pgcn_checkpoint_info, _flags, _attention, _sage and
 * _readout accept version 8. */
#define PGCN_CKPT_LINKS 64
int pgcn_checkpoint_links(const char *path, int *decoder, long long *num_pairs);
/* sizeof(pgcn_params) of this library (bindings check their struct layout against it) */
int pgcn_params_sizeof(void);
/* An eval-mode forward over every row this rank owns (no split, no row restriction whatever
 * "split_rows" says), then pgcn_predict_rows.  Host outputs, any may be NULL; probs is
 * [rows][output_dim] dense.  Returns the row count (node_range's) or a status < 0.  Leaves
 * the training state exactly as it was: no results slot written, epoch count, Adam and
 * dropout position unchanged, and training continued after it is bit-identical to training
 * without it.  Edge-cut: a collective, every rank calls it.  A readout engine (pgcn_params.readout):
 * one row per graph -- num_graphs rows of pooled logits -- and pgcn_gcn_confusion counts the
 * split's labelled graphs. */
long long pgcn_gcn_predict(pgcn_gcn *g, int *cls, float *conf, float *probs);
/* predict + pgcn_confusion against split's labels: counts[c*c], this rank's rows (the caller
 * adds the ranks' matrices, as it concatenates get_var's rows). */
int pgcn_gcn_confusion(pgcn_gcn *g, int split, long long *counts);
/* Multi-label engines (others: PGCN_E_INVALID; pgcn_gcn_confusion refuses them in turn).
 * pgcn_gcn_predict's eval-mode forward and guarantees (training state untouched, training
 * continued after it bit-identical, collective on edge-cut engines), then
 * pgcn_predict_multilabel_rows: bits [rows][ceil(output_dim / 32)], probs (may be NULL)
 * [rows][output_dim] dense.  Returns the row count or a status < 0. */
long long pgcn_gcn_predict_multilabel(pgcn_gcn *g, uint32_t *bits, float *probs);
/* ... + pgcn_multilabel_counts against split's labels: counts [3][output_dim] = tp, fp, fn per
 * class over this rank's rows (the caller adds the ranks' counts; micro / macro F1 follow from
 * the integer sums). */
int pgcn_gcn_multilabel_counts(pgcn_gcn *g, int split, long long *counts);
/* Link engines (pgcn_params.link_decoder; PGCN_E_INVALID otherwise, as pgcn_gcn_predict,
 * pgcn_gcn_confusion and the multi-label services are on a link engine).
 * pgcn_gcn_predict_links: pgcn_gcn_predict's eval-mode forward, with the same guarantees, then the
 * scores of the engine's num_pairs pairs and their sigmoids (either may be NULL); returns the pair
 * count or a status < 0.
 * pgcn_gcn_link_counts: that forward + pgcn_multilabel_counts with one class against split's
 * labelled pairs: counts[3] = tp, fp, fn (a pair is predicted a link iff its score > 0).
 * pgcn_gcn_score_pairs: the same forward, then pgcn_link_score_fwd over m caller-given candidate
 * pairs (host arrays, endpoints in [0, num_nodes)) through a temporary pair index; scores [m].
 * pgcn_gcn_link_ranks: the same forward, then pgcn_link_rank over the output embedding for split's
 * (1..3) positive pairs (pair_label == 1) in pair order; returns their number, or a status < 0.
 * greater / equal: host arrays of at least that many entries; both NULL returns the number only.
 * side 0: the anchor is src_e, the target dst_e (the destination is corrupted); side 1: the
 * anchor is dst_e, the target src_e.  filtered 0: every node but the target competes.  filtered 1:
 * F_e is the ascending, deduplicated union, minus the target, of the anchor itself, the anchor's
 * neighbours in the message-passing pattern (side 0: the j of row a's slots; side 1: the i of the
 * slots into column a) and the other endpoints of every pair with pair_label == 1, of any split,
 * that has the anchor in the anchor's role (side 0: dst_p where src_p == a; side 1: src_p where
 * dst_p == a).  The query set of a (split, side, filtered) is built on the host at its first call
 * and kept until the engine is destroyed.
 * pgcn_gcn_top_links: the same forward, then pgcn_link_topk over the output embedding for m anchor
 * nodes (host array, in [0, num_nodes), duplicates allowed); idx / score: host, [m][k]; returns m or
 * a status < 0.  side 0: the candidates are destinations for src = node; side 1: sources for dst =
 * node.  filtered 1: X_e is pgcn_gcn_link_ranks' list without its "minus the target".  The nodes
 * are processed pgcn_link_topk_chunk() = 16,384 at a time; the query set and the device outputs
 * of a chunk are freed after it, so the device memory in use is bounded whatever m is.
 * The training state is untouched. */
long long pgcn_gcn_predict_links(pgcn_gcn *g, float *scores, float *probs);
int pgcn_gcn_link_counts(pgcn_gcn *g, int split, long long *counts);
long long pgcn_gcn_link_ranks(pgcn_gcn *g, int split, int side, int filtered, long long *greater,
                              long long *equal);
long long pgcn_gcn_top_links(pgcn_gcn *g, const int *nodes, long long m, int k, int side,
                             int filtered, int *idx, float *score);
int pgcn_gcn_score_pairs(pgcn_gcn *g, const int *src, const int *dst, long long m, float *scores);
/* per-call device timing of the GraphSum kernels (enable before the timed region) */
int pgcn_gcn_profile(pgcn_gcn *g, int enable);
int pgcn_gcn_profile_read(pgcn_gcn *g, double *graphsum_ms_total, long long *graphsum_calls,
                          double *graphsum_bytes_total);
/* The same for the XW contractions on the MFMA kernels (dense X W1 / its weight gradient,
 * H W / its two gradients): summed event time, launches, 2*M*N*K flops. */
int pgcn_gcn_profile_read_mm(pgcn_gcn *g, double *ms_total, long long *calls,
                             double *flops_total);
/* this rank's node range [first, last) (edge-cut engine; whole graph otherwise) */
int pgcn_gcn_node_range(pgcn_gcn *g, int *first, int *last);

/* --- data (kept hpdga loader + synthetic inputs) ---------------------------------------- */
typedef struct pgcn_dataset pgcn_dataset;
/* Parser(GCNParams*, GCNData*, name).parse(): reads data/<name>.{graph,split,svmlight}
 * under `root` with hpdga-spring23/src/parser.cpp:6-140 semantics. */
int pgcn_dataset_load(const char *root, const char *name, pgcn_dataset **out);
/* The same load through the binary cache <root>/data/<name>.pgcnbin:
 * read when its recorded size + mtime of the three text files match, else the text is parsed
 * (identical arrays) and the cache rewritten, best effort.  *from_cache (may be NULL) = 1 on a
 * cache hit.  Errors as pgcn_dataset_load. */
int pgcn_dataset_load_cached(const char *root, const char *name, pgcn_dataset **out,
                             int *from_cache);
/* Write / read the parsed arrays as one binary file (any dataset, synthetic ones included).
 * PGCN_E_IO on a write failure or an invalid / truncated / corrupted file. */
int pgcn_dataset_save(const pgcn_dataset *ds, const char *path);
/* PART2 NO_FEATURE (src/parser.cpp:100-104): every feature value of `ds` becomes 1.0 (the
 * feature ids stay, so input_dim is unchanged). */
int pgcn_dataset_binarize(pgcn_dataset *ds);
int pgcn_dataset_load_binary(const char *path, pgcn_dataset **out);
/* Seeded reddit-shaped synthetic: n nodes, f dense features, c classes,
 * Chung-Lu power-law undirected graph with `undirected_edges` edges (2x directed slots). */
int pgcn_dataset_synthetic(int n, int f, int c, long long undirected_edges, uint64_t seed,
                           pgcn_dataset **out);
/* Multi-label data: attaches the bit matrix bits [num_nodes][words] (copied; words = ceil(c /
 * 32), 1 <= c <= 128, bits from c on must be zero) and sets output_dim = c.  label[i] of every
 * node keeps its sign: a node that was labelled stays labelled.  PGCN_E_INVALID otherwise. */
int pgcn_dataset_set_multilabel(pgcn_dataset *ds, const uint32_t *bits, int words, int c);
/* The same from the sidecar text file `path` (by convention <root>/data/<name>.labels): line i
 * holds the class ids of node i separated by spaces; an empty line is a labelled node with no
 * class.  num_classes 0: max id + 1.  Every node becomes labelled (label[i] >= 0).  PGCN_E_IO for a missing file, a line
 * count different from num_nodes, a token that is not a number, or an id outside [0,
 * min(num_classes or 128, 128)).  The .svmlight / .graph / .split parser and the .pgcnbin cache
 * are untouched: pgcn_dataset_save of a multi-label dataset returns PGCN_E_INVALID. */
int pgcn_dataset_load_labels(pgcn_dataset *ds, const char *path, int num_classes);
/* Graph-level data: attaches G graphs as contiguous row ranges (graph_ptr [G + 1] from 0 to
 * num_nodes, non-decreasing), their labels (in [0, classes) or -1: unlabelled) and splits (0..3),
 * all copied; num_classes 0: max label + 1.  Sets output_dim = the class count, as
 * pgcn_dataset_load_labels does.  PGCN_E_INVALID otherwise. */
int pgcn_dataset_set_graphs(pgcn_dataset *ds, const int *graph_ptr, const int *label,
                            const int *split, int G, int num_classes);
/* The same from the sidecar text file `path` (by convention <root>/data/<name>.graphs): line g is
 * `<rows> <label> <split>` -- graph g owns the next <rows> rows, the rows of all lines sum to
 * num_nodes.  PGCN_E_IO for a missing file, a line that is not three integers, negative rows,
 * rows that do not sum to num_nodes, a label below -1 or >= min(num_classes or 128, 128), a
 * split outside 0..3.  The .pgcnbin cache does not carry graph arrays (pgcn_dataset_save writes
 * the node-level arrays only): attach them after every load. */
int pgcn_dataset_load_graphs(pgcn_dataset *ds, const char *path, int num_classes);
/* Pair-level data for link prediction: attaches E >= 1 node pairs (src, dst in [0, num_nodes)),
 * their labels (1, 0 or -1: unlabelled) and splits (0..3), all copied, and sets output_dim =
 * embed_dim in 1..128, the width of the node embedding the decoder reads.  PGCN_E_INVALID
 * otherwise.  The adjacency is not changed: it stays the message-passing graph, so validation and
 * test positives must be kept out of it by whoever builds the dataset. */
int pgcn_dataset_set_links(pgcn_dataset *ds, const int *src, const int *dst, const int *label,
                           const int *split, long long E, int embed_dim);
/* The same from the sidecar text file `path` (by convention <root>/data/<name>.links): line e is
 * `<src> <dst> <label> <split>`.  PGCN_E_IO for a missing file, a line that is not four integers,
 * an endpoint out of range, a label outside {-1, 0, 1}, a split outside 0..3, no pair at all;
 * PGCN_E_INVALID for embed_dim outside 1..128.  The .pgcnbin cache does not carry pair arrays
 * (the .graphs rule): attach them after every load. */
int pgcn_dataset_load_links(pgcn_dataset *ds, const char *path, int embed_dim);
/* (label_bits / label_words of the view: NULL / 0 for single-label data; num_graphs and the graph
 * arrays: 0 / NULL without graphs; num_pairs and the pair arrays: 0 / NULL without pairs) */
int pgcn_dataset_view(const pgcn_dataset *ds, pgcn_data *view, int *input_dim, int *output_dim);
int pgcn_dataset_free(pgcn_dataset *ds);

/* --- edge-cut partition plan (host only; no device needed) ------------------------------ */
/* contiguous nnz-balanced node ranges: bounds_out[world+1], padded rows per rank */
int pgcn_partition_bounds(int n, const int *indptr, int world, int *bounds_out, int *maxrows);
/* rank's column block of Â in padded row layout (world*maxrows rows, local column ids,
 * global coefficients). Returns nnz (call with null arrays to size them) or a status < 0. */
long long pgcn_partition_subgraph(int n, const int *indptr, const int *indices, int world,
                                  int rank, int *sub_indptr, int *sub_indices, float *sub_vals);

/* --- diagnostics (profiling ablations; not for production use) ------------------------ */
/* The edge-cut engine's GraphSum graph of rank `rank`, reduce-scatter chunk `chunk` of
 * `chunks` at `world` ranks (rows world*maxrows/chunks, columns = the rank's nodes, global
 * coefficients and scales), as GCN builds it: times the per-rank GraphSum of an N-GPU run on
 * one GPU.  *rows / *cols give its shape. */
int pgcn_debug_rank_graph(int n, const int *indptr, const int *indices, int world, int rank,
                          int chunks, int chunk, pgcn_graph **out, int *rows, int *cols);
/* Engine options.  pgcn_debug_set writes one process-wide table; an engine (pgcn_gcn_create*)
 * and a graph (pgcn_graph_create*, pgcn_debug_rank_graph) copy that table when they are created
 * and follow their copy from then on -- an engine hands its copy to every graph it creates,
 * those it builds at a later split switch included.  So a key applies to the engines and graphs
 * created after the call and changes nothing in those that exist.  Two keys are read at the
 * call instead: "parse_threads" (the loader has no engine) and "xstream_ring" (read where the
 * X-stream GEMM launchers dispatch, which pgcn_gemm_xstream* share with the engine).  The
 * reference-shaped C++ API (pgcn.hpp) has no engine: its modules read the table at each call.
 * Each key selects between bit-identical or oracle-tested forms of the same reference epoch
 * (19 keys, r05):
 *   "train_ahead" 0/1, "eval_ax" 0/1, "split_cols" 0/1, "epoch_graph" 0/1, "mm_side" 0/1/2,
 *   "eval_tail" 0/1 (edge-cut between processes: the eval pass's last exchange and output
 *   layer beside the next epoch's first kernels, default 0),
 *   "fuse_epilogue" bits 1 tails | 2 prestaged tables | 4 X-stream epilogue | 8 Dropout /
 *   ReLU backward in a Matmul's input-grad product (default 15),
 *   "fuse_output" 0..3 (default 2), "xstream_ring" 0/1, "lds_min_kb" (< 0: default),
 *   "lds_blocks" 0 (by shape) or 1..32, "parse_threads" (0: up to 16),
 *   "co_draw" 0/1 (sparse X: the hidden dropout's mask drawn in the input dropout's launch,
 *   default 1), "sparse_dual" 0/1 (sparse X: eval's first-layer product also computes the next
 *   training forward's, default 1), "gs_split" 0..3 (the plain GraphSum's rows longer than one
 *   work item on graphs of <= 2^20 slots: 0 a combine launch, 1 the row's last item sums the
 *   slots, 2 long rows as one item, 3 (default) rows of up to 8 workgroup iterations summed
 *   by one workgroup, longer ones as 1), "gs_item_iters" 0/2/4/8/16/32 (group iterations per
 *   work item there; 0 (default): by shape, the shortest leaving <= 1,536 workgroup items),
 *   "gs_orig_cols" 0/1 (a column subset's plain GraphSum gathers through the original column
 *   ids instead of compacting its input, default 1), "gs16_gather" 0..2 (the blocked d = 16
 *   gather kernel: 0 (default) by mean segment length, 1 k_graphsum16, 2 interleaved slots);
 *   r06 (30 keys): "co_draw" also 2 (dense X too, the default), "tn_fold" 0/1 (one GPU and
 *   edge-cut ranks between processes: the weight gradients' last reduction pass inside the
 *   Adam launch / the all-reduce push, default 1), "fuse_finish" 0..2 (one GPU, <= 512 loss
 *   blocks: the loss kernel's last block finishes the pass's scalars, default 1; 2: above 512
 *   blocks too, two levels of arrivals), "mask_per"
 *   0..2 (64-draw mask words per stored RNG state; default 0: 2 for masks of >= 2^20 words,
 *   else 1), "csc_tree" 0/1 (sparse X's
 *   W1.grad as a fixed tree over each feature's entries; default 0: the reference's sequential
 *   order, bit-exact; the tree measured slower), "mask_adam" 0/1 (one GPU: the next epoch's
 *   input mask drawn by the Adam launch, default 1, bit-identical), "mask_xstream" 0/1 (dense X, eval_ax: that mask drawn by
 *   two extra waves of eval's first-layer X-stream pass instead, bit-identical, default 0:
 *   measured slower), "reassoc_small" 0/1 (graphs
 *   under 65,536 nodes: the output layer as (A H) W with its Matmul in the loss kernel even when
 *   the classes are no more than the last hidden width <= 16, default 1; fp32 order only),
 *   "defer_wgrad" 0/1 (one GPU, <= 128 loss blocks: the output layer's W.grad block partials
 *   summed by the Adam launch, default 1; another grouping of the same sums), "peer_uncached" 0/1 (the peer
 *   exchange's receive slots in uncached memory, default 0), and the ring GraphSum's schedule
 *   shapes "ring_pair" 0/1 and "ring_window" 0/2/3 (0: the default window 3), both measured
 *   slower and off;
 * and one diagnostic, not reference-equivalent: "split_rows" 0/1 (the output layer's forward
 *   over the current split's rows only: stale logits elsewhere, which get_var refuses).
 * Returns PGCN_E_INVALID on an unknown key or on a value outside the key's range (nothing is
 * changed then). */
int pgcn_debug_set(const char *key, int value);
/* The table behind pgcn_debug_set, row `index` (0, 1, ...): the key's name (a static string)
 * and its default value; either pointer may be NULL.  PGCN_E_INVALID past the last row.
 * pgcn_gcn_query(g, "knob.<key>") returns the value engine `g` was built with ("lds_min_kb"
 * keeps the caller's unit there, and its default reads as -1). */
int pgcn_debug_knob(int index, const char **name, int *default_value);
/* Host-only check of the d = 16 LDS ring schedule (window must be 5) of a CSR pattern: builds
 * it, walks it as k_graphsum_ring consumes it over a seeded input and returns the max relative
 * error of the row sums against a direct CSR sum, and the number of 4-step entry blocks. */
int pgcn_debug_lds_check(int n_rows, int n_cols, const int *indptr, const int *indices,
                         int window, double *max_rel_err, long long *n_blocks);
/* Host-only: the same schedule's per-(workgroup, slice, wave, slot) step counts (uint16, up to
 * cap) and its shape {n_batches, t_max, waves, slots, window}; returns the count or -1. */
long long pgcn_debug_lds_counts(int n_rows, int n_cols, const int *indptr, const int *indices,
                                int window, unsigned short *dst, long long cap, int *shape5);
/* Launch counts of the engine's kernel families since the last reset (process-wide), so a test
 * can assert which kernels a configuration took: "xs_nn_ring" / "xs_tn_ring" (loader + MFMA-wave
 * X-stream kernels), "xs_nn" / "xs_tn" (register-streamed X-stream kernels), "gs_ring" (LDS ring
 * GraphSum), "gs_gather" (gather GraphSum), "out_xent" (output layer fused into the loss),
 * "gemm_nn" / "gemm_tn" (general MFMA GEMMs), "gat_fwd" / "gat_bwd" (graph attention forward /
 * backward calls, pgcn_gat_fwd / pgcn_gat_bwd and their _mh forms), "gat_heads" (those of them
 * with heads > 1), "spmm_csr" / "spmm_csr_dual" (sparse X: the CSR forward and its dual form,
 * c = X b beside c2 = drop(X) b), "spmm_csc_256" / "spmm_csc_1024" (sparse X: the weight
 * gradient's sequential-chain kernel, 256 threads per feature or 1024 on matrices of more than
 * 512 entries per feature), "spmm_tree_256" / "spmm_tree_1024" (its fixed-tree form, csc_tree),
 * "launches" (every kernel launch of the library), "link_fwd" / "link_bwd" (the pair-score
 * forward and backward calls that launched), "rank_sweep" / "rank_filter" (pgcn_link_rank's
 * sweep and filter-correction launches), "topk_sweep" / "topk_merge" (pgcn_link_topk's two).
 * A non-null name returns its count (then zeroes it
 * when reset bit 0 is set); a null name with reset bit 0 zeroes every counter.  Bit 1 of reset
 * selects the counters of the calling host thread instead of the process-wide ones (each rank
 * of an in-process loopback group runs on a thread of its own).  Status < 0 on an unknown
 * name. */
long long pgcn_debug_path_count(const char *name, int reset);
/* n empty kernels back to back on `stream` (the per-launch floor the small graphs' epochs are
 * compared with: launches per epoch x the time of one empty launch). */
int pgcn_debug_empty_launches(int n, void *stream);
/* mine[i] = the loss kernel's exp of x[i] (x <= 0: the device expf sequence without its
 * overflow select), lib[i] = the device library's expf(x[i]); device pointers */
int pgcn_debug_exp_check(const float *x, long long n, float *mine, float *lib, void *stream);
/* q[i] = the loss kernel's quotient a[i] / b[i] (div_rn: from the reciprocal of b[i], the IEEE
 * division below 2^-125); device pointers */
int pgcn_debug_div_check(const float *a, const float *b, long long n, float *q, void *stream);

/* --- the loss kernel family, every argument exposed (kernel tests) ----------------------
 * Arguments are checked before anything touches the device (PGCN_E_INVALID); n = 0 (n_blocks =
 * 0 for the reductions) is PGCN_OK and launches nothing.  Device pointers throughout. */
/* The pass's scalars finished by the loss kernel's last block instead of pgcn_finalize: every
 * block stores {loss, wrong, its slice of sum w^2, 0} to part4[block] (16 B each) and arrives on
 * *ticket; the last one sums them and writes out2 = {loss / count + wd * sum w^2 / 2, (count -
 * wrong) / count} (with ctr, a device {step, epoch} pair: at out2 + 4 * (ctr[1] % ring_cap)),
 * sums = {loss, wrong} when given, and zeroes the ticket.  group > 0: two levels -- blocks
 * arrive in groups of `group` on gticket[16 g], a group's last block sums its partials into
 * gpart4[g] (16 B each) and arrives on *ticket; ceil(blocks / group) groups.  ticket and
 * gticket must be zero before the first launch; w may be NULL when n_w = 0. */
typedef struct {
  const float *w;
  long long n_w;
  float wd;
  float *out2;
  const int *ctr;
  int ring_cap;
  float *sums;
  unsigned int *ticket;
  void *part4;
  int group;
  unsigned int *gticket;
  void *gpart4;
} pgcn_xent_final;
/* rows per slice of the ring GraphSum's prescaled table (the layout pgcn_debug_out_xent's
 * table is written in) */
int pgcn_debug_ring_slice_rows(void);
/* pgcn_xent_fwd with write_back (0: the logits buffer is left untouched) and the fused finish
 * (NULL: none).  1 <= c <= ld <= 124, ld a multiple of 4; grad may be NULL when !training. */
int pgcn_debug_xent_fwd(float *logits, int ld, float *grad, const int *truth, int n, int c,
                        int count, int training, float *partials, int write_back,
                        const pgcn_xent_final *fin, void *stream);
/* The output layer fused into the loss: logits = H W (H [n][ldh], 1 <= kh <= 16 columns; W
 * [kh][ldw]) written max-shifted on labelled rows, then pgcn_xent_fwd's loss / grad / partials
 * (1 <= c <= ld <= 116, ld a multiple of 4).  training with dH: dH [n][lddh] = grad W^T, columns
 * [kh, min(16, lddh)) zero, lddh >= kh.  training with dWp (ld <= 48): per-block partials
 * [pgcn_xent_blocks(n)][kh][48] of H^T grad, columns [c, 48) zero, for
 * pgcn_debug_tn_reduce_blocks.  training with dH and table (kh = 16, scale given): float4
 * (p / S) * 4 S + v * S + p % S of table = scale[p] * dH[i][4 v .. 4 v + 3] for v < 4, with S =
 * pgcn_debug_ring_slice_rows() and p = pos[i] (skipped when < 0), or p = i for i < table_rows
 * when pos is NULL.  fin as above (NULL: none). */
int pgcn_debug_out_xent(const float *H, int ldh, int kh, const float *W, int ldw, float *logits,
                        int ld, float *grad, const int *truth, int n, int c, int count,
                        int training, float *partials, float *dH, int lddh, float *dWp,
                        float *table, const float *scale, const int *pos, int table_rows,
                        const pgcn_xent_final *fin, void *stream);
/* pgcn_finalize's launch with the results-ring slot: out2 (2 floats written) at out2 + 4 *
 * (ctr[1] % ring_cap) when ctr (a device {step, epoch} pair) is given; sums (may be NULL) =
 * {loss sum, wrong}. */
int pgcn_debug_finalize_ring(const float *partials, int n_blocks, int count, const float *w_l2,
                             long long n_l2, float weight_decay, float *out2, const int *ctr,
                             int ring_cap, float *sums, void *stream);
/* C [K][ldc] (columns [N, ldc) zero) = the n_blocks partials [K][ldp] summed in a fixed order:
 * groups of spg consecutive partials in order, then the group sums in order, spg the smallest
 * multiple of 16 with spg^2 >= n_blocks (one sequential pass when n_blocks <= spg).  `partial`
 * holds pgcn_debug_tn_reduce_blocks_workspace bytes: the partials first, the group sums after
 * them.  N <= ldc <= ldp.  The one-pass form sums n partials sequentially, no workspace. */
size_t pgcn_debug_tn_reduce_blocks_workspace(int n_blocks, int K, int ldp);
int pgcn_debug_tn_reduce_blocks(float *partial, int n_blocks, int K, int N, int ldp, float *C,
                                int ldc, void *stream);
int pgcn_debug_tn_reduce_one_pass(const float *partial, int n, int K, int N, int ldp, float *C,
                                  int ldc, void *stream);
/* pgcn_gemm / pgcn_gemm_tn with A's dropout bits in the nibble layout as well (mask_nib, from
 * pgcn_mask_nibbles of the same bitmap; NULL: none), as the engine hands them to a dense first
 * layer of 33..128 columns: the wide kernels read the nibbles instead of the flat bitmap when
 * a_mask is given and K <= 1024; every other shape ignores them.  Same argument checks and the
 * same bits as the plain entries. */
int pgcn_debug_gemm_nib(int M, int N, int K, const float *A, int lda, const float *B, int ldb,
                        int trans_b, float *C, int ldc, const uint64_t *a_mask,
                        long long mask_base, long long mask_ld, float a_scale,
                        const uint64_t *mask_nib, void *stream);
int pgcn_debug_gemm_tn_nib(int M, int N, int K, const float *A, int lda, const float *G, int ldg,
                           float *C, int ldc, const uint64_t *a_mask, long long mask_base,
                           long long mask_ld, float a_scale, const uint64_t *mask_nib,
                           void *workspace, void *stream);
/* The sparse first layer's products with every argument the engine varies (pgcn_spmm_csr and
 * pgcn_spmm_csc_bwd fix ldc = ldg = p, mask_base = 0, nnz = 0, no order, the chain kernel).
 * Bit `mask_base + position` of `mask` keeps value `position` of `a` (NULL: no dropout); b and
 * bgrad are tight ([..][p]), c / c2 / cgrad have rows of ldc / ldg >= p floats whose padding is
 * never written and never reaches a result.
 * pgcn_debug_spmm_csr: c2 == NULL: c = drop(X) b; else the dual forward, c = X b and
 * c2 = drop(X) b from one pass (mask required: PGCN_E_INVALID without it, nothing written).
 * pgcn_debug_spmm_csc_bwd: bgrad = drop(X)^T cgrad over the transposed index of
 * pgcn_csr_transpose; nnz (the entries of all nf columns, 0: unknown) above 512 nf selects the
 * 1024-thread kernels; order (optional): the nf feature ids in workgroup launch order (any
 * permutation gives the same bits); tree != 0: the fixed-tree kernel (csc_tree) instead of the
 * sequential chain. */
int pgcn_debug_spmm_csr(int m, int p, int ldc, const int *indptr, const int *indices,
                        const float *a, const uint64_t *mask, long long mask_base, float scale,
                        const float *b, float *c, float *c2, void *stream);
int pgcn_debug_spmm_csc_bwd(int nf, int p, int ldg, const int *csc_ptr, const int *csc_row,
                            const int *csc_pos, const float *a, const uint64_t *mask,
                            long long mask_base, float scale, const float *cgrad, float *bgrad,
                            long long nnz, const int *order, int tree, void *stream);
/* pgcn_dropout_mask with the engine's other arguments: per = 1 | 2 mask words (64 draws each)
 * per stored state (per = 2: state k sits at draw elem0 + 128 k and ceil(n_chunks / 2) states
 * are read and advanced); max_blocks > 0 caps the grid (0: by size).  Words [0, n_chunks) of
 * `mask` are written: bit j of word c is element elem0 + 64 c + j, zero from elem_end on.
 * pgcn_debug_dropout_mask2 draws two such segments in one launch (one jump table: the same
 * period); a segment with n_chunks = 0 is skipped. */
int pgcn_debug_dropout_mask(uint64_t *states, long long n_chunks, long long elem0,
                            long long elem_end, float p, uint64_t *mask, const void *table,
                            int per, int max_blocks, void *stream);
int pgcn_debug_dropout_mask2(uint64_t *states0, long long n_chunks0, long long elem0_0,
                             long long elem_end0, float p0, uint64_t *mask0, int per0,
                             uint64_t *states1, long long n_chunks1, long long elem0_1,
                             long long elem_end1, float p1, uint64_t *mask1, int per1,
                             const void *table, void *stream);
/* pgcn_dropout_apply reading keep bit base + i for x[i] (x 16-byte aligned) */
int pgcn_debug_dropout_apply(float *x, long long n, const uint64_t *mask, long long base,
                             float scale, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PGCN_H */
