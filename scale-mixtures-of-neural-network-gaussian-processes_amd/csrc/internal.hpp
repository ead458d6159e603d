// internal.hpp — C++-side interfaces between the translation units of libsmnngp.so.
#pragma once
#include <climits>
#include <cmath>
#include <functional>

#include "common.hpp"

constexpr int kTile = 128;   // GEMM block edge; every padded dimension is a multiple of it
constexpr int kMaxColPieces = 32;   // pieces of a column-first exchange

// Cyclic column-first shard of the symmetric kernel build over P ranks (host side: sharding.py, same formulas).
//   tile rows (128 rows) are dealt in boustrophedon order with period 2P: group j = tile rows [jP, (j+1)P), rank r owns
//   t_j(r) = jP + (j even ? r : P-1-r)  -- tile row t holds t+1 lower tiles, and every pair of groups gives every rank the same
//   number of them, so the build is balanced and EVERY aligned group of P tile rows holds exactly one tile row per rank;
//   piece g = tile columns [c[g], c[g+1]) of every tile row from the group of c[g] down (group f = floor(c[g] / P)): slots =
//   ceil(T / P) - f strips of 128 x (c[g+1]-c[g])*128 elements per rank -- the same count on every rank, so ONE equal-count
//   all-gather moves a whole column range of the lower triangle (tile rows that start inside or above it carry their
//   above-diagonal tiles as padding: at most one strip per rank and piece when c[g] is not a multiple of P).
struct ColPieces {
  int P = 1, np = 0;
  int64_t T = 0;                       // tile rows of the kernel: ceil(n / 128)
  int64_t c[kMaxColPieces + 1] = {};   // tile-column boundaries, c[0] = 0, c[np] = T
  int64_t off[kMaxColPieces + 1] = {}; // element offset of piece g in a rank's chunk; off[np] = elements per rank
  int64_t slots(int g) const { return (T + P - 1) / P - c[g] / P; }
  int64_t width(int g) const { return (c[g + 1] - c[g]) * kTile; }
  int64_t count(int g) const { return slots(g) * kTile * width(g); }
};
int col_pieces_make(smn_ctx* ctx, int64_t n, int nranks, int npieces, const int64_t* piece_cols, ColPieces* out);

struct BuildSpec {
  int dtype, net, act, num_hiddens;
  double w_std, b_std, last_w_std;
};

// The `net` argument of the model entries: SMN_NET_MLP or SMN_NET_DENSE_RESNET, with SMN_NET_NTK OR-ed in where the entry's
// covariance is the tangent kernel Theta instead of the NNGP kernel K.  split_net leaves the architecture in *net and the flag in
// *ntk; any other bit is SMN_EINVAL naming the value.  no_ntk_net: entries that have no Theta form (the batched and grid ones).
inline int split_net(smn_ctx* ctx, int* net, bool* ntk) {
  const int base = *net & ~SMN_NET_NTK;
  if (base != SMN_NET_MLP && base != SMN_NET_DENSE_RESNET) return smn_fail(ctx, SMN_EINVAL, "unknown net %d", *net);
  *ntk = (*net & SMN_NET_NTK) != 0;
  *net = base;
  return SMN_OK;
}
inline int no_ntk_net(smn_ctx* ctx, const char* who, int net) {
  const int base = net & ~SMN_NET_NTK;
  if ((net & SMN_NET_NTK) && (base == SMN_NET_MLP || base == SMN_NET_DENSE_RESNET))
    return smn_fail(ctx, SMN_ENOTSUP, "%s: no SMN_NET_NTK form (net %d)", who, net);
  return SMN_OK;   // (any other value is the entry's own SMN_EINVAL)
}

enum { STORE_BOUNDS = 0, STORE_PAD_IDENTITY = 1 };

// One fused Gram + layer-recursion launch.  Operands are PADDED copies (rows a multiple of 128,
// K a multiple of 32 elements, zero filled) made by pad_rows(); q1/q2 are ||x||^2/d per padded row.
struct BuildCall {
  BuildSpec spec;
  const void* x1p; int64_t ld1; int64_t rows1;
  const void* x2p; int64_t ld2; int64_t rows2;
  int kp; int64_t d;
  const double* q1; const double* q2;
  int symmetric;               // 1: x2 == x1, only tiles with tc <= tr are computed
  int mirror;                  // symmetric only: also store the transposed tile (full matrix out)
  int lower_skip;              // rectangular only: skip tiles wholly above the global diagonal (row shards)
  int64_t row_off, col_off;    // added to local indices for the row == col (exact diagonal) test
  int exact_diag;              // write the closed-form diagonal where global row == global col
  int store_mode;              // STORE_BOUNDS: write [0,out_rows) x [0,out_cols) only
  int64_t out_rows, out_cols;  // STORE_PAD_IDENTITY: write everything, identity outside `valid`
  int64_t nv0, aug0, nv1;      // valid(i) = i < nv0 || (aug0 <= i < aug0 + nv1)
  int get_mask;
  void* out_k; void* out_t; int64_t ldo;
  // paired lower-block shard (symmetric operands): two tile-aligned row blocks [rb,re), each written as
  // rows x columns [0,re) into its own packed output of leading dimension shard_ld
  int shard; int64_t shard_rb[2], shard_re[2]; void* shard_k[2]; void* shard_t[2]; int64_t shard_ld[2];
  // shard == 2: cyclic column-first shard (ColPieces below); shard_k[0] / shard_t[0] = the rank's chunk
  int cy_P, cy_rank, cy_np; int64_t cy_c[kMaxColPieces + 1]; int64_t cy_off[kMaxColPieces];
  // batched build (nbatch > 0): the same operands under nbatch layer programs that differ in (w_std, b_std, last_w_std)
  // only -- host arrays bw / bb / blw --, problem g written at out_k + g * out_bs elements
  int nbatch; const double* bw; const double* bb; const double* blw; int64_t out_bs;
  // split_corner = TB > 0 (symmetric, un-sharded, one problem): the tiles with row AND column >= T - TB go out as a second
  // launch on the bulk stream, still in flight when run_build returns (BuildOut::corner_col)
  int split_corner;
  // want_trace: leave sum_i<nv0 K_ii (from the exact-diagonal table) in ctx->d_scal[1] (BuildOut::trace)
  int want_trace;
  // Gram cache (smn_spr_loss; gram_cache_plan): GRAM_CALL_STORE = the fused build also leaves its raw accumulators in the
  // context's cache when x equals the cached copy; GRAM_CALL_BOTH = the cached accumulators are valid for the cached copy: every
  // launch goes out in both forms and the device word decides which of the two runs.  gram_gen = this call's generation number.
  int gram_mode; unsigned gram_gen;
};
enum { GRAM_CALL_NONE = 0, GRAM_CALL_FIRST = 1, GRAM_CALL_STORE = 2, GRAM_CALL_BOTH = 3 };
// What one smn_spr_loss call does with the context's Gram cache (kernel_build.hip).  plan never fails: anything in the way
// (switched off, too small, too large, no memory, another key) ends in GRAM_CALL_NONE or a cold cache.  settle, after the
// call's synchronisation, moves the state on what the device reported; rc != SMN_OK drops the cache.
struct GramPlan {
  int mode = GRAM_CALL_NONE;
  unsigned gen = 0;
  void* xc = nullptr;   // the cache's own padded copy ([n_total] doubles q, then [n_total, kp] elements): the build's operand
};
GramPlan gram_cache_plan(smn_ctx* ctx, int dtype, int net, int64_t n, int64_t d, int64_t kp, int64_t n_total);
void gram_cache_settle(smn_ctx* ctx, const GramPlan& p, int rc);
void gram_cache_drop(smn_ctx* ctx, bool free_memory);
// What a build leaves behind for the factorisation after it (heads.hip aug_finish).
struct BuildOut {
  int64_t corner_col = 0;   // first column of the corner of a split build, still being built on the bulk stream (0: none)
  bool trace = false;       // the trace of the kernel's diagonal is in ctx->d_scal[1]
  // the closed-form diagonals K(x1_i, x1_i) / Theta(x1_i, x1_i) of the rows1 operand (the table exact_diag reads, element type
  // = the build's; diag_t is Theta only under SMN_GET_NTK): in workspace slot 1, valid until the context's next build
  const void* diag_k = nullptr; const void* diag_t = nullptr;
};
int run_build(smn_ctx* ctx, const BuildCall& c, BuildOut* out = nullptr);   // out: needed by split_corner
// TB for a split build of T tile rows on this context (0: do not split)
int split_corner_tiles(const smn_ctx* ctx, int64_t tiles);

// dst[rows_pad, kp] (ld = kp) <- zero-padded copy of src[n, d]; also q[rows_pad] = ||row||^2 / d.
// rows_a > 0: rows [rows_a, rows_pad) are src2[n2, d] (zero-padded like the first block): one launch for both blocks of an
// augmented operand
int pad_rows(smn_ctx* ctx, int dtype, const void* src, int64_t n, int64_t lds, int64_t d,
             void* dst, int64_t rows_pad, int64_t kp, double* q, int64_t rows_a = 0, const void* src2 = nullptr, int64_t n2 = 0,
             int64_t lds2 = 0, unsigned* changed = nullptr, unsigned gen = 0);
// (changed != nullptr: the compare form -- dst holds an earlier call's copy; elements that differ bitwise are rewritten and
// *changed = gen is stored by every lane that saw one)

inline int64_t k_pad(int dtype, int64_t d) { return round_up(d, dtype == SMN_F64 ? 16 : 32); }

// One partial Cholesky on a padded matrix (n_total, n_factor multiples of 128).  Device-side results: logdet (double) and
// info (int) are left in ctx->d_scal[0] / ctx->d_info[0] (batched: batch_logdet[g] / batch_info[g]); no host sync.
struct FactorCall {
  int dtype; void* a; int64_t n_total, n_factor, lda;
  int64_t n_shift; double jitter_abs, ridge_rel;
  bool keep_factor;
  int64_t id0 = -1, id1 = -1;   // appended rows [id0, id1) hold an identity block (row id0 + i is zero left of column i)
  bool prepped = false;         // the caller has shifted the diagonal and reset logdet / info already (aug_prep)
  bool noschur = false;         // the appended rows' trailing block is neither read nor written (cholesky.hip)
  // batched (batch_logdet != nullptr, a batch of one included): `batch` problems of identical shape, problem g at
  // a + g * batch_stride elements; every panel / update launch gets grid.y = batch
  int batch = 1; int64_t batch_stride = 0; double* batch_logdet = nullptr; int* batch_info = nullptr;
  // pieces of the matrix still landing (cholesky.hip need_columns), their events recorded on stream arrivals_on; the
  // caller's stream is behind all of them when the factorisation returns
  const smn_ctx::Arrival* arrivals = nullptr; size_t n_arrivals = 0; hipStream_t arrivals_on = nullptr;
};
int cholesky_padded(smn_ctx* ctx, const FactorCall& f);
// K written by the caller: fill(k_d, ldk) puts the lower triangle of K (n rows) into the matrix it is handed (heads.hip)
using KernelInto = std::function<int(void* k_d, int64_t ldk)>;
// Gaussian / multivariate-t log-pdf from (quad = y^T cov^-1 y, logdet = log det cov) in dimension n (heads.hip)
double logpdf_from(double quad, double logdet, int64_t n, double df, double scale, int info);
// What a factorisation leaves for the host: one quadratic form per target column, logdet K~ and info (0, or the first failing
// pivot).  THE NaN CONVENTION: info != 0 makes logdet and every quadratic form NaN -- head_decode applies it to a device record
// {logdet, info as a double (INT_MAX: never set = 0), quad[0..nq)}, the layout of the mailbox and of a row of spr_batch's res.
struct HeadScalars {
  double quad[48]; double logdet = 0.0; int info = 0;
};
inline void head_decode(const volatile double* rec, int nq, HeadScalars* h) {
  h->info = (int)rec[1];
  if (h->info == INT_MAX) h->info = 0;
  h->logdet = h->info != 0 ? std::nan("") : rec[0];
  for (int i = 0; i < nq; ++i) h->quad[i] = h->info != 0 ? std::nan("") : rec[2 + i];
}
// The mailbox, decoded.  fetch_mail: after a launch that published into it (extract_posterior(..., publish = true)) -- ONE
// synchronisation and the read.  fetch_results: the tiny publish launch for nq device doubles (quadratic forms), then that.
int fetch_mail(smn_ctx* ctx, int nq, HeadScalars* h);
int fetch_results(smn_ctx* ctx, const double* quad_dev, int nq, HeadScalars* h);
// The joint head of c target columns from their quadratic forms, published to whichever outputs the caller wants: total quad,
// log-pdf in dimension n c with logdet c logdet K~, the per-column quads, logdet, info, and NaN terms when the matrix was not
// positive definite.  Returns the total.  A single-output entry (multi = false) publishes its one quadratic form as it is:
// 0.0 + quad would turn a -0.0 into +0.0.
inline double publish_head(const HeadScalars& h, int64_t c, bool multi, int64_t n, double df, double scale, double* logpdf_h,
                           double* quad_h, double* quad_cols_h, double* logdet_h, int* info_h, double* terms_h = nullptr) {
  double tot = h.quad[0];
  if (multi) {
    tot = 0.0;
    for (int64_t k = 0; k < c; ++k) tot += h.quad[k];
  }
  if (h.info != 0) tot = std::nan("");
  if (logpdf_h) *logpdf_h = logpdf_from(tot, (double)c * h.logdet, n * c, df, scale, h.info);
  if (quad_h) *quad_h = tot;
  for (int64_t k = 0; k < c && quad_cols_h; ++k) quad_cols_h[k] = h.info != 0 ? std::nan("") : h.quad[k];
  if (logdet_h) *logdet_h = h.logdet;
  if (info_h) *info_h = h.info;
  for (int i = 0; i < 4 && terms_h && h.info != 0; ++i) terms_h[i] = std::nan("");
  return tot;
}
// coef of the Student-t head of c columns, G = coef A A^T - c K~^-1: (df + n c) / ((df + Q / s) s), Q = the total quadratic
// form; 1 for the Gaussian head.  Operation by operation the expression the device-side grad_coef (grad.hip) repeats.
inline double lml_coef(double df, double scale, double quad_total, int64_t n, int64_t c) {
  if (!(df > 0.0)) return 1.0;
  return (df + (double)n * (double)c) / ((df + quad_total / scale) * scale);
}
// The factored posterior every gradient, leave-one-out and K~^-1 entry starts from: alpha = K~^-1 Y [n, c] row-major and -K~^-1
// (lower triangle, ld = ldinv) in workspace slot 7 -- or in the caller's buffers --, the c quadratic forms, logdet K~ and info
// (NaN in quad and logdet when info != 0).  The MLP / dense-ResNet builder also leaves the Gram matrix k0 = x x^T / d (ld = ld0)
// and its diagonal q in slot 5: what the tangent pass of grad.hip reads.  A new objective adds a tail behind one of these, a new
// kernel family a builder beside them; neither copies the pipeline.
struct Posterior : HeadScalars {
  void* k0 = nullptr; void* q = nullptr; int64_t ld0 = 0;
  void* ninv = nullptr; int64_t ldinv = 0; void* alpha = nullptr;
};
// from x [n, d]: gram_lower, then K (spec.net may carry SMN_NET_NTK: Theta, the posterior is that of Theta~ = Theta + eps I) by
// the layer recursion of the Gram matrix.  ninv_d / alpha_d: the caller's storage (ld = ldinv) instead of slot 7.
int posterior_from_x(smn_ctx* ctx, const BuildSpec& spec, const void* x_d, int64_t n, int64_t ldx, int64_t d, const void* y_d,
                     int64_t c, double eps_abs, Posterior* p, void* ninv_d = nullptr, int64_t ldinv = 0, void* alpha_d = nullptr);
// from K written by `build` into the factorisation workspace
int posterior_from_build(smn_ctx* ctx, int dtype, int64_t n, const KernelInto& build, const void* y_d, int64_t c, double eps_abs,
                         Posterior* p);
// from images x [n, H, W, C] under get_cnn_kernel (spec.net is not read): the lower build of smn_kernel_cnn
int posterior_from_images(smn_ctx* ctx, const BuildSpec& spec, const void* x_d, int64_t n, int64_t H, int64_t W, int64_t C,
                          const void* y_d, int64_t c, double eps_abs, Posterior* p);
// true from the size on at which the gradient takes the rectangle route instead of the joint factorisation (heads.hip)
bool grad_uses_rectangle(int64_t n);
int gram_lower(smn_ctx* ctx, int dtype, const void* x_d, int64_t n, int64_t ldx, int64_t d, void* k0_d, int64_t ldk, void* q_d);
// smn_recursion's symmetric NNGP form (lower 64x64 tiles + mirror, exact diagonal) for nbatch problems over ONE Gram matrix:
// problem g runs under (w_std[g], b_std[g], last_w_std[g]) (host arrays; the spec's own three are not read) and writes
// out_d + g * out_bs elements (ld = ldo).
// One table launch and one recursion launch with grid.y = nbatch; per problem the bits of the serial call.
// No synchronisation: the host source of the layer programs' upload is kept in `stage`, which the caller leaves alone until it
// has synchronised the stream itself.
int recursion_lower_batch(smn_ctx* ctx, const BuildSpec& spec, int nbatch, const double* w_std, const double* b_std,
                          const double* last_w_std, const void* k0_d, int64_t n, int64_t ldk0, const void* q_d, void* out_d,
                          int64_t ldo, int64_t out_bs, std::vector<char>& stage);
// -x x^T (lower, into neg_inv [n, n] ld = ldo) and alpha = x z from the rows x [n, kcols] (ld = ldx, row i zero left of its
// 128-column tile) and the vector z [kcols]; *quad_dev = z^T z.  c > 1: z [c, kcols] (ld = ldz) holds c vectors, alpha is
// [n, c] row-major and quad_dev [c].  cholesky.hip.
int inverse_from_rows(smn_ctx* ctx, int dtype, const void* x, int64_t ldx, const void* z, int64_t kcols, int64_t n,
                      void* neg_inv, int64_t ldo, void* alpha, double* quad_dev, int64_t c = 1, int64_t ldz = 0);

// small helpers implemented in util.hip
int fill_identity_pad(smn_ctx* ctx, int dtype, void* a, int64_t lda, int64_t n_pad, int64_t n_valid);
int copy_matrix(smn_ctx* ctx, int dtype, void* dst, int64_t ldd, const void* src, int64_t lds,
                int64_t rows, int64_t cols, int lower_only);
// a[row0 + k, i] = (i < n ? y[i*ldy + k] : 0) for k < c, i < ncols   (whole rows are written)
int set_aug_rows(smn_ctx* ctx, int dtype, void* a, int64_t lda, int64_t row0, int64_t ncols, const void* y,
                 int64_t n, int64_t c, int64_t ldy);
// predictive read-out of a factored augmented matrix (see heads.hip)
int extract_posterior(smn_ctx* ctx, int dtype, const void* a, int64_t lda, int64_t aug0, int64_t t, int64_t c,
                      void* mean, void* cov, int64_t ldcov, double* quad_dev, bool publish = false);
// set_aug_rows + absolute diagonal shift + reset of logdet / info in one launch (cholesky_padded then runs with
// FactorCall::prepped set and skips its own two)
// (columns [col0, ncols) only, on stream st: the corner of a split build is prepped behind its own launch)
// ridge_rel != 0: the shift is jitter_abs + ridge_rel * d_scal[1] / n_trace (the trace left there by the build: want_trace)
int aug_prep(smn_ctx* ctx, int dtype, void* a, int64_t lda, int64_t row0, int64_t ncols, const void* y, int64_t n,
             int64_t c, int64_t ldy, int64_t n_shift, double jitter_abs, int64_t col0 = 0, hipStream_t st = nullptr,
             double ridge_rel = 0.0, int64_t n_trace = 0);
int solve_rows_padded(smn_ctx* ctx, int dtype, void* a, int64_t n_total, int64_t n_factor, int64_t lda);
// Schur update of solved appended rows: the lower tiles of a[n_factor:n_total, n_factor:n_total] -= R R^T with R = rows
// [n_factor, n_total) x columns [0, n_factor) -- the far update of cholesky_padded, one launch per super-panel of columns
int schur_rows_padded(smn_ctx* ctx, int dtype, void* a, int64_t n_total, int64_t n_factor, int64_t lda);
int transpose_matrix(smn_ctx* ctx, int dtype, void* dst, int64_t ldd, const void* src, int64_t lds,
                     int64_t rows, int64_t cols);   // dst[c, r] = src[r, c]
// dst[i, j] = src[n-1-j, n-1-i] for j <= i  (J L^T J);  transpose with the src rows / dst rows reversed
int flip_transpose_lower(smn_ctx* ctx, int dtype, void* dst, int64_t ldd, const void* src, int64_t lds, int64_t n);
int transpose_flip(smn_ctx* ctx, int dtype, void* dst, int64_t ldd, const void* src, int64_t lds, int64_t rows,
                   int64_t cols, int flip_src_rows, int flip_dst_rows);
// column-first exchange (comm.hip): the all-gather of piece g on stream `st`, and its scatter into k (lower triangle by
// 128-column tiles; diag_add is added to the diagonal entries as they are written: the absolute jitter of SPR.loss)
int allgather_piece_on(smn_ctx* ctx, hipStream_t st, int dtype, const void* mine_d, void* stage_d, const ColPieces& cp, int g);
int scatter_piece_on(smn_ctx* ctx, hipStream_t st, int dtype, const void* stage_d, int64_t n, const ColPieces& cp, int g,
                     void* k_d, int64_t ldk, double diag_add);

// The derivative of an MLP / dense-ResNet kernel entry in its first argument (input_grad.hip).  Operands are padded copies as
// pad_rows leaves them (rows a multiple of 128, ld = kp); spec.net is the architecture alone, `ntk` says the kernel is Theta.
struct InputGradOps {
  BuildSpec spec; bool ntk;
  const void* x1p; const double* q1; int64_t n1, rows1;
  const void* x2p; const double* q2; int64_t n2, rows2;
  const void* x2t;   // [round_up(d, 128), rows2]: the padded x2 transposed (input_grad_transpose)
  int64_t kp, d;
};
// One call's scratch, carved from a single allocation.  Plain form: f1, f2 = F_1, F_2 [rows1, rows2]; seeded form: partial.
// w [rows1, rows2] = seed o F_1 and s [rows1] = rowsum(seed o F_2) feed the contraction; ddiag [rows1] = d K_rr / d q0_r.
struct InputGradWs {
  void* tab1; void* tab2; void* ddiag; double* s; void* w; void* f1; void* f2; double* partial;
  size_t bytes;   // of the whole layout
};
constexpr int kTabFields = 4;   // the table layout input_grad_tables writes, per activation layer and row: q, p = dq/dq0, ra, rb
int input_grad_nsets(const BuildSpec& spec);   // activation layers of the stack
// The argument checks every input-gradient entry shares: dtype, net (its SMN_NET_NTK flag split off into *ntk), act, num_hiddens
// and the number of activation layers.  Leaves the architecture alone in spec->net.
int input_grad_check(smn_ctx* ctx, const char* who, int dtype, int net, int act, int num_hiddens, double w_std, double b_std,
                     double last_w_std, BuildSpec* spec, bool* ntk);
bool input_grad_seeded_fused(int dtype, bool ntk);   // false: no fused seeded kernel for this form (plain form + input_grad_seed)
size_t input_grad_ws_bytes(int dtype, int nsets, int64_t rows1, int64_t rows2, bool seeded);
InputGradWs input_grad_ws_carve(void* base, int dtype, int nsets, int64_t rows1, int64_t rows2, bool seeded);
// tables + the hot kernel.  gbar_d == nullptr: F_1, F_2 into ws.f1 / ws.f2; else gbar o F_1 into ws.w and the row sums into ws.s
int input_grad_factors(smn_ctx* ctx, const InputGradOps& o, const InputGradWs& w, const void* gbar_d, int64_t ldg);
// the table kernel alone: tab_d [nsets][4][rows] = (q, p = dq/dq0, ra, rb) per activation layer and row of q64 [rows], and
// ddiag_d [rows] = dK_rr/dq0 (ntk: dTheta_rr/dq0), both of spec.dtype (input_grad_sym.hip)
int input_grad_tables(smn_ctx* ctx, const BuildSpec& spec, bool ntk, const double* q64, int64_t rows, void* tab_d, void* ddiag_d);
// ws.w = F_1 o seed, ws.s = rowsum(F_2 o seed); seed [rows1, rows2] with row stride lds, or one row for all (lds = 0)
int input_grad_seed(smn_ctx* ctx, const InputGradOps& o, const InputGradWs& w, const void* seed_d, int64_t lds);
// out[r, e] = ca (ws.w X2)[r, e] + (cs ws.s[r] + cd ws.ddiag[r]) x1[r, e]   (r < n1, e < d; cd == 0: ws.ddiag is not read).
// fpart_d != nullptr: fpart_d [rows1 / 128][round_up(d, 128)] takes, per 128-row tile and e, the fp64 sum of out o x1 over the
// tile's rows (input_grad_sym.hip adds the tiles up in order), and out_d may be null.  Reads o.spec.dtype, x1p, x2t, n1, rows1,
// rows2, kp, d and ws.w, ws.s, ws.ddiag.
int input_grad_contract(smn_ctx* ctx, const InputGradOps& o, const InputGradWs& w, double ca, double cs, double cd, void* out_d,
                        int64_t ldo, double* fpart_d = nullptr);
// xt_d [round_up(d, 128), rows] = the padded xp [rows, kp] transposed, zero rows behind d
int input_grad_transpose(smn_ctx* ctx, int dtype, const void* xp, int64_t rows, int64_t kp, int64_t d, void* xt_d);
// dst[r, cols - 1 - j] = src[r, j]
int flip_rows(smn_ctx* ctx, int dtype, void* dst, int64_t ldd, const void* src, int64_t lds, int64_t rows, int64_t cols);

// K(x_i, x_i) for i < n: the per-image pass of smn_kernel_cnn / smn_kernel_conv_resnet alone (cnn.hip / cnn_resnet.hip), the
// same launch that fills the diagonal of their symmetric build, so the values are those bits.  diag_d [n] of `dtype`.
int cnn_diag(smn_ctx* ctx, int dtype, int act, int layers, double w, double b, double lw, const void* x_d, int64_t n,
             int64_t H, int64_t W, int64_t C, void* diag_d);
int conv_resnet_diag(smn_ctx* ctx, int dtype, int act, int block_size, double w, double b, double lw, const void* x_d,
                     int64_t n, int64_t H, int64_t W, int64_t C, void* diag_d);
