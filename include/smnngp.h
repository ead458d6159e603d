/* smnngp.h — C-ABI of libsmnngp.so: the MI355X (gfx950) scale-mixture NNGP hot path.
 *
 * Drop-in boundary for ONE path of Hyungi-Lee/Scale-Mixtures-of-Neural-Network-Gaussian-Processes:
 * NNGP/NTK kernel-matrix build -> jittered Cholesky -> triangular solves -> Gaussian / Student-t
 * log-marginal-likelihood and predictive mean / covariance.  The reference has no FFI of its own
 * (it is pure Python over JAX + neural_tangents); every entry point below names the reference
 * call (file:line under /root/reference) whose arithmetic it replaces.  The Python side binds this
 * header with ctypes; there are no torch / JAX types anywhere in the ABI.
 *
 * Conventions
 *   - every function returns int status: SMN_OK (0) or a negative SMN_E* code; the message is
 *     kept per context and read with smn_last_error().  Nothing throws across the ABI.
 *   - matrices are dense row-major with an explicit leading dimension (elements, not bytes).  A matrix may be a
 *     window into a larger allocation: an entry reads and writes only the rows x cols elements it is given, never the
 *     ld - cols elements between two rows nor anything before the first or after the last row.  Every leading
 *     dimension must be at least the number of elements of a row it strides (ldx >= d, ldk >= the columns of the
 *     kernel block, ldk >= n + t for the joint kernel of smn_predict, ldcov >= t, ldb >= nrhs, ...): a smaller one
 *     would make rows alias each other and is refused with SMN_EINVAL and a message that names the argument, before
 *     anything is allocated or launched.  No alignment is required of pointers or leading dimensions except where
 *     an entry says so: smn_recursion (k0_d and both outputs 16-byte aligned, ldk0 and ldk multiples of 16 bytes:
 *     SMN_EINVAL otherwise), smn_spr_kinv (ldkinv a multiple of 16 bytes), and smn_cholesky, which factors in place
 *     when n_total and n_factor are multiples of 128, a_d is 16-byte aligned and lda a multiple of 16 bytes, and
 *     through a padded copy otherwise (same contract, another schedule: not the same bits).
 *   - "d" pointers are DEVICE pointers obtained from smn_malloc(); "h" pointers are host memory
 *     borrowed for the duration of the call.  dtype: SMN_F32 / SMN_F64.
 *   - calls are stream-ordered on the context's stream; functions that return host scalars
 *     synchronise that stream.  A context is not thread-safe.
 *   - numerical failure is NOT an error status: a non-positive pivot is reported through *info
 *     (1-based index of the first bad pivot, 0 = fine) and the dependent outputs are NaN, which is
 *     what the reference's JAX Cholesky does (silent NaN, experiments/regression/train.py:211).
 */
#ifndef SMNNGP_H
#define SMNNGP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct smn_ctx smn_ctx;

enum { SMN_OK = 0, SMN_EINVAL = -1, SMN_EHIP = -2, SMN_ENOMEM = -3, SMN_ENOTSUP = -4, SMN_ECOMM = -5 };
enum { SMN_F32 = 0, SMN_F64 = 1 };
enum { SMN_ACT_RELU = 0, SMN_ACT_ERF = 1 };            /* experiments/nt_kernels.py:12-18           */
enum { SMN_GET_NNGP = 1, SMN_GET_NTK = 2 };            /* kernel_fn(..., get=) bit mask             */
enum { SMN_FILL_FULL = 0, SMN_FILL_LOWER = 1 };        /* symmetric build: mirror or lower triangle */
enum { SMN_NET_MLP = 0, SMN_NET_DENSE_RESNET = 1 };    /* nt_kernels.py:21-31 / :83-103             */
/* SMN_NET_NTK, OR-ed into the `net` argument (SMN_NET_MLP | SMN_NET_NTK, SMN_NET_DENSE_RESNET | SMN_NET_NTK): the model's
 * covariance function is the neural tangent kernel Theta instead of the NNGP kernel K -- a GP (or Student-t process) with
 * K~ = Theta(X,X) + eps I, posterior mean Theta_td Theta~^-1 y and covariance Theta_tt - Theta_td Theta~^-1 Theta_dt.  (This is
 * not neural_tangents' get="ntk" ensemble covariance, which mixes K and Theta; the two means coincide.)  The gradient entries
 * then differentiate Theta (csrc/grad.hip).  Entries that take the flag:
 *   smn_spr_loss, smn_spr_loss_multi, smn_spr_predict,
 *   smn_spr_loss_grad, smn_spr_loss_grad_multi, smn_lml_grad_terms, smn_lml_grad_terms_multi,
 *   smn_spr_loo_grad (one entry for every c), smn_spr_kinv.
 * With the flag smn_spr_loss neither reads nor writes its Gram cache.  The batched and grid entries (smn_spr_loss_batch,
 * smn_spr_predict_batch, smn_spr_loss_grad_batch) return SMN_ENOTSUP with it; every other entry, and any other bit in `net`,
 * SMN_EINVAL naming the value. */
enum { SMN_NET_NTK = 0x100 };

/* ---- context, errors, memory (JAX array semantics: the spax modules never manage memory themselves) ---- */
int smn_version(void);
int smn_device_count(int* n);
int smn_ctx_create(int device_id, smn_ctx** out);
int smn_ctx_destroy(smn_ctx* ctx);
int smn_last_error(smn_ctx* ctx, char* buf, size_t n);
int smn_synchronize(smn_ctx* ctx);
int smn_malloc(smn_ctx* ctx, size_t bytes, void** dptr);
int smn_free(smn_ctx* ctx, void* dptr);
int smn_memset(smn_ctx* ctx, void* dptr, int value, size_t bytes);
int smn_memcpy_h2d(smn_ctx* ctx, void* dst_d, const void* src_h, size_t bytes);
int smn_memcpy_d2h(smn_ctx* ctx, void* dst_h, const void* src_d, size_t bytes);
int smn_memcpy_d2d(smn_ctx* ctx, void* dst_d, const void* src_d, size_t bytes);
/* 2-D copies (row pitch in bytes) used to move unpadded host matrices into padded device ones */
int smn_memcpy2d_h2d(smn_ctx* ctx, void* dst_d, size_t dpitch, const void* src_h, size_t spitch,
                     size_t width_bytes, size_t rows);
int smn_memcpy2d_d2h(smn_ctx* ctx, void* dst_h, size_t dpitch, const void* src_d, size_t spitch,
                     size_t width_bytes, size_t rows);
/* timing hooks (hipEvents on the context's stream) */
int smn_timer_start(smn_ctx* ctx);
int smn_timer_stop_ms(smn_ctx* ctx, double* ms);           /* synchronises */
/* per-kernel timing: while enabled kernel launches are bracketed by a hipEvent pair on their own
 * stream.  category: 0 prep (pad/tables), 1 fused Gram+recursion build, 2 stand-alone recursion,
 * 3 Cholesky panel, 4 Cholesky strip update, 5 Cholesky trailing update, 6 other (scatter of gathered blocks),
 * 7 all-gathers, 8 the wait of the main stream for the FIRST piece of a column-first exchange (its exposed part),
 * 9 later waits of the factorisation for pieces the first panel chain did not cover (stalls).
 * on: 0 off; 1 every category; (2 << c) only category c (values add up to a mask).  An event pair
 * costs a few microseconds of queue time per launch, so timing ONE category perturbs a step far less
 * than timing all ~280 launches of it. */
int smn_profile_enable(smn_ctx* ctx, int on);
int smn_profile_read(smn_ctx* ctx, int category, double* total_ms, int* launches);
/* MFMA flops the launches of a category have EXECUTED since the last smn_profile_enable (whole 128x128 tiles, counted
 * on the host as they are issued): 4 strip updates, 5 trailing updates.  What a roofline
 * fraction of those kernels is priced with. */
int smn_profile_flops(smn_ctx* ctx, int category, double* flops);

/* ---- NNGP / NTK kernel build ----
 * Replaces kernel_fn(x1, x2, get) produced by get_mlp_kernel / get_dense_resnet_kernel
 * (experiments/nt_kernels.py:21-31, :83-103; called from spax/kernels.py:23-27 and
 * experiments/regression/find.py:64-70): K0 = x1 x2^T / d on MFMA, then num_hiddens x
 * [Dense(w_std,b_std); act] and Dense(last_w_std, b=0) fused into the GEMM epilogue.
 *   x1_d [n1,d] ld=ldx1; x2_d [n2,d] or NULL (symmetric: x2 = x1, fill selects mirror/lower).
 *   get_mask: SMN_GET_NNGP | SMN_GET_NTK; nngp_d [n1,n2] ld=ldk (may be NULL if not requested),
 *   ntk_d likewise. */
int smn_kernel_mlp(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens,
                   double w_std, double b_std, double last_w_std,
                   const void* x1_d, int64_t n1, int64_t ldx1,
                   const void* x2_d, int64_t n2, int64_t ldx2, int64_t d,
                   int get_mask, int fill,
                   void* nngp_d, void* ntk_d, int64_t ldk);

/* Row-sharded variant (multi-GPU build): computes rows [row_begin,row_end)
 * of the symmetric kernel of x_d against all n columns into out_d [(row_end-row_begin), n]. */
int smn_kernel_mlp_rows(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens,
                        double w_std, double b_std, double last_w_std,
                        const void* x_d, int64_t n, int64_t ldx, int64_t d,
                        int64_t row_begin, int64_t row_end, int get_mask,
                        void* nngp_rows_d, void* ntk_rows_d, int64_t ldk);

/* Balanced symmetric shard: rows [row_begin,row_end) x columns [0,row_end) only (the lower
 * trapezoid of that row block; 128x128 tiles wholly above the diagonal are skipped and what lies
 * right of the diagonal inside the written range is unspecified except that the diagonal itself is
 * exact).  out_d [(row_end-row_begin), >= row_end] with ld = ldk; see smn_unpack_lower_blocks. */
int smn_kernel_mlp_lower_rows(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens,
                              double w_std, double b_std, double last_w_std,
                              const void* x_d, int64_t n, int64_t ldx, int64_t d,
                              int64_t row_begin, int64_t row_end, int get_mask,
                              void* nngp_rows_d, void* ntk_rows_d, int64_t ldk);

/* One rank's whole share of the paired layout in ONE launch: the lower trapezoids of row blocks
 * `rank` and 2*nranks-1-rank (block_rows rows each, a multiple of 128), packed into
 * nngp_chunk_d / ntk_chunk_d [block_rows^2 * (2*nranks+1)] exactly as smn_unpack_lower_blocks
 * expects them after the all-gather. */
int smn_kernel_mlp_shard(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens,
                         double w_std, double b_std, double last_w_std,
                         const void* x_d, int64_t n, int64_t ldx, int64_t d,
                         int nranks, int rank, int64_t block_rows, int get_mask,
                         void* nngp_chunk_d, void* ntk_chunk_d);

/* The two halves of the build, exposed separately for sweeps that reuse K0 across (w_std,b_std)
 * (experiments/regression/find.py:134-138) and for roofline measurement of the recursion alone.
 * smn_gram: k0_d = x1 x2^T / d (+ q1_d [n1], q2_d [n2] diagonals ||x||^2/d).
 * smn_recursion: applies the layer stack elementwise to k0 (HBM-streaming kernel, 16-byte vector accesses: k0_d, nngp_d and
 *   ntk_d must be 16-byte aligned and ldk0, ldk multiples of 16 bytes; SMN_EINVAL otherwise). */
int smn_gram(smn_ctx* ctx, int dtype, const void* x1_d, int64_t n1, int64_t ldx1,
             const void* x2_d, int64_t n2, int64_t ldx2, int64_t d,
             void* k0_d, int64_t ldk, void* q1_d, void* q2_d);
int smn_recursion(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens,
                  double w_std, double b_std, double last_w_std,
                  const void* k0_d, int64_t n1, int64_t n2, int64_t ldk0,
                  const void* q1_d, const void* q2_d, int symmetric, int get_mask,
                  void* nngp_d, void* ntk_d, int64_t ldk);

/* conv-NNGP (experiments/nt_kernels.py:34-45): x [n,H,W,C] NHWC, 3x3 SAME stride 1, Flatten, Dense. */
int smn_kernel_cnn(smn_ctx* ctx, int dtype, int act, int num_hiddens,
                   double w_std, double b_std, double last_w_std,
                   const void* x1_d, int64_t n1, const void* x2_d, int64_t n2,
                   int64_t H, int64_t W, int64_t C, int fill, void* nngp_d, int64_t ldk);

/* Conv-ResNet NNGP kernel: experiments/nt_kernels.py:48-80 get_conv_resnet_kernel = WideResnet(block_size, k=1)
 * without pooling: Conv; four groups of block_size residual blocks (strides 1,2,2,2; Conv shortcut in the first
 * block of a group, Identity after; main path act, Conv(stride), act, Conv); Flatten; Dense(last_w_std).
 * Same argument meaning as smn_kernel_cnn; H and W must be multiples of 8; block_size <= 6. */
int smn_kernel_conv_resnet(smn_ctx* ctx, int dtype, int act, int block_size,
                           double w_std, double b_std, double last_w_std,
                           const void* x1_d, int64_t n1, const void* x2_d, int64_t n2,
                           int64_t H, int64_t W, int64_t C, int fill, void* nngp_d, int64_t ldk);

/* conv-NNGP with global average pooling in front of the read-out:
 *   num_hiddens x [stax.Conv(1, (3,3), padding SAME, W_std=w_std, b_std=b_std); act];  stax.GlobalAvgPool();
 *   stax.Dense(num_class, W_std=last_w_std, b_std=0)
 * -- get_cnn_kernel with stax.Flatten replaced by stax.GlobalAvgPool (the stax.AvgPool left commented out at
 * experiments/nt_kernels.py:75).  The read-out averages the covariance of every pixel p of x1[n] with every pixel q of x2[m]:
 *   K0[p,q] = sum_c x1[n,p,c] x2[m,q,c] / C;   per layer K~[p,q] = w_std^2/9 sum_{d in 3x3} K[p+d,q+d] + b_std^2 (terms outside
 *   either image are 0), K[p,q] = act(K~[p,q]; K~_nn[p,p], K~_mm[q,q]);   nngp[n,m] = last_w_std^2 sum_{p,q} K[p,q] / (H W)^2
 * -- (H W)^2 entries per pair and layer where smn_kernel_cnn has H W.  num_hiddens == 0: last_w_std^2 (mean_p x1[n,p]) .
 * (mean_q x2[m,q]) / C.
 * smn_kernel_cnn_pool: same argument meaning and validation as smn_kernel_cnn (x2_d == NULL: the symmetric build, pairs m <= n,
 *   mirrored under SMN_FILL_FULL; SMN_FILL_LOWER leaves the strict upper triangle and everything past the row's n2 entries
 *   untouched).  Null ctx / x1_d / nngp_d, n < 1, ldk < n2 and a bad act, dtype or fill: SMN_EINVAL, by name.
 *   Limit: H*W <= SMN_CNN_POOL_MAX_PIXELS whatever the aspect ratio (1 x 1024 included); larger images return SMN_ENOTSUP with a
 *   message naming the limit.  b_std == 0 and all-zero neighbourhoods give finite values (a zero-variance pixel contributes 0
 *   under ReLU).  Per-entry arithmetic in `dtype`; every sum over pixels and offsets in fp64, in an order fixed by (H, W): no
 *   floating-point atomics, and the bits of nngp[n,m] depend on the two images, the hyper-parameters and (H, W, C) alone -- not
 *   on n1, n2, fill, ldk, the pair's position, or the number of passes the pair list is cut into when its partial sums exceed the
 *   workspace budget (256 MB, or smn_debug_batch_bytes if smaller).  The diagonal pair (n, n) of a symmetric build takes its
 *   same-pixel entries K[p,p] from the per-image variance recursion, as smn_kernel_cnn takes its diagonal.  No synchronisation.
 * smn_kernel_cnn_pool_diag: diag_d[i] = nngp[i,i] of the symmetric build, i < n, bit for bit, without the other pairs. */
#define SMN_CNN_POOL_MAX_PIXELS 1024
int smn_kernel_cnn_pool(smn_ctx* ctx, int dtype, int act, int num_hiddens,
                        double w_std, double b_std, double last_w_std,
                        const void* x1_d, int64_t n1, const void* x2_d, int64_t n2,
                        int64_t H, int64_t W, int64_t C, int fill, void* nngp_d, int64_t ldk);
int smn_kernel_cnn_pool_diag(smn_ctx* ctx, int dtype, int act, int num_hiddens,
                             double w_std, double b_std, double last_w_std,
                             const void* x_d, int64_t n, int64_t H, int64_t W, int64_t C, void* diag_d);

/* ---- factorisation and solves ----
 * smn_cholesky: in-place lower Cholesky of the leading n_factor x n_factor block of the symmetric
 * matrix a_d [n_total,n_total] (lower triangle read/written), carried through the remaining
 * n_total-n_factor rows: on return rows >= n_factor hold B L^-T in their first n_factor columns
 * and the Schur complement C - B A^-1 B^T in the trailing block (lower triangle).  With
 * n_total == n_factor this is a plain potrf.  Before factoring, jitter_abs + ridge_rel*tr(A)/n
 * is added to the first n_shift diagonal entries: jitter_abs is spax/utils.py:26-27 +
 * spax/models.py:96 (absolute), ridge_rel is neural_tangents' diag_reg scaling used by
 * spax/kernels.py:29-32 (trace taken over those n_shift entries).
 * Replaces lax.linalg.cholesky + triangular_solve (spax/utils.py:179-180), the Cholesky inside
 * jax.scipy.stats.multivariate_normal.logpdf (spax/likelihoods.py:27) and cho_factor/cho_solve
 * inside gradient_descent_mse_ensemble.  *logdet_h = 2 sum log L_ii over n_factor columns. */
int smn_cholesky(smn_ctx* ctx, int dtype, void* a_d, int64_t n_total, int64_t n_factor, int64_t lda,
                 int64_t n_shift, double jitter_abs, double ridge_rel, int* info_h, double* logdet_h);

/* X = op(L)^-1 B in place, B [n,nrhs] row-major ld=ldb, L lower [n,n]; trans=0: L, 1: L^T.
 * (lax.linalg.triangular_solve, spax/utils.py:180.) */
int smn_trsm(smn_ctx* ctx, int dtype, const void* l_d, int64_t n, int64_t ldl,
             void* b_d, int64_t nrhs, int64_t ldb, int trans);
/* dst_d[c, r] = src_d[r, c] for r < rows, c < cols (row-major, leading dimensions in elements; no overlap).  The NTK
 * posterior of gradient_descent_mse_ensemble (sample.ipynb:194-195) needs Theta~^-1 Theta_dt as a left operand. */
int smn_transpose(smn_ctx* ctx, int dtype, void* dst_d, int64_t ldd, const void* src_d, int64_t lds, int64_t rows,
                  int64_t cols);

/* smn_eigh_pd: eigendecomposition A = V diag(w) V^T of a symmetric POSITIVE DEFINITE matrix a_d [n,n] (lower triangle read,
 * ld = lda, not modified).  Replaces jnp.linalg.eigh inside neural_tangents.predict.gradient_descent_mse_ensemble
 * (predict_fn(t=...), reached from spax/kernels.py:29-32) and inside neural_tangents.predict.max_learning_rate.
 * w_d [n]: eigenvalues, ascending, in dtype.  v_d [n,n] ld = ldv: v_d[i*ldv + k] = component i of eigenvector k.
 * Method: the project's Cholesky factorisation, then one-sided Jacobi on the factor in fp64 (csrc/eigh.hip); the host
 * reads one convergence word per sweep.  Two calls on the same input return the same bits.
 * *info_h: 0 converged; k > 0: not positive definite (the factorisation's failing pivot, 1-based), w and v are NaN;
 * -1: not converged within max_sweeps (results still written).  max_sweeps <= 0 means 30 (at most 1000).
 * *sweeps_h (may be NULL): sweeps taken.  Workspace (kept by the context): the padded factor (round_up(n,128)^2 elements),
 * the fp64 working matrix (n^2 doubles) and V^T (n^2 elements): about 3 n^2 elements in fp64, 4 n^2 in fp32. */
int smn_eigh_pd(smn_ctx* ctx, int dtype, const void* a_d, int64_t n, int64_t lda, void* w_d, void* v_d, int64_t ldv,
                int max_sweeps, int* info_h, int* sweeps_h);

/* smn_predict_gd: mean and covariance of the infinite ensemble after gradient-flow time t on the MSE loss
 * (neural_tangents.predict.gradient_descent_mse_ensemble, predict_fn(t=...); sample.ipynb:194-195 is the t = None form).
 * k_joint_d / theta_joint_d: NNGP / NTK kernels of [x_train; x_test], [n+t, n+t] ld = ld, lower triangles read, neither
 * modified; theta_joint_d NULL selects get="nngp" (G = K), otherwise get="ntk" (G = Theta).  y_d [n,c] row-major.
 *   G~ = G_dd + (diag_abs + diag_rel tr(G_dd)/n) I = V diag(lambda) V^T (smn_eigh_pd's solver), lambda clamped at 0,
 *   s = learning_rate * time / (n c),  d = -expm1(-lambda s)/lambda,  e = -expm1(-2 lambda s)/lambda  (time = +inf: 1/lambda),
 *   P = G_*d V,  mean = (P.d) V^T y,  nngp: cov = K_** - (P.e) P^T,
 *   ntk: A = (P.d) V^T, cov = K_** + A K_dd A^T - (A K_d* + K_*d A^T)   (K_dd without the ridge).
 * times_h [nt] host, each >= 0 or +inf.  mean_d [nt,t,c]; cov_d [nt,t,ldc] (ldc >= t; NULL: mean only), symmetric to
 * the bit; evals_d [n] (may be NULL) receives lambda.  The products that do not depend on the time are formed once.
 * *info_h: smn_eigh_pd's; != 0 gives NaN results and SMN_OK. */
int smn_predict_gd(smn_ctx* ctx, int dtype, const void* k_joint_d, const void* theta_joint_d, int64_t n, int64_t t,
                   int64_t ld, const void* y_d, int64_t c, double diag_rel, double diag_abs, const double* times_h,
                   int64_t nt, double learning_rate, void* mean_d, void* cov_d, int64_t ldc, void* evals_d,
                   int* info_h);

/* ---- likelihood heads (host scalars out) ----
 * smn_lml: log-marginal likelihood of y_d [n] under cov = K + eps I, K given as k_d [n,n] lower
 * (destroyed: overwritten by its factor).  df <= 0: Gaussian (spax/likelihoods.py:25-28);
 * df > 0: multivariate Student-t with shape = scale*cov, df = 2a, scale = b/a
 * (spax/likelihoods.py:45-50, spax/utils.py:178-183).  NaN + info>0 when not PD. */
int smn_lml(smn_ctx* ctx, int dtype, void* k_d, int64_t n, int64_t ldk, const void* y_d,
            double eps_abs, double df, double scale, double* logpdf_h, double* quad_h,
            double* logdet_h, int* info_h);

/* smn_predict: t=infinity NNGP posterior (spax/kernels.py:29-32 -> neural_tangents
 * gradient_descent_mse_ensemble).  kj_d is the JOINT kernel of [x_train; x_test] ([n+t, n+t],
 * lower triangle, destroyed).  y_d [n,c] row-major.  mean_d [t,c], cov_d [t,t] (full, symmetric).
 * ridge_rel = diag_reg (relative: * tr(K_dd)/n); ridge_abs adds an absolute term.
 * quad_h (may be NULL) receives y_k^T K~^-1 y_k for each output column k. */
int smn_predict(smn_ctx* ctx, int dtype, void* kj_d, int64_t n, int64_t t, int64_t ldk,
                const void* y_d, int64_t c, double ridge_rel, double ridge_abs,
                void* mean_d, void* cov_d, int64_t ldcov, double* quad_h, double* logdet_h, int* info_h);

/* ---- fused model-level calls (what the spax facade uses; nothing leaves the GPU but scalars) ----
 * smn_spr_loss: SPR.loss (spax/models.py:93-98): builds K(x,x) straight into the factorisation
 * workspace, adds eps_abs, factors, and returns the log-pdf of y (Gaussian df<=0 / Student-t).
 *
 * Gram cache.  The input Gram x x^T depends on x alone -- net, activation, depth, w_std, b_std, last_w_std, eps, df, scale and
 * y all enter after it -- and a training loop calls this with the same x thousands of times.  From 2560 padded rows on the
 * context therefore keeps its own padded copy of x and, from the second call on one x, the raw MFMA accumulators of the lower
 * 128x128 tiles of x x^T; later calls run the layer recursion over those instead of the matrix product.  Whether x is
 * unchanged is decided by CONTENT on every call, never by pointer: the padding pass compares all of x with the copy bit for
 * bit (NaN and signed zeros included), so freeing and re-allocating x, or overwriting it in place, is seen.  The results are
 * bit-identical to a call without the cache (same accumulators, same epilogue code).  The memory belongs to the context
 * (freed by smn_ctx_destroy): copy + accumulators are 0.75 GB at n = 16384, d = 3072 in fp32 and 2.6 GB at n = 32768; above
 * 8 GiB, or when the allocation fails, the call runs without the cache -- it never fails because of it.  Other entry points
 * neither read nor write the cache. */
int smn_spr_loss(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens,
                 double w_std, double b_std, double last_w_std,
                 const void* x_d, int64_t n, int64_t ldx, int64_t d, const void* y_d,
                 double eps_abs, double df, double scale,
                 double* logpdf_h, double* quad_h, double* logdet_h, int* info_h);
/* smn_spr_predict: NNGPKernel.predict (spax/kernels.py:29-32) from the raw inputs: joint kernel of
 * [x; x_test], relative/absolute ridge on the training block, posterior mean [t,c] and cov [t,t]. */
int smn_spr_predict(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens,
                    double w_std, double b_std, double last_w_std,
                    const void* x_d, int64_t n, int64_t ldx, const void* xt_d, int64_t t, int64_t ldxt,
                    int64_t d, const void* y_d, int64_t c, double ridge_rel, double ridge_abs,
                    void* mean_d, void* cov_d, int64_t ldcov,
                    double* quad_h, double* logdet_h, int* info_h);

/* ---- fit once, predict many: a device-resident posterior (csrc/fit.hip) ----
 * Every entry above refactors the training kernel for each prediction.  A fitted state keeps the Cholesky factor L of
 * K~ = K_dd + (ridge_abs + ridge_rel tr(K_dd) / n) I -- the posterior of smn_spr_predict -- and beta^T = Y^T L^-T, and answers
 * prediction calls of any size t >= 1 at O(n^2 t): chunks of at most `capacity` test rows go through the cross kernel (written
 * straight into the state), one triangular solve and one read-out pass (mean = V^T beta, var = k_tt - |L^-1 k|^2, fp64 sums in
 * a fixed order: the same arguments give the same bits).  The state owns its memory ([n_pad + round_up(capacity, 128) + 128]^2
 * elements plus, in the fused form, a padded copy of x), uses no workspace slot of the context between calls, and is immutable:
 * later changes to x_d, y_d or the hyper-parameters do not reach it.  dtype is fixed at creation; 1 <= c <= 48 (SMN_ENOTSUP
 * above); capacity >= 1.
 *   smn_fit_create              fused form (SMN_NET_MLP / SMN_NET_DENSE_RESNET, optionally | SMN_NET_NTK: the GP of Theta);
 *                               y_d [n, c] row-major; quad_h [c], logdet_h, info_h (any may be NULL) as smn_spr_predict.
 *   smn_fit_create_from_kernel  matrix form: k_d [n, n] lower, NOT modified.
 *   smn_fit_predict             fused states: xt_d [t, ldxt] -> mean_d [t, c], var_d [t] and / or cov_d [t, ldcov] (full,
 *                               symmetric); var_d and cov_d may be NULL.  cov_d needs t <= capacity (SMN_EINVAL otherwise:
 *                               the Schur block K_tt - V^T V sits behind the factor); the diagonal path never forms a t x t
 *                               object.  No host synchronisation once the context's workspace has reached the call's size (the first
 *                               call of a shape grows it, before anything is launched).
 *   smn_fit_apply               either kind of state, the caller supplies k_td_d [t, n] and ktt_diag_d [t] and / or k_tt_d
 *                               [t, t] (lower): var_d needs one of the two (the diagonal is taken from ktt_diag_d when both are
 *                               given), cov_d needs k_tt_d.
 *   smn_fit_predict_grad        fused states only (matrix form: SMN_EINVAL as smn_fit_predict): the derivatives of what
 *                               smn_fit_predict returns with respect to the test inputs, dmean_d [t, c, d] = d mean[r, k] / d x_r
 *                               and / or dvar_d [t, d] = d var[r] / d x_r (one may be NULL), in chunks of `capacity` rows.  The
 *                               kernel-side derivative is smn_kernel_mlp_input_grad's; the first call adds L' = J L^T J, alpha =
 *                               K~^-1 Y and X^T to the state (smn_fit_info's bytes grow); nothing smn_fit_predict or smn_fit_apply
 *                               reads changes.  A call also takes context workspace (freed with the context, not counted by
 *                               smn_fit_info): F_1, F_2, their seeded product and U, 4 x round_up(min(capacity, t), 128) x n_pad
 *                               elements -- 0.54 GB in fp32 at n = 16384, capacity 2048.  Sums in fp64 and in a fixed order: the same arguments give the same bits, and a
 *                               row's values do not depend on the rows it shares a call with.  info != 0 -> NaN outputs, SMN_OK.
 *   smn_fit_weights             either kind of state: the solve behind those gradients for a cross kernel of the caller's, u_d
 *                               [t, ldu >= n] = K_td K~^-1 from k_td_d [t, ldk >= n] (the two forward sweeps, on L and on L' =
 *                               J L^T J; 1 <= t <= capacity per call) and / or alpha_d [n, c] row-major = K~^-1 Y; either output
 *                               may be NULL.  With smn_kernel_cnn_input_grad_cross these are jax.grad of the predictive of
 *                               experiments/nt_kernels.py:34-45 with respect to the test images.  The first call adds L' and
 *                               alpha to the state (smn_fit_info's bytes grow; a matrix-form state adds no X^T);
 *                               smn_fit_reserve, the appends and smn_fit_remove drop and rebuild them as for
 *                               smn_fit_predict_grad; nothing smn_fit_predict or smn_fit_apply reads changes.  info != 0 ->
 *                               NaN outputs, SMN_OK.  No synchronisation.
 *   smn_fit_info                sizes and the bytes the state owns (NULL outputs are skipped).
 *   smn_fit_destroy             synchronises the context's stream and frees the state.
 * Not positive definite: *info_h = the failing pivot, the state is still returned (SMN_OK) and every prediction from it is NaN.
 * A state must be destroyed before its context; using it after smn_fit_destroy is undefined. */
typedef struct smn_fit smn_fit;
int smn_fit_create(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens,
                   double w_std, double b_std, double last_w_std,
                   const void* x_d, int64_t n, int64_t ldx, int64_t d, const void* y_d, int64_t c,
                   double ridge_rel, double ridge_abs, int64_t capacity,
                   smn_fit** out, double* quad_h, double* logdet_h, int* info_h);
int smn_fit_create_from_kernel(smn_ctx* ctx, int dtype, const void* k_d, int64_t n, int64_t ldk, const void* y_d, int64_t c,
                               double ridge_rel, double ridge_abs, int64_t capacity,
                               smn_fit** out, double* quad_h, double* logdet_h, int* info_h);
int smn_fit_predict(smn_fit* fit, const void* xt_d, int64_t t, int64_t ldxt, void* mean_d, void* var_d, void* cov_d, int64_t ldcov);
int smn_fit_apply(smn_fit* fit, const void* k_td_d, int64_t t, int64_t ldk, const void* ktt_diag_d, const void* k_tt_d, int64_t ldtt,
                  void* mean_d, void* var_d, void* cov_d, int64_t ldcov);
int smn_fit_predict_grad(smn_fit* fit, const void* xt_d, int64_t t, int64_t ldxt, void* dmean_d, void* dvar_d);
int smn_fit_weights(smn_fit* fit, const void* k_td_d, int64_t t, int64_t ldk, void* u_d, int64_t ldu, void* alpha_d);
int smn_fit_info(smn_fit* fit, int64_t* n, int64_t* c, int64_t* capacity, size_t* bytes);
int smn_fit_destroy(smn_fit* fit);

/* ---- appending training points to a fitted state: O(n^2 k + n k^2 + k^3) instead of a refit ----
 * THE FROZEN RIDGE.  A state is made with K~ = K_dd + lambda I, lambda = ridge_abs + ridge_rel tr(K_dd) / n, and lambda is
 * fixed at creation (smn_fit_stats reads it).  Every appended point gets that lambda as an ABSOLUTE ridge: after any sequence of
 * appends the state is the posterior of all N = n0 + sum k points under K(X, X) + lambda I -- what smn_fit_create on all the
 * points with ridge_rel = 0, ridge_abs = lambda gives, NOT the fit whose relative ridge is recomputed at the new N (the two
 * coincide when the kernel's diagonal is constant).  For new points x+ [k, d], y+ [k, c] and the factor L (n x n):
 *     V = K(x+, X) L^-T,  S = K(x+, x+) + lambda I - V V^T,  L22 = chol(S),  z = L22^-1 (y+ - V beta)
 *     L <- [[L, 0], [V, L22]],  beta <- [beta; z],  logdet += 2 sum log diag L22,  quad_c += |z_c|^2
 * The new rows take the place of the identity padding behind row n; V is solved and S formed where a cov = full prediction
 * forms them, one splice pass streams each V_i once (into row n + i of L, and into the residual y+ - V beta with the read-out's
 * own fp64 sums), and S is factored in place by the creation path on that window.
 *   smn_fit_reserve             room for max_points training rows: n_pad becomes round_up(max_points, 128); the matrix, the
 *                               padded x copy are reallocated and the factor, the beta rows and x copied (O(n^2); peak memory
 *                               = old + new state), identity on the new rows' diagonal.  What smn_fit_predict_grad added is
 *                               dropped and made again by its next call.  max_points within the current room: nothing happens,
 *                               no bit of the state moves; max_points < n: SMN_EINVAL.  A reserved state predicts at once, at
 *                               the per-call cost of the new n_pad; the read-out's sums run over n_pad columns, so their order
 *                               and with it the last bits may differ from the unreserved state's.
 *   smn_fit_append              fused states: x_new_d [k, ldx], y_new_d [k, c].  quad_h [c], logdet_h: the updated totals;
 *                               any of the three outputs may be NULL.
 *   smn_fit_append_from_kernel  matrix-form states (a fused state keeps its own x: SMN_ENOTSUP): k_nd_d [k, n] = K(x+, X)
 *                               against the state's n rows (n != the state's: SMN_EINVAL), k_nn_d [k, k] = K(x+, x+), lower.
 * Both: a state without room for n + k rows grows itself as smn_fit_reserve(max(n + k, n + n / 2)) would.  k > capacity goes
 * through in chunks of `capacity` rows, in order, each seeing the earlier ones as training rows.  A chunk whose S is not
 * positive definite leaves the state exactly as it was before that chunk -- the earlier chunks stay in --, *info_h is the
 * 1-based index among all training rows of the failing pivot and the entry returns SMN_OK (smn_fit_info tells how many rows the
 * state holds).  A state whose own info != 0 takes no rows (SMN_EINVAL).  One host synchronisation per chunk (info).
 *   smn_fit_stats               max_points (the room, n_pad), lambda, quad [c] and logdet as they stand (NULLs are skipped). */
int smn_fit_reserve(smn_fit* fit, int64_t max_points);
int smn_fit_append(smn_fit* fit, const void* x_new_d, int64_t k, int64_t ldx, const void* y_new_d,
                   double* quad_h, double* logdet_h, int* info_h);
int smn_fit_append_from_kernel(smn_fit* fit, const void* k_nd_d, int64_t k, int64_t n, int64_t ldk, const void* k_nn_d, int64_t ldnn,
                               const void* y_new_d, double* quad_h, double* logdet_h, int* info_h);
int smn_fit_stats(smn_fit* fit, int64_t* max_points, double* ridge, double* quad_h, double* logdet_h);

/* ---- removing training points from a fitted state: O(n^2 k) instead of a refit (csrc/fit_remove.hip) ----
 * No hyperbolic downdate: an orthogonal triangularisation, backward stable, which cannot fail for lack of positive definiteness.
 * With L (n x n, lower), L L^T = K~ = K(X, X) + lambda I, beta^T = Y^T L^-T, J the k removed rows, R the kept ones in their order
 * and H = L[R, :] ((n - k) x n): H H^T = K~_RR and Y_R = H beta.  For any orthogonal Q with H Q = [L' 0], L' lower triangular
 * with a positive diagonal,
 *     [ H      ]       [ L'       0     ]      L' L'^T = K(X_R, X_R) + lambda I,   beta' = L'^-1 Y_R,   rho is discarded.
 *     [ beta^T ] Q  =  [ beta'^T  rho^T ]
 * THE FROZEN RIDGE holds as for an append: lambda is unchanged and absolute, so after a removal the state is the posterior of the
 * kept points under K + lambda I -- what smn_fit_create on the kept points with ridge_rel = 0, ridge_abs = lambda gives.
 * Only the tail moves: columns left of j1 = min J and rows above it are untouched; behind it new row i ends at column i + r(i)
 * (r(i) <= k removed rows above it), and the band is reduced in steps of b = 64 rows: the LQ factorisation of a b x (b + KMAX)
 * block in fp64 (both dtypes; sign flips folded in so that diag L' > 0, exact zeros where the block becomes zero), then the rows
 * below -- the beta rows among them -- times Q_s on the MFMA tile engine in the state's dtype; two launches per step, no host
 * synchronisation inside the sweep.  KMAX = 32 rows per pass; more rows go in passes of KMAX from the highest indices down, each
 * a complete removal.  J = exactly the last k rows (any k) touches no entry of L: the rows become identity padding, the beta
 * columns are cleared -- the exact undo of smn_fit_append.  quad [c] = sum beta'^2 and logdet = 2 sum log diag L' are recomputed
 * over the new state in fp64 in a fixed order (one host synchronisation, at the end); the same removal on the same state gives
 * the same bits.  Workspace: the sweep runs in context workspace (freed with the context, not counted by smn_fit_info):
 * (MB + 192) x (MB + 64) elements, MB = round_up(n - k - floor(j1 / 64) 64, 64) -- at most about the factor's own size, 1.07 GB
 * in fp32 at n = 16384 when row 0 goes.  The state's n_pad, capacity and allocation stay as they are; the freed rows are
 * identity padding again, and (fused states) the padded x copy is compacted.  What smn_fit_predict_grad keeps beside the factor
 * is made again by its next call.
 *   smn_fit_remove              idx_h: k distinct 0-based row indices on the HOST, any order; fused and matrix-form states.  Rows
 *                               behind a removed one move down by one index each.  SMN_EINVAL, naming the value, with nothing
 *                               moved and nothing launched: k < 1, k >= n (a state keeps at least one point), an index outside
 *                               [0, n), an index given twice, a state whose own info != 0.  quad_h, logdet_h may be NULL. */
int smn_fit_remove(smn_fit* fit, const int64_t* idx_h, int64_t k, double* quad_h, double* logdet_h);

/* ---- batched small problems: G evaluations on ONE data set in one sequence of launches (grid.y = G) ----
 * The reference's real workloads are small and many: experiments/regression/find.py:134-199 factors the kernel of one data
 * set 2 x 99 times under a grid of (w_std, b_std, eps), train.py:178-212 takes thousands of steps at N = 245, where one
 * SPR.loss occupies two workgroups of a 256-CU chip.  These calls run nprob problems of identical shape -- same x, y, net,
 * act and depth; per-problem w_std[], b_std[], last_w_std[] and diagonal shift (host arrays of nprob doubles) -- through
 * the fused build, the factorisation and the read-out together; each problem's result is bit-identical to the serial call.
 *   smn_spr_loss_batch     nprob x smn_spr_loss: eps_abs[], df[] (NULL: Gaussian), scale[] -> logpdf_h[], quad_h[], logdet_h[],
 *                          info_h[] (any output may be NULL)
 *   smn_spr_predict_batch  nprob x smn_spr_predict: ridge_rel[], ridge_abs[] (NULL: 0) -> mean_d [nprob,t,c], cov_d
 *                          [nprob,t,ldcov] and / or var_d [nprob,t] = diag(cov) (what find.py:50-55 uses; either may be
 *                          NULL), quad_h [nprob,c], logdet_h[], info_h[]
 * Batches whose workspaces (nprob x (n_pad + (t+c)_pad)^2 elements) exceed 48 GB run in chunks (smn_debug_batch_bytes: test
 * hook that sets that budget). */
int smn_spr_loss_batch(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, int nprob,
                       const double* w_std, const double* b_std, const double* last_w_std,
                       const void* x_d, int64_t n, int64_t ldx, int64_t d, const void* y_d,
                       const double* eps_abs, const double* df, const double* scale,
                       double* logpdf_h, double* quad_h, double* logdet_h, int* info_h);
int smn_debug_batch_bytes(smn_ctx* ctx, size_t bytes);
/* Test hook: smn_spr_loss under the look-ahead (n_total >= 8192) builds the bottom-right corner of the kernel matrix as a second
 * launch on the bulk stream, beside the first super-panel's panel chain (same tiles, same bits: only the order changes).
 * on = 0 switches that off (one launch, as every other entry point builds). */
int smn_debug_split_build(smn_ctx* ctx, int on);
/* on = 0 above also bypasses the Gram cache of smn_spr_loss (kept, not dropped): "one build launch with the chip to itself".
 * Test hook: smn_debug_gram_cache(ctx, 0) bypasses the cache and frees it; 1 (the default) enables it again, cold.
 * smn_gram_cache_stats: calls served from the cached accumulators (hits), calls that went through the cache and ran the
 * matrix product (misses) since the context was created, and the bytes the cache holds now (any pointer may be NULL). */
int smn_debug_gram_cache(smn_ctx* ctx, int on);
int smn_gram_cache_stats(smn_ctx* ctx, int64_t* hits, int64_t* misses, size_t* bytes);
/* Test hook: a panel workgroup of the factorisation carries up to max_passes groups of rows when there are more groups than CUs
 * (default 4; the later groups ride through the solve alone; same bits).  1 = one group per workgroup. */
int smn_debug_panel_passes(smn_ctx* ctx, int max_passes);
int smn_spr_predict_batch(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, int nprob,
                          const double* w_std, const double* b_std, const double* last_w_std,
                          const void* x_d, int64_t n, int64_t ldx, const void* xt_d, int64_t t, int64_t ldxt,
                          int64_t d, const void* y_d, int64_t c, const double* ridge_rel, const double* ridge_abs,
                          void* mean_d, void* cov_d, int64_t ldcov, void* var_d,
                          double* quad_h, double* logdet_h, int* info_h);

/* ---- predictive NLL under a sampled scale mixture (experiments/regression/find.py:165-187) ----
 * For nprob problems with posterior mean_d / var_d [nprob,t] (normalised units; smn_spr_predict_batch), quad_h / logdet_h [nprob]
 * (smn_spr_loss_batch) and nmix proposals of nsamples sigma^2 draws each (sample_q_h [nmix,nsamples]; ratio_h = prior /
 * proposal density per draw, NULL = 1, which is what find.py:168-169 evaluates to):
 *   tnll_h[p, m] = - mean_t logsumexp_s [ log(w~_s + 1e-24) + log N(y_test_t; mean_t y_std + y_mean, sqrt(q_s var_t) y_std) ]
 * with w~ the self-normalised weights of log p(y_train | q_s) = -(n/2) log 2 pi - logdet/2 - quad/(2 q_s) - (n/2) log q_s.
 * skip_h[p] != 0 (may be NULL): NaN for that problem.  fp64 arithmetic throughout; y_test_h in original units. */
int smn_mixture_nll(smn_ctx* ctx, int dtype, int nprob, int64_t t, const void* mean_d, const void* var_d,
                    const double* quad_h, const double* logdet_h, const int* skip_h, const double* y_test_h,
                    double y_mean, double y_std, int64_t n, int nmix, int nsamples, const double* sample_q_h,
                    const double* ratio_h, double* tnll_h);

/* ---- hyper-parameter gradients of the log-marginal likelihood ----
 * What objax.GradValues(model.loss, vars) supplies to experiments/regression/train.py:61-67.
 * With K~ = K(w_std, b_std, last_w_std) + eps I, alpha = K~^-1 y and G = coef * alpha alpha^T - K~^-1:
 *     terms_h[0..3] = sum_ij G_ij dK~_ij/d{w_std, b_std, last_w_std, eps}      (so d logpdf/d theta = terms/2)
 * smn_lml_grad_terms: the contraction alone.  k0_d [n,n] = X X^T / d and q_d [n] its diagonal (smn_gram),
 *   neg_kinv_d [n,n] = -K~^-1 and alpha_d [n] as smn_predict returns them for K_td = I, K_tt = 0
 *   (covariance = -K~^-1, mean = alpha).  coef = 1 (Gaussian) or (df+n)/((df + quad/scale) scale) (Student-t).
 *   neg_kinv_d is read in its lower triangle and, whole, in the 64 x 64 blocks on the diagonal (entries above the diagonal
 *   inside those blocks carry weight 0 and must be finite); no tile strictly above the block diagonal is touched.
 *   b_std == 0 exactly (MLP / dense ResNet, as the conv entries below): every returned value is finite and terms_h[1] is 0 -- an
 *   all-zero input row has zero variance at every layer, where the ReLU map is not differentiable; such a row contributes
 *   nothing to terms_h[0..2], and its G_ii still counts in terms_h[3].  This holds for every dense gradient entry below.
 * smn_spr_loss_grad: everything from X and y (MLP / dense ResNet kernels): also returns quad = y^T K~^-1 y,
 *   logdet K~ and info, from which the host forms the log-pdf and the derivatives w.r.t. (a, b).
 *   On a non-PD matrix info > 0 and the terms are NaN. */
int smn_lml_grad_terms(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens,
                       double w_std, double b_std, double last_w_std,
                       const void* k0_d, int64_t n, int64_t ldk0, const void* q_d,
                       const void* neg_kinv_d, int64_t ldkinv, const void* alpha_d,
                       double coef, double terms_h[4]);
int smn_spr_loss_grad(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens,
                      double w_std, double b_std, double last_w_std,
                      const void* x_d, int64_t n, int64_t ldx, int64_t d, const void* y_d,
                      double eps_abs, double df, double scale,
                      double* quad_h, double* logdet_h, int* info_h, double terms_h[4]);
/* smn_spr_loss_grad_batch: nprob x smn_spr_loss_grad on ONE data set in one sequence of launches (grid.y = the problem), for
 *   multi-start training and for refining the cells of a grid search: per-problem w_std[], b_std[], last_w_std[], eps_abs[],
 *   df[] (NULL: Gaussian) and scale[] (host arrays of nprob doubles) -> quad_h[], logdet_h[], info_h[] (any may be NULL) and
 *   terms_h [nprob][4].  Problem b returns, bit for bit, what smn_spr_loss_grad returns for its parameters.  X X^T / d is
 *   formed once per call; the nprob joint matrices [[K~, .], [I, 0], [y^T, 0, 0]] lie side by side in the workspace and are
 *   factored together, and the contraction reads -K~^-1 and alpha where the factorisation left them.  A problem that is not
 *   positive definite reports its own info > 0 and NaN quad, logdet and terms; the others are unaffected and the call returns
 *   SMN_OK.  Batches whose workspaces (nprob x (n_pad + (n+1)_pad)^2 elements) exceed the budget of smn_debug_batch_bytes run in
 *   chunks.  From n_pad = 8192 on (the rectangle route of the serial call) the problems run one after another. */
int smn_spr_loss_grad_batch(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, int nprob,
                            const double* w_std, const double* b_std, const double* last_w_std,
                            const void* x_d, int64_t n, int64_t ldx, int64_t d, const void* y_d,
                            const double* eps_abs, const double* df, const double* scale,
                            double* quad_h, double* logdet_h, int* info_h, double* terms_h);

/* ---- the same for the conv-NNGP kernel of smn_kernel_cnn (experiments/nt_kernels.py:34-45) ----
 * What objax.GradValues(model.loss, vars) supplies to experiments/regression/train.py:61-67 when the kernel function is
 * get_cnn_kernel.  terms_h[0..3] as above.  For an image pair the forward-mode state is three H x W maps (K, dK/dw^2, dK/db^2)
 * carried through L x [Conv 3x3 SAME; act] on chip, one wave per pair of the lower triangle; the N^2 H W per-pixel entries are
 * never stored.  x_d [n,H,W,C] row-major.
 * smn_kernel_cnn_grad_terms: the contraction alone, the counterpart of smn_lml_grad_terms: neg_kinv_d [n,n] = -K~^-1 (lower
 *   triangle read) and alpha_d [n] as smn_predict returns them for K_td = I, K_tt = 0; coef as above.
 * smn_spr_cnn_loss_grad: everything from x and y: the forward build of the lower triangle straight into the factorisation
 *   workspace, the factorisation with identity, the contraction; also quad = y^T K~^-1 y, logdet K~ and info.  On a non-PD
 *   matrix info > 0, the terms are NaN and the call returns SMN_OK.
 * Limit: H*W <= SMN_CNN_GRAD_MAX_PIXELS (three maps of 16 pixels per lane live in registers); larger images return
 * SMN_ENOTSUP (smn_kernel_cnn itself goes to 4096 pixels).  b_std == 0 exactly: terms_h[1] is 0 and every value is finite -- a
 * pixel whose 3x3 neighbourhood is all zero has zero variance, where the ReLU map is not differentiable; such pixels
 * contribute no variance-side term. */
#define SMN_CNN_GRAD_MAX_PIXELS 1024
int smn_kernel_cnn_grad_terms(smn_ctx* ctx, int dtype, int act, int num_hiddens,
                              double w_std, double b_std, double last_w_std,
                              const void* x_d, int64_t n, int64_t H, int64_t W, int64_t C,
                              const void* neg_kinv_d, int64_t ldkinv, const void* alpha_d,
                              double coef, double terms_h[4]);
int smn_spr_cnn_loss_grad(smn_ctx* ctx, int dtype, int act, int num_hiddens,
                          double w_std, double b_std, double last_w_std,
                          const void* x_d, int64_t n, int64_t H, int64_t W, int64_t C, const void* y_d,
                          double eps_abs, double df, double scale,
                          double* quad_h, double* logdet_h, int* info_h, double terms_h[4]);

/* ---- C target columns that share one kernel matrix: the exact multi-output GP / Student-t process (MultiSPR) ----
 * A network with C outputs whose last-layer variance carries ONE inverse-gamma scale has a jointly multivariate-t prior over all
 * N C outputs: vec(Y) ~ MVT_{NC}(nu = 2a, 0, s (I_C x K~)), s = b/a, K~ = K + eps I -- not C independent Student-t processes.
 * With y_d [n,c] row-major, A = K~^-1 Y, Q = tr(Y^T K~^-1 Y) and ld = logdet K~:
 *     Gaussian (df <= 0):  log p = -Q/2 - (n c / 2) log 2 pi - (c/2) ld        (the sum of c multivariate_normal.logpdf)
 *     Student-t (df > 0):  the multivariate_t_logpdf of spax/utils.py:160-183 in dimension n c with quadratic form Q / scale
 *                          and log-determinant c ld + n c log scale
 *     d log p / d theta = 1/2 sum_ij G_ij dK~_ij/d theta,   G = coef A A^T - c K~^-1,
 *     coef = 1 (Gaussian) or (df + n c) / ((df + Q/scale) scale) (Student-t)
 * The c columns ride through ONE factorisation as c appended rows Y^T (n_total = n_pad + round_up(n + c, 128) for the gradient
 * entries): K~, its factor, -K~^-1 and the tangent pass over the pairs are shared.  1 <= c <= 48 (the limit smn_predict has);
 * c > 48 returns SMN_ENOTSUP.  At c = 1 every entry returns what its single-column counterpart returns.  A matrix that is
 * not positive definite gives info > 0, NaN outputs and SMN_OK.  None of these entries reads or writes the Gram cache of
 * smn_spr_loss.
 * smn_lml_multi: smn_lml for y_d [n,c]: k_d [n,n] lower (destroyed) -> *logpdf_h (joint), *quad_h = Q, quad_cols_h [c] (may be
 *   NULL) = y_k^T K~^-1 y_k per column, *logdet_h = ld, *info_h.  With smn_kernel_cnn in front: the conv build + joint LML.
 * smn_spr_loss_multi: smn_spr_loss for y_d [n,c]: the fused build of the MLP / dense-ResNet kernel, same outputs.
 * smn_lml_grad_terms_multi / smn_kernel_cnn_grad_terms_multi: the rank-c contraction alone, the counterparts of
 *   smn_lml_grad_terms / smn_kernel_cnn_grad_terms: alpha_d [n,c] row-major = A, neg_kinv_d = -K~^-1;
 *   terms_h[0..3] = sum_ij (coef sum_k A_ik A_jk + c (-K~^-1)_ij) dK~_ij/d{w_std, b_std, last_w_std, eps}.  Per entry (per image
 *   pair) the c-term sum is formed once, behind the layer loop; the sums and the reduction tree are those of the single-column
 *   kernels, so two calls give the same bits.
 * smn_spr_loss_grad_multi / smn_spr_cnn_loss_grad_multi: everything from x and Y, the counterparts of smn_spr_loss_grad /
 *   smn_spr_cnn_loss_grad: *quad_h = Q, quad_cols_h [c] (may be NULL), *logdet_h, *info_h, terms_h[4]; the host forms the
 *   log-pdf and the (a, b) derivatives from them.  The conv entries keep the limit H*W <= SMN_CNN_GRAD_MAX_PIXELS. */
int smn_lml_multi(smn_ctx* ctx, int dtype, void* k_d, int64_t n, int64_t ldk, const void* y_d, int64_t c,
                  double eps_abs, double df, double scale, double* logpdf_h, double* quad_h, double* quad_cols_h,
                  double* logdet_h, int* info_h);
int smn_spr_loss_multi(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens,
                       double w_std, double b_std, double last_w_std,
                       const void* x_d, int64_t n, int64_t ldx, int64_t d, const void* y_d, int64_t c,
                       double eps_abs, double df, double scale,
                       double* logpdf_h, double* quad_h, double* quad_cols_h, double* logdet_h, int* info_h);
int smn_lml_grad_terms_multi(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens,
                             double w_std, double b_std, double last_w_std,
                             const void* k0_d, int64_t n, int64_t ldk0, const void* q_d,
                             const void* neg_kinv_d, int64_t ldkinv, const void* alpha_d, int64_t c,
                             double coef, double terms_h[4]);
int smn_kernel_cnn_grad_terms_multi(smn_ctx* ctx, int dtype, int act, int num_hiddens,
                                    double w_std, double b_std, double last_w_std,
                                    const void* x_d, int64_t n, int64_t H, int64_t W, int64_t C,
                                    const void* neg_kinv_d, int64_t ldkinv, const void* alpha_d, int64_t c,
                                    double coef, double terms_h[4]);
int smn_spr_loss_grad_multi(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens,
                            double w_std, double b_std, double last_w_std,
                            const void* x_d, int64_t n, int64_t ldx, int64_t d, const void* y_d, int64_t c,
                            double eps_abs, double df, double scale,
                            double* quad_h, double* quad_cols_h, double* logdet_h, int* info_h, double terms_h[4]);
int smn_spr_cnn_loss_grad_multi(smn_ctx* ctx, int dtype, int act, int num_hiddens,
                                double w_std, double b_std, double last_w_std,
                                const void* x_d, int64_t n, int64_t H, int64_t W, int64_t C, const void* y_d, int64_t c,
                                double eps_abs, double df, double scale,
                                double* quad_h, double* quad_cols_h, double* logdet_h, int* info_h, double terms_h[4]);

/* ---- leave-one-out cross-validation of the exact models (Rasmussen & Williams 5.4.2; nothing in the reference to mirror: it
 *      selects hyper-parameters on a held-out split, experiments/regression/train.py, find.py) ----
 * Leaving out point i leaves out all c outputs of that point.  With P = K~^-1, A = P Y, p_i = P_ii, Q = sum_ic Y_ic A_ic and
 * e_i = sum_c A_ic^2 / p_i the leave-one-out predictive of point i has mean Y_ic - A_ic / p_i and
 *     Gaussian (df <= 0):  variance 1 / p_i,  log p_i = -(c/2) log 2 pi + (c/2) log p_i - e_i / 2
 *     Student-t (df > 0):  a c-variate t with df + (n-1) c degrees of freedom and shape sigma_i^2 I,
 *                          sigma_i^2 = (df + (Q - e_i) / scale) / (df + (n-1) c) * scale / p_i  (the matrix-t prior of MultiSPR)
 * Lambda = sum_i log p_i; G is its seed: d Lambda = sum_ij G_ij dK~_ij over all i, j (csrc/loo.hip has the closed form), so
 * smn_lml_grad_terms / smn_kernel_cnn_grad_terms with neg_kinv_d = G, alpha_d = zeros and coef = 0 return d Lambda / d(w_std,
 * b_std, last_w_std, eps).  1 <= c <= 48 (SMN_ENOTSUP above), fp32 and fp64.  Per-point arithmetic and every sum over points
 * are fp64 in a fixed order: two calls give the same bits.
 * smn_loo_head: the head alone.  neg_kinv_d [n,n] = -K~^-1 (ld = ldkinv; only the LOWER triangle is read, which is what both
 *   routes of the gradient entries leave), alpha_d [n,c] = A and y_d [n,c] row-major.  Out: *loo_logpdf_h = Lambda, loo_mean_d
 *   [n,c], loo_scale2_d [n] (1 / p_i, or sigma_i^2), dhead_h[2] = d Lambda / d(df, scale) (zeros for df <= 0), and, when g_d is
 *   not NULL, the lower triangle of G in g_d [n,n] (ld = ldg; may be neg_kinv_d itself; the 64 x 64 blocks on the diagonal are
 *   written whole, nothing else above the diagonal is touched).  loo_mean_d and loo_scale2_d may be NULL.  The seed costs one n^3-flop product -(-K~^-1) diag(d) (-K~^-1) over the lower 128 x 128 tiles on the MFMA tile engine
 *   and a workspace of 2 n_pad^2 elements (n_pad = n rounded up to 128): the mirrored, zero-padded operand and its column-
 *   scaled copy.  Synchronises.
 * smn_loo_multi: the counterpart of smn_lml_multi: k_d [n,n] lower (may be overwritten), factorisation with identity, the
 *   head; also *logdet_h and *info_h.  With a kernel build in front this serves every kernel, the conv ResNet included.
 * smn_spr_loo_grad / smn_spr_cnn_loo_grad: everything from x and Y [n,c], the counterparts of smn_spr_loss_grad_multi /
 *   smn_spr_cnn_loss_grad_multi (the conv entry keeps H*W <= SMN_CNN_GRAD_MAX_PIXELS): terms_h[0..3] = d Lambda / d(w_std,
 *   b_std, last_w_std, eps), *loo_logpdf_h, dhead_h[2], *info_h and, when not NULL, loo_mean_d / loo_scale2_d.
 * A matrix that is not positive definite gives info > 0, NaN outputs and SMN_OK. */
int smn_loo_head(smn_ctx* ctx, int dtype, const void* neg_kinv_d, int64_t ldkinv, const void* alpha_d, const void* y_d,
                 int64_t n, int64_t c, double df, double scale, double* loo_logpdf_h, void* loo_mean_d, void* loo_scale2_d,
                 double dhead_h[2], void* g_d, int64_t ldg);
int smn_loo_multi(smn_ctx* ctx, int dtype, void* k_d, int64_t n, int64_t ldk, const void* y_d, int64_t c, double eps_abs,
                  double df, double scale, double* loo_logpdf_h, void* loo_mean_d, void* loo_scale2_d, double dhead_h[2],
                  double* logdet_h, int* info_h, void* g_d, int64_t ldg);
int smn_spr_loo_grad(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens,
                     double w_std, double b_std, double last_w_std,
                     const void* x_d, int64_t n, int64_t ldx, int64_t d, const void* y_d, int64_t c,
                     double eps_abs, double df, double scale, double* loo_logpdf_h, double dhead_h[2], int* info_h,
                     double terms_h[4], void* loo_mean_d, void* loo_scale2_d);
/* smn_spr_kinv: -K~^-1 (neg_kinv_d [n,n], ld = ldkinv a multiple of 16 bytes; the lower triangle is valid) and A = K~^-1 Y
 * (alpha_d [n,c]) exactly as the gradient entries form them from x and Y -- the joint factorisation below n_pad = 8192, the
 * rectangle route from there on -- i.e. what smn_spr_loo_grad hands to the head; also logdet K~ and info. */
int smn_spr_kinv(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens,
                 double w_std, double b_std, double last_w_std,
                 const void* x_d, int64_t n, int64_t ldx, int64_t d, const void* y_d, int64_t c, double eps_abs,
                 void* neg_kinv_d, int64_t ldkinv, void* alpha_d, double* logdet_h, int* info_h);
int smn_spr_cnn_loo_grad(smn_ctx* ctx, int dtype, int act, int num_hiddens,
                         double w_std, double b_std, double last_w_std,
                         const void* x_d, int64_t n, int64_t H, int64_t W, int64_t C, const void* y_d, int64_t c,
                         double eps_abs, double df, double scale, double* loo_logpdf_h, double dhead_h[2], int* info_h,
                         double terms_h[4], void* loo_mean_d, void* loo_scale2_d);

/* ---- sparse variational classifier, evaluation (spax/models.py:58-78 SVSP.test_acc_nll; experiments/classification/test.py) ----
 * With inducing images Z [I], q_mu [C,I], q_var [C,I] = diag(q_sqrt) as the reference uses it (NOT squared) and K the NNGP kernel:
 *     K_rel = K_ZZ + eps tr(K_ZZ)/I I   (NNGPKernel.predict: relative ridge)      K_abs = K_ZZ + eps I   (models.py:68)
 *     mean[t,c] = (K_tZ K_rel^-1 q_mu^T)[t,c]        v0[t] = K(x_t,x_t) - K_tZ K_rel^-1 K_Zt        A = K_tZ K_abs^-1
 *     var[t,c]  = v0[t] + sum_j A[t,j]^2 q_var[c,j]  (sample_f_iid reads only the diagonal of the reference's [B,B] covariance)
 *     f[c,t,s]  = mean[t,c] + sigma[t,c] xi[c,t,s],  xi iid N(0,1) (GaussianPrior: sigma = sqrt(var)) or Student-t(2a)
 *                 (InverseGammaPrior: sigma = sqrt(b/a var));   lsm = f - logsumexp_c f
 *     score[t,c] = logsumexp_s lsm[c,t,s]      ll[t] = score[t,y_t] - log S      pred[t] = argmax_c score[t,c]
 *
 * smn_kernel_conv_diag: diag_d[i] = K(x_i, x_i), i < n, of smn_kernel_cnn (kind 0) or smn_kernel_conv_resnet (kind 1; num_hiddens
 *   is the block size): the per-image pass those builds run first, alone; no pair kernel is launched and the values are, bit
 *   for bit, the diagonal of the symmetric build.  x_d [n,H,W,C], diag_d [n] of `dtype`.
 * smn_svsp_moments: k_zz_d [I,I] (full), q_mu_d [C,I], q_var_d [C,I] are ALWAYS fp64 -- a 1e-6 jitter is not numerically
 *   positive definite in fp32 --; k_zt_d [I,T], ktt_diag_d [T], mean_d [T,C], var_d [T,C] are `dtype`.  Both factorisations and
 *   the three solves run in fp64 through smn_cholesky / smn_trsm.  *info_h: 0, or the 1-based index of the first pivot of K_rel
 *   (then K_abs) that is non-positive or below I * 2^-52 * max_j K_jj; then mean and var are NaN and the call returns SMN_OK.
 *   *nonpos_h: entries of var that are <= 0 (their sigma is NaN downstream, as the reference's sqrt gives; nothing is clamped).
 * smn_mc_softmax: mean_d, sigma_d [T,C] of `dtype`; labels_h [T] host int32, validated to [0,C) (SMN_EINVAL); df <= 0 normal,
 *   df > 0 Student-t(df) variates; point0 = global index of the first point; noise_d NULL, or [T,C,S] standard variates of
 *   `dtype` to use instead of the generator.  Out: ll_d [T] fp64, pred_d [T] int32 (first maximum), score_d [T,C] fp64 or NULL.
 *   `dtype` selects the arithmetic of the generator, the fused multiply-add and the exponentials; the running maxima over
 *   the draws, every merge of (max, sum) pairs and the outputs are fp64 (for C <= 16 a lane's own running sums are `dtype`:
 *   terms in [0, 1] relative to its fp64 maximum).  Log-sum-exps over S are online: nothing of size T C S exists, and with
 *   noise_d == NULL the variates are made in registers and never stored.  1 <= C <= SMN_SVSP_MAX_CLASSES.  Synchronises.
 * smn_rng_variates: out_d [npoints,C,S] of `dtype` = exactly the variates smn_mc_softmax(noise_d = NULL) consumes for points
 *   point0 .. point0 + npoints - 1.
 *
 * Generator: Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11), key = (seed & 0xffffffff, seed >> 32).  The variate of
 * (seed, global point index p, class c, draw s, df) is a pure function of those five values -- not of T, the batch a point
 * arrives in, the grid, or C.  Counter layout (four 32-bit words; p, s < 2^32):
 *     normal     ctr = (s, p, c >> 2, 0): the block's words (r0, r1) give classes 4g, 4g+1 and (r2, r3) classes 4g+2, 4g+3 by
 *                Box-Muller: u = (r_even + 1/2) 2^-32, z = sqrt(-2 ln u) (cos, sin)(2 pi (r_odd + 1/2) 2^-32)
 *     Student-t  ctr = (s, p, c, 0x80000000 | k), k = 0 .. 31: Bailey's polar method, two tries per block -- (r0, r1), then
 *                (r2, r3) -> (u, v) = (r + 1/2) 2^-31 - 1; the first try with w = u^2 + v^2 <= 1 gives
 *                t = u sqrt(df (w^(-2/df) - 1) / w).  64 tries at most (a loop of fixed trip count; 1e-43 of the variates
 *                find none and are 0).
 *     chi-square ctr = (s, 0, 0, 0xC0000000 | k), k = 0 .. 31: the mixing variate g_s ~ chi2(df) of draw s (smn_rng_chi2,
 *                smn_mvn_draws below), chi2(df) = 2 Gamma(df / 2) by Marsaglia & Tsang: a = df / 2 (a + 1 and the boost U^(1/a)
 *                if a < 1), d = a - 1/3, c = 1 / sqrt(9 d); try k: (r0, r1) -> x by Box-Muller (cos branch), v = (1 + c x)^3,
 *                rejected if 1 + c x <= 0; r2 -> u, accepted if ln u < x^2 / 2 + d - d v + d ln v; r3 -> the boost uniform.
 *                32 tries at most (fixed trip count; a draw that finds none is df, probability below 1e-40).  Always fp64.
 *                Word 3 collides with neither the normal stream (0) nor the Student-t stream (0x80000000 | k, k < 32).
 * fp32 evaluates the same formulas in fp32 on the top 23 bits of a word for u in (0, 1) ((r >> 9) 2^-23 + 2^-24) and the top 24
 * for (u, v) in (-1, 1) ((r >> 8) 2^-23 + 2^-24 - 1): odd multiples of 2^-24, exact in fp32, never 0 or +-1.
 * smn_debug_philox: test hook, one raw block: out = Philox4x32-10(ctr, key), computed on the device. */
#define SMN_SVSP_MAX_CLASSES 128
int smn_kernel_conv_diag(smn_ctx* ctx, int dtype, int kind, int act, int num_hiddens,
                         double w_std, double b_std, double last_w_std,
                         const void* x_d, int64_t n, int64_t H, int64_t W, int64_t C, void* diag_d);
int smn_svsp_moments(smn_ctx* ctx, int dtype, const void* k_zz_d, const void* k_zt_d, const void* ktt_diag_d,
                     const void* q_mu_d, const void* q_var_d, int64_t I, int64_t T, int64_t C, double eps,
                     void* mean_d, void* var_d, int* info_h, int64_t* nonpos_h);
int smn_mc_softmax(smn_ctx* ctx, int dtype, const void* mean_d, const void* sigma_d, const int* labels_h,
                   int64_t T, int64_t C, int64_t S, double df, uint64_t seed, int64_t point0, const void* noise_d,
                   void* ll_d, void* pred_d, void* score_d);
int smn_rng_variates(smn_ctx* ctx, int dtype, uint64_t seed, double df, int64_t point0, int64_t npoints, int64_t C,
                     int64_t S, void* out_d);
int smn_debug_philox(smn_ctx* ctx, const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);

/* ---- sparse variational classifier, training (spax/models.py:30-56 SVSP.loss; spax/priors.py:21-26,36-42,52-58,70-82;
 *      experiments/classification/train.py:61-75) ----
 * The negative ELBO and its analytic gradient with respect to every trainable (the inducing images: smn_kernel_cnn_input_grad).  U = [Z; x] (I inducing
 * and B batch images), K = K(U,U), q_var = diag(q_sqrt) as above, scale = 1 / s = 1 (GaussianPrior) or b/a / a/b
 * (InverseGammaPrior), df = 2a, N = num_train:
 *     K_abs = K_ZZ + eps I     K_rel = K_ZZ + eps tr(K_ZZ)/I I     Kinv = K_abs^-1     A = K_xZ Kinv     P = K_rel^-1 K_Zx
 *     mean[c] = A q_mu[c]  (K_abs here; the evaluation path uses K_rel: the reference's own difference)
 *     cov[c]  = A diag(q_var[c]) A^T + K_xx - K_xZ P          L_c = chol(scale cov[c])
 *     f[c,b,s] = mean[c,b] + sum_k L_c[b,k] xi[c,k,s]         xi[c,k,s] = the variate of (seed, point0 + k, class c, draw s)
 *     ll = mean_{b,s} log_softmax_c(f)[y_b,b,s]
 *     kl = 1/2 (C logdet K_ZZ [no jitter] - sum log q_var - I C + sum_c sum_i Kinv_ii q_var[c,i] + s sum_c q_mu[c]^T Kinv q_mu[c])
 *     loss = -ll + kl / N   (+ the closed-form inverse-gamma terms of priors.py:78-81, which the host adds)
 * The Student-t variates are iid per (class, point, draw) (priors.py:52-58 through utils.py multivariate_t: NOT a multivariate t);
 * their pathwise derivative in df (Bailey's polar method at fixed (u, v)) replaces the implicit gamma gradient of JAX's random.t.
 *
 * smn_rng_variates_ddf: out_d [npoints,C,S] = exactly what smn_rng_variates returns, dout_d [npoints,C,S] = d out / d df
 *   (zeros for df <= 0):  dt/ddf = t/2 [1/df + (2 ln w / df^2) w^(-2/df) / (w^(-2/df) - 1)].
 * smn_svsp_head_grad: mean_d [C,B], cov_d [C,B,B] (lower triangles read), gmean_d [C,B], gcov_d [C,B,B] (symmetric, full) are
 *   ALWAYS fp64; labels_h [B] host int32, validated.  Out: *ll_h; gmean = d(-ll)/d mean; gcov = d(-ll)/d cov through the
 *   reverse-mode Cholesky (Phi = tril(L^T gL) with the diagonal halved, gS = sym(L^-T Phi L^-1), gcov = scale gS);
 *   *gscale_h = d(-ll)/d scale = sum_c <gS_c, cov[c]>; *dfterm_h = sum gf[c,b,s] L_c[b,k] d xi[c,k,s]/d df (0 for df <= 0), the
 *   pathwise part of d(-ll)/d df.  noise_d NULL, or [C,B,S] standard variates of `dtype` used instead of the generator, with
 *   dnoise_d NULL (zeros) or their df-derivatives.  `dtype` selects the arithmetic of the variates and of the exponentials:
 *   f_c - max_c f is rounded to `dtype` once and exp / log are `dtype`'s, so that every softmax entry is within a few units of
 *   `dtype`'s roundoff of the exact one in ABSOLUTE terms, whatever the level of f.  The factors, the sums over k (f itself), s
 *   and c, and every gradient are fp64, in a fixed order (no floating-point atomics): two calls give the same bits.  1 <= C <= SMN_SVSP_MAX_CLASSES; B > SMN_SVSP_MAX_BATCH: SMN_ENOTSUP.
 *   A cov[c] that is not positive definite (a pivot non-positive or below B * 2^-52 * max_j cov_jj): *info_h > 0, NaN outputs,
 *   SMN_OK.  Synchronises.
 * smn_svsp_elbo_grad: k_d [I+B, I+B] (ld = ldk, full), q_mu_d, q_var_d [C,I], g_q_mu_d, g_q_var_d [C,I], gbar_d [I+B, I+B]
 *   (ld = ldg) ALWAYS fp64; `dtype` is the head's.  Out: *nll_h = -ll, *kl_n_h = kl / N, g q_mu, g q_var (with respect to q_var,
 *   not the raw q_sqrt), *g_eps_h, *gscale_h (as above), *g_s_h = d loss / d s, *dfterm_h, and Gbar = d loss / d K, symmetric
 *   with both triangles filled, so that sum_ij Gbar_ij dK_ij/d theta is d loss / d theta for a kernel hyper-parameter:
 *   smn_kernel_cnn_grad_terms over the I + B images with neg_kinv_d = Gbar, alpha_d = zeros, coef = 0 gives it for w_std, b_std
 *   and last_w_std, and smn_kernel_cnn_input_grad (below) over the same images with gbar_d = Gbar and n_grad = I gives it for the
 *   inducing images.  Three I x I factorisations (K_ZZ, K_abs, K_rel) through the library's Cholesky; *info_h > 0 (first bad
 *   pivot of K_ZZ, K_abs, K_rel, then of the head) with NaN outputs and SMN_OK when one is not positive definite.  One
 *   synchronisation, at the end. */
#define SMN_SVSP_MAX_BATCH 256
int smn_rng_variates_ddf(smn_ctx* ctx, int dtype, uint64_t seed, double df, int64_t point0, int64_t npoints, int64_t C,
                         int64_t S, void* out_d, void* dout_d);
int smn_svsp_head_grad(smn_ctx* ctx, int dtype, const void* mean_d, const void* cov_d, const int* labels_h,
                       int64_t B, int64_t C, int64_t S, double df, double scale, uint64_t seed, int64_t point0,
                       const void* noise_d, const void* dnoise_d, double* ll_h, void* gmean_d, void* gcov_d,
                       double* gscale_h, double* dfterm_h, int* info_h);
int smn_svsp_elbo_grad(smn_ctx* ctx, int dtype, const void* k_d, int64_t ldk, int64_t I, int64_t B, int64_t C,
                       const void* q_mu_d, const void* q_var_d, double eps, double s, double num_train,
                       const int* labels_h, int64_t S, double df, double scale, uint64_t seed, int64_t point0,
                       const void* noise_d, const void* dnoise_d, double* nll_h, double* kl_n_h, void* g_q_mu_d,
                       void* g_q_var_d, double* g_eps_h, double* gscale_h, double* g_s_h, double* dfterm_h,
                       void* gbar_d, int64_t ldg, int* info_h);

/* ---- joint posterior function draws of the exact models (SPR / MultiSPR.sample_posterior) ----
 * From the posterior mean [T,C] and a finished lower Cholesky factor L [T,T] of the (ridged) posterior covariance:
 *     out[s,t,c] = mean[t,c] + r_s sum_{k<=t} L[t,k] xi[k,c,s]
 * xi[k,c,s] is the NORMAL variate of (seed, point point0 + k, class c, draw s) of the generator above -- the value
 * smn_rng_variates(df = 0) returns, whatever df is here -- or noise_d[k,c,s] when noise_d [T,C,S] of `dtype` is given (the
 * seam the product is tested through; its strided loads are not meant to be fast).  r_s = 1 for df <= 0 (a Gaussian draw;
 * shape is ignored).  For df > 0, r_s = sqrt(shape df / g_s) with ONE g_s ~ chi2(df) per draw, shared by all its points and
 * outputs -- which makes draw s a multivariate t with df degrees of freedom and shape matrix shape (I_C x L L^T), not T C
 * independent ones: g_s = mix_d[s] (fp64 [S]) when mix_d is given, else the variate smn_rng_chi2 returns for (seed, s); r_s is
 * formed in fp64 and rounded to `dtype` once.
 * The product runs on the MFMA tile engine (f32 / f64 16x16x4) in `dtype`; its operand xi is generated tile by tile into the
 * LDS image and never stored.  Only the lower triangle of l_d (ld = ldl >= T, no alignment asked) is read, and only the
 * K-steps at or left of a column tile's last row are run.  The order of the sum over k depends on T alone -- not on S, C or
 * the grid --, there are no floating-point atomics: two calls give the same bits, and noise_d = smn_rng_variates(df = 0),
 * mix_d = smn_rng_chi2 give the bits of noise_d = mix_d = NULL.  out_d [S,T,C] of `dtype`.
 * SMN_EINVAL: null pointers, bad dtype, T, C or S < 1, df > 0 without shape > 0, point0 < 0, point0 + T > 2^32, S > 2^32,
 * ldl < T (by name); SMN_ENOTSUP: C > SMN_SVSP_MAX_CLASSES.  Synchronises.
 * smn_rng_chi2: out_d [S] fp64 = the chi-square mixing variates of (seed, s), s < S (layout above); df > 0. */
int smn_rng_chi2(smn_ctx* ctx, uint64_t seed, double df, int64_t S, void* out_d);
int smn_mvn_draws(smn_ctx* ctx, int dtype, const void* mean_d, const void* l_d, int64_t ldl, int64_t T, int64_t C, int64_t S,
                  double df, double shape, uint64_t seed, int64_t point0, const void* noise_d, const void* mix_d, void* out_d);

/* ---- reverse mode of the conv-NNGP kernel with respect to its input images (spax/models.py:21,31: SVSP.inducing_variable is
 *      a TrainVar; experiments/classification/train.py:205 puts model.vars() into the optimiser) ----
 * smn_kernel_cnn_input_grad: gx_d [n_grad,H,W,C] = sum_ab gbar_ab dK_ab/dx_i for the first n_grad of the n images x_d [n,H,W,C],
 *   K = smn_kernel_cnn(x, x) with its exact diagonal; the other images are partners only (in SVSP: the batch).  gbar_d [n,n] of
 *   `dtype` (ld = ldg): only the lower triangle is read and it is taken as symmetric, the convention of
 *   smn_kernel_cnn_grad_terms, so the Gbar of smn_svsp_elbo_grad goes in unchanged.  One reverse sweep per image pair, one wave
 *   per (image, slice of its partners); per-element arithmetic in `dtype`, the sums over partners in fp64 and in a fixed order
 *   (no floating-point atomics: two calls give the same bits).  Workspace: the per-image tables, one slab of forward values
 *   per resident wave and one block of sums per slice; nothing of size n^2 H W.  fp32 / fp64, relu / erf.
 *   Limit: H*W <= SMN_CNN_GRAD_MAX_PIXELS whatever the aspect ratio (1 x 1024 included), larger images return SMN_ENOTSUP; no
 *   limit on num_hiddens (0: the Flatten + Dense of the raw pixel products alone).  b_std == 0 exactly and
 *   images with all-zero neighbourhoods, or an image that also occurs among the partners, give finite values (zero-variance
 *   pixels contribute no variance-side term, as above).  1 <= n_grad <= n, ldg >= n (SMN_EINVAL otherwise).  Synchronises. */
int smn_kernel_cnn_input_grad(smn_ctx* ctx, int dtype, int act, int num_hiddens,
                              double w_std, double b_std, double last_w_std,
                              const void* x_d, int64_t n, int64_t H, int64_t W, int64_t C,
                              const void* gbar_d, int64_t ldg, int64_t n_grad, void* gx_d);

/* ---- the conv-NNGP kernel differentiated in its first argument for many seeds at once: saliency maps of a fitted posterior
 *      (jax.grad of the predictive of experiments/nt_kernels.py:34-45 with respect to the test images) ----
 * smn_kernel_cnn_input_grad_cross: for K = smn_kernel_cnn, rows x1_d [n1,H,W,C] and partners x2_d [n2,H,W,C], which do not move,
 *     gmean_d [n1, c, H, W, C]:  gmean[r, k] = sum_j alpha[j, k] dK(x1_r, x2_j)/dx1_r     (alpha_d [n2, c] row-major: column seeds,
 *                                                                                          shared by all rows)
 *     gvar_d  [n1, H, W, C]:     gvar[r] = gdiag[r] dK(x1_r, x1_r)/dx1_r + sum_j gbar[r, j] dK(x1_r, x2_j)/dx1_r
 *   with K(x, x) the exact per-image diagonal; gbar_d [n1, ldg >= n2], gdiag_d [n1]; gdiag_d == NULL: no diagonal term, gbar_d ==
 *   NULL: no cross term.  Either output may be NULL (its seeds are then not run); gmean_d needs alpha_d, gvar_d needs gbar_d or
 *   gdiag_d; 1 <= c <= 48, c is ignored (and may be 0) when alpha_d is NULL.  A fitted posterior's gradients are alpha = K~^-1 Y,
 *   gbar = -2 K_td K~^-1 (smn_fit_weights) and gdiag = 1.
 *   The reverse sweep is linear in its seed: a pair runs ONE forward and ONE reverse sweep (from the unit seed, without the
 *   mirror factor 2 of the symmetric entry) for all c + 1 seeds, and only the n1 x n2 cross pairs are visited -- against
 *   (n1 + n2)^2 pairs once per seed through smn_kernel_cnn_input_grad on the union.  Per-element arithmetic in `dtype`, the sums
 *   over partners in fp64 and in a fixed order (no floating-point atomics: two calls give the same bits).  A row's partner list
 *   is cut into slices by n1, n2, the pixels-per-lane form and the device alone; the sums ([seeds][rows x slices][L + C][64 NP]
 *   doubles) are capped at min(256 MB, smn_debug_batch_bytes) by running the seeds in groups -- one more pass over the pairs
 *   each -- and, beyond that, the rows in batches: the bits depend neither on the budget nor on which outputs are asked for
 *   (a mean-only or variance-only call gives the bits of the joint call).  ROWS COMPUTED ALONE NEED NOT CARRY THE BITS OF THE
 *   SAME ROWS IN A LARGER CALL: n1 enters the cut.
 *   fp32 / fp64, relu / erf, num_hiddens >= 0, H*W <= SMN_CNN_GRAD_MAX_PIXELS at any aspect ratio (SMN_ENOTSUP above, naming the
 *   limit); zero-variance pixels and an x1 image that also occurs in x2 give finite values, as in the symmetric entry.
 *   SMN_EINVAL by name: x1_d / x2_d NULL, both outputs NULL, gmean_d without alpha_d, gvar_d without gbar_d and gdiag_d, n1 < 1,
 *   n2 < 1, ldg < n2; SMN_ENOTSUP: c > 48.  A refused call writes nothing.  Synchronises. */
int smn_kernel_cnn_input_grad_cross(smn_ctx* ctx, int dtype, int act, int num_hiddens,
                                    double w_std, double b_std, double last_w_std,
                                    const void* x1_d, int64_t n1, const void* x2_d, int64_t n2, int64_t H, int64_t W, int64_t C,
                                    const void* alpha_d, int64_t c, const void* gbar_d, int64_t ldg, const void* gdiag_d,
                                    void* gmean_d, void* gvar_d);

/* ---- the MLP / dense-ResNet kernels differentiated in their first argument (experiments/nt_kernels.py:21-31, 83-103 under
 *      jax.grad with respect to x1: sensitivities, acquisition ascent, saliency) ----
 * smn_kernel_mlp_input_grad: gx_d [n1, ldgx >= d] = sum_j gbar[r, j] dK(x1_r, x2_j)/dx1_r for K = smn_kernel_mlp(x1, x2); net
 *   may carry SMN_NET_NTK (then K is Theta).  With u = x1_r . x2_j / d and v = |x1_r|^2 / d, dK_rj/dx1_r = (F_1 x2_j + 2 F_2
 *   x1_r) / d: F_1 = dK/du and F_2 = dK/dv are carried through the layer stack in forward mode in the epilogue of the fused MFMA
 *   Gram tile (per-element arithmetic in `dtype`), (gbar o F_1) X2 runs on the tile engine, the row sums of gbar o F_2 in fp64
 *   in a fixed order (no floating-point atomics: two calls give the same bits).  x2_d must be given: the form in which both
 *   arguments move (x2 == x1) is not implemented -> SMN_EINVAL by name.  gbar_d [n1, ldg >= n2] of `dtype`.  A row of x1 equal
 *   to a row of x2 (ReLU: D_A = D_1 = 0 there) and an all-zero row with b_std == 0 (no variance-side term) give finite values.
 *   fp32 / fp64, relu / erf, any num_hiddens up to 16 activation layers (SMN_ENOTSUP above).  No synchronisation. */
int smn_kernel_mlp_input_grad(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, double w_std, double b_std, double last_w_std,
                              const void* x1_d, int64_t n1, int64_t ldx1, const void* x2_d, int64_t n2, int64_t ldx2, int64_t d,
                              const void* gbar_d, int64_t ldg, void* gx_d, int64_t ldgx);

/* ---- the log-marginal likelihood differentiated in the INPUTS: per-feature input scales (automatic relevance determination) and
 *      d loss / d X (experiments/regression/train.py:61-67 under objax.GradValues with the inputs, or a per-feature scale in front
 *      of experiments/nt_kernels.py:21-31, 83-103, among the variables; spax/models.py:93-98 is the loss) ----
 * Notation: x~ = the inputs as the kernel sees them, G = coef A A^T - c K~^-1 the seed of smn_lml_grad_terms_multi (A = K~^-1 Y
 * [n, c]), u_nm = x~_n . x~_m / d, v_n = |x~_n|^2 / d, F_1 = dK_nm/du, F_2[n, m] = dK_nm/dv_n, ddiag_n = dK_nn/dv_n (closed-form
 * diagonal).  Then with W = G o F_1 (zero diagonal) and r_n = sum_{m != n} G_nm F_2[n, m]
 *     gx_n   = d log p / d x~_n = (sum_m W_nm x~_m + (2 r_n + G_nn ddiag_n) x~_n) / d
 *     feat_j = sum_n gx[n, j] x~[n, j]        (x~ = s o x:  d log p / d s_j = feat_j / s_j,  d log p / d x_n = s o gx_n)
 * smn_scale_columns: out_d [n, ldo >= d] = x_d [n, ldx >= d] with column j multiplied by s_h[j] (a host vector, rounded to `dtype`
 *   first; the product in `dtype`: the bits of NumPy's x * s.astype(dtype)).  out_d may be x_d.  16-byte accesses when ldx and ldo
 *   are multiples of 16 bytes and both bases are aligned.  One synchronisation (the upload of s).
 * smn_kernel_mlp_input_grad_sym: gx_d [n, ldgx >= d] and / or feat_h [d] (host, fp64; one may be NULL, each leaves the other's bits
 *   as they are) for a generic symmetric seed, the way smn_kernel_cnn_grad_terms takes one: neg_kinv_d [n, ldkinv >= n] (its lower
 *   triangle is read), alpha_d [n, c] row-major and coef; with coef = 0, a zero alpha and c = 1 the seed is the matrix passed as
 *   neg_kinv_d.  net may carry SMN_NET_NTK (Theta in place of K).  One elementwise pass over the lower triangle of the Gram matrix
 *   x~ x~^T / d (built here as the gradient entries build it) carries (K, K_u, K_v, K_v') -- the row-side and the column-side variance
 *   tangent -- through the layer stack in `dtype` and writes W; the sums of G o F_2 are fp64, one slot per (tile, row), added in
 *   tile order (no floating-point atomics: two calls give the same bits, and a row's values do not depend on ldx, ldgx or an earlier
 *   call); W X~ runs on the MFMA tile engine, its epilogue adding the row term and, for feat_h, the fp64 column sums of gx o x~.
 *   Two exactly equal rows (ReLU: D_A = D_1 = 0 there) and an all-zero row with b_std == 0 give finite values.  Workspace, beside
 *   the Gram matrix: one n_pad x n_pad matrix (W), the transposed padded inputs and (n_pad / 64 + 1) x n_pad doubles, n_pad =
 *   round_up(n, 128) -- 1.1 GB in fp32 at n = 16384 --, all acquired before the first launch.  c <= 48; at most 16 activation layers
 *   (SMN_ENOTSUP above).  feat_h != NULL: one synchronisation at the end; else none.
 * smn_spr_loss_grad_inputs: smn_spr_loss_grad_multi followed by that pass on the posterior it leaves on the device: quad_h,
 *   quad_cols_h, logdet_h, info_h and terms_h[0..3] are smn_spr_loss_grad_multi's bits on the same arguments, gx_d / feat_h those of
 *   smn_kernel_mlp_input_grad_sym fed smn_spr_kinv's outputs and coef = the head's (1: Gaussian; (df + n c) / ((df + Q / scale)
 *   scale): Student-t).  These are derivatives of log p, not of the loss (the loss is -log p / n).  Not positive definite: *info_h
 *   != 0, NaN in the scalar outputs, gx_d and feat_h untouched, SMN_OK. */
int smn_scale_columns(smn_ctx* ctx, int dtype, const void* x_d, int64_t n, int64_t ldx, int64_t d, const double* s_h, void* out_d,
                      int64_t ldo);
int smn_kernel_mlp_input_grad_sym(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, double w_std, double b_std,
                                  double last_w_std, const void* x_d, int64_t n, int64_t ldx, int64_t d, const void* neg_kinv_d,
                                  int64_t ldkinv, const void* alpha_d, int64_t c, double coef, void* gx_d, int64_t ldgx,
                                  double* feat_h);
int smn_spr_loss_grad_inputs(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, double w_std, double b_std,
                             double last_w_std, const void* x_d, int64_t n, int64_t ldx, int64_t d, const void* y_d, int64_t c,
                             double eps_abs, double df, double scale, double* quad_h, double* quad_cols_h, double* logdet_h,
                             int* info_h, double terms_h[4], void* gx_d, int64_t ldgx, double* feat_h);

/* ---- multi-GPU (nothing in the reference to mirror) ----
 * One process per GPU.  Rank 0 calls smn_comm_unique_id and ships the 128 bytes to the other
 * ranks by any host channel; every rank then calls smn_comm_init.  smn_allgather is an RCCL
 * all-gather of `count` elements per rank on the context's stream; the caller states the world it
 * believes it is in: SMN_ECOMM when that is not the communicator's size (a context without a
 * communicator is a world of one, where the gather is a copy) -- a world > 1 call can never quietly
 * gather nothing. */
int smn_comm_unique_id(char id_out[128]);
int smn_comm_init(smn_ctx* ctx, int nranks, int rank, const char id[128]);
int smn_comm_destroy(smn_ctx* ctx);
int smn_allgather(smn_ctx* ctx, int nranks, int dtype, const void* send_d, void* recv_d, int64_t count);
/* Paired lower-trapezoid layout (host side: sharding.py).  The n rows are cut into 2*nranks blocks
 * of block_rows rows (a multiple of 128); rank r owns blocks r and 2*nranks-1-r and packs block b
 * densely as block_rows rows of leading dimension (b+1)*block_rows, low block first, so every rank
 * contributes block_rows^2 * (2*nranks+1) elements to ONE smn_allgather.  This call scatters the
 * gathered stage_d [nranks * that count] into the lower triangle (by 128-column tiles) of
 * k_d [n,n] ld=ldk in natural row order. */
int smn_unpack_lower_blocks(smn_ctx* ctx, int dtype, const void* stage_d, int64_t n, int nranks,
                            int64_t block_rows, void* k_d, int64_t ldk);
/* smn_lml (same outputs, same likelihood arguments) fed from the gathered staging buffer: the blocks are
 * scattered straight into the factorisation workspace, K is never assembled separately. */
int smn_lml_from_blocks(smn_ctx* ctx, int dtype, const void* stage_d, int64_t n, int nranks,
                        int64_t block_rows, const void* y_d, double eps_abs, double df, double scale,
                        double* logpdf_h, double* quad_h, double* logdet_h, int* info_h);
/* nranks / rank of the context's communicator (1 / 0 without one). */
int smn_comm_info(smn_ctx* ctx, int* nranks, int* rank);

/* ---- column-first exchange: the factorisation starts on the columns that have arrived ----
 * Cyclic layout (host side: sharding.py; nothing in the reference to mirror, run.py:17 only masks devices).  The 128-row
 * tile rows are dealt to the ranks in boustrophedon order with period 2*nranks: group j = tile rows [j P, (j+1) P), rank r
 * owns t_j(r) = j P + (j even ? r : P-1-r).  Every rank builds the same number of lower tiles and every aligned group of P
 * tile rows holds one tile row per rank, so any tile-COLUMN range [c0, c1) with c0 a multiple of P is an equal-count
 * all-gather: ceil((T - c0) / P) strips of 128 x (c1-c0)*128 elements per rank (T = ceil(n / 128)).  piece_cols[0..npieces]
 * are those boundaries (0 = piece_cols[0] < ... < piece_cols[npieces] = T, at most 16 pieces); a rank's chunk holds its
 * pieces one after the other, the staging buffer piece g of all ranks at nranks * (offset of piece g).
 *   smn_shard_begin            the factorisation workspace of smn_lml_from_shards, made ready before the first piece lands;
 *                              eps_abs is the absolute jitter (spax/models.py:96), added to the diagonal as it is scattered
 *   smn_kernel_mlp_shard_cols  the rank's whole share of the build in ONE launch, into its chunk nngp_chunk_d / ntk_chunk_d
 *   smn_shard_exchange_cols    piece `piece`: RCCL all-gather on the context's communication stream (ordered after everything
 *                              issued so far on its main stream), scatter into the workspace on a third stream; returns at
 *                              once.  nranks must equal the communicator's size (SMN_ECOMM otherwise)
 *   smn_shard_exchange_cols_to the same, scattered into k_d [n,n] ld=ldk (lower triangle by 128-column tiles): the NTK of a
 *                              joint NNGP + NTK shard (BASELINE config 5; the reference's only use: sample.ipynb cells 194-195)
 *   smn_shard_scatter_cols     the scatter half alone, from a staging buffer the caller filled on the main stream (k_d NULL:
 *                              into the workspace, as smn_shard_exchange_cols does)
 *   smn_shard_wait             the main stream waits for every piece issued so far
 *   smn_lml_from_shards        factorisation + head, same outputs as smn_lml.  The factorisation waits for the pieces one by
 *                              one as it reaches their columns: only the first piece is exposed, the rest of the exchange
 *                              rides under the first super-panel's panel chain
 *   smn_debug_delay            test hook: holds stream 0 (main) / 1 (communication) / 2 (scatter) for usec microseconds */
int smn_shard_begin(smn_ctx* ctx, int dtype, int64_t n, double eps_abs);
int smn_kernel_mlp_shard_cols(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens,
                              double w_std, double b_std, double last_w_std,
                              const void* x_d, int64_t n, int64_t ldx, int64_t d,
                              int nranks, int rank, int npieces, const int64_t* piece_cols,
                              int get_mask, void* nngp_chunk_d, void* ntk_chunk_d);
int smn_shard_exchange_cols(smn_ctx* ctx, int dtype, const void* mine_d, void* stage_d, int64_t n, int nranks,
                            int npieces, const int64_t* piece_cols, int piece);
int smn_shard_exchange_cols_to(smn_ctx* ctx, int dtype, const void* mine_d, void* stage_d, int64_t n, int nranks,
                               int npieces, const int64_t* piece_cols, int piece, void* k_d, int64_t ldk);
int smn_shard_scatter_cols(smn_ctx* ctx, int dtype, const void* stage_d, int64_t n, int nranks, int npieces,
                           const int64_t* piece_cols, int piece, void* k_d, int64_t ldk);
int smn_shard_wait(smn_ctx* ctx);
int smn_lml_from_shards(smn_ctx* ctx, int dtype, int64_t n, const void* y_d, double df, double scale,
                        double* logpdf_h, double* quad_h, double* logdet_h, int* info_h);
int smn_debug_delay(smn_ctx* ctx, int stream_id, int64_t usec);

/* ---- greedy pivoted Cholesky: a rank-M factor K ~ L L^T and M inducing points, without the N x N matrix (csrc/pchol.hip) ----
 * State: L_d [n, ldl] of `dtype`, row-major, column j written at step j; resid_d [n] in fp64, r_i = K_ii - sum_t L_it^2.  One
 * step with pivot p and its kernel row k = K(x_p, X): l_i = (k_i - sum_{t<j} L_it L_pt) / sqrt(r_p), L_ij = l_i rounded to
 * `dtype`, r_i <- r_i - L_ij^2; the pivot's row gets L_pj = sqrt(r_p) and r_p = 0, a row whose residual is exactly 0 (an earlier
 * pivot, a zero diagonal) gets L_ij = 0 and stays at 0.  Next pivot: argmax r_i, ties to the LOWEST index; remaining trace:
 * sum_i max(r_i, 0).  Sums in fp64 in a fixed order (per lane ascending, then a butterfly; partials of 16 rows, then one
 * reducing workgroup): no floating-point atomics, two calls give the same bits, and the bits depend neither on the grid nor on
 * the alignment of the operands.  16-byte loads when a base is 16-byte aligned and its leading dimension a multiple of 16 bytes.
 *   smn_pchol_begin  matrix form: resid_d <- diag_d [n] (of `dtype`) in fp64; *pivot_h, *rmax_h, *trace_h = the first pivot, its
 *                    residual and the trace.  One synchronisation.
 *   smn_pchol_step   matrix form: step j with `pivot` and its row krow_d [n] of `dtype` (from any kernel function);
 *                    *next_pivot_h, *rmax_h, *trace_h = the next pivot, its residual, the remaining trace.  SMN_EINVAL with the
 *                    state untouched when resid[pivot] is not > 0, when j >= ldl or j >= n.  When to stop is the caller's
 *                    decision.  Two synchronisations.
 *   smn_pchol_mlp    fused form for SMN_NET_MLP / SMN_NET_DENSE_RESNET (NNGP; SMN_NET_NTK -> SMN_ENOTSUP): the rows are made in
 *                    the step kernel from x_d [n, ldx >= d] -- K0 = x_i . x_p / d streamed once per step, then the layer stack in
 *                    fp64 for both dtypes -- and the initial residual is the closed-form diagonal of smn_kernel_mlp.  Up to
 *                    max_rank <= n steps (ldl >= max_rank) are queued without a host round trip; the loop stops before step j
 *                    when trace_j <= tol_rel trace_0 (tol_rel >= 0; 0: never) or when the largest residual is not above
 *                    4 (j + 1) eps max_i K_ii, eps the unit roundoff of `dtype`: the rounding noise of a residual computed from
 *                    j stored columns -- the matrix has run out of numerical rank.  The floor does not grow with n.  *rank_h = columns made; pivots_h [max_rank]: [0, rank) written; trace_h [max_rank + 1]:
 *                    [0, rank] written (the trace before each step and after the last); columns [rank, max_rank) of L_d are
 *                    zero.  One synchronisation, at the end. */
int smn_pchol_begin(smn_ctx* ctx, int dtype, int64_t n, const void* diag_d, double* resid_d, int64_t* pivot_h,
                    double* rmax_h, double* trace_h);
int smn_pchol_step(smn_ctx* ctx, int dtype, int64_t n, int64_t j, int64_t pivot, const void* krow_d, void* L_d, int64_t ldl,
                   double* resid_d, int64_t* next_pivot_h, double* rmax_h, double* trace_h);
int smn_pchol_mlp(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, double w_std, double b_std, double last_w_std,
                  const void* x_d, int64_t n, int64_t ldx, int64_t d, int64_t max_rank, double tol_rel, void* L_d, int64_t ldl,
                  double* resid_d, int64_t* pivots_h, double* trace_h, int64_t* rank_h);
/* smn_pchol_mlp_at: smn_pchol_mlp at PRESCRIBED pivots: step j is taken at pivots_h[j] (host, m entries in [0, n), else
 * SMN_EINVAL; 1 <= m <= n, ldl >= m) instead of the arg-max.  The same step kernel is queued, with no host round trip and one
 * synchronisation at the end; the pivot's residual is read behind step j - 1 and in front of step j.  The loop stops before
 * step j when resid[pivots_h[j]] is not above the floor 4 (j + 1) eps max_i K_ii (an index listed twice, or a duplicate of an
 * earlier pivot's row, therefore ends the factor there) or on tol_rel, as above.  At the pivots smn_pchol_mlp returned, with the
 * same hyper-parameters, L_d, resid_d and trace_h carry that call's bits.  trace_h [m + 1], *rank_h as above. */
int smn_pchol_mlp_at(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, double w_std, double b_std, double last_w_std,
                     const void* x_d, int64_t n, int64_t ldx, int64_t d, const int64_t* pivots_h, int64_t m, double tol_rel,
                     void* L_d, int64_t ldl, double* resid_d, double* trace_h, int64_t* rank_h);

/* ---- regression on the pivoted-Cholesky factor: GP / Student-t models at O(n m^2) work and O(n m) memory (csrc/lowrank.hip) ----
 * With L_d [n, ldl >= m] of `dtype` from smn_pchol_* and d_i = fitc max(resid_i, 0) + lambda, the model covariance is
 * K^ = L L^T + diag(d): FITC on the greedy inducing points (fitc = 1) or SoR / DTC (fitc = 0).  Woodbury, W = diag(1 / d):
 *   G = L^T W L,  B = L^T W Y,  s_k = sum_i w_i y_ik^2,  A = I + G = C C^T,  beta = A^-1 B,
 *   quad_k = y_k^T K^^-1 y_k = s_k - |C^-1 B_k|^2,   logdet = log|K^| = log|A| + sum_i log d_i.
 * Everything of size m x m is fp64 for both dtypes.  1 <= m <= SMN_LOWRANK_MAX_RANK, else SMN_ENOTSUP naming the limit.
 * SMN_EINVAL, before anything is allocated or launched: a NULL pointer where one is needed, n, m or t below 1, c below its
 * minimum (above 48: SMN_ENOTSUP), a leading dimension below the extent it strides, lambda not a positive finite number, fitc
 * neither 0 nor 1.  SMN_ENOTSUP also for an n whose splits do not fit a launch (about 2^31 / (block pairs) splits).
 *   smn_lowrank_gram     G_d [m, ldg >= m] (the whole matrix, the upper half mirrored from the lower bit for bit), B_d [m, c] and
 *                        s_d [c], all fp64, from L_d, the weights w_d [n] (fp64; NULL: every weight 1) and y_d [n, ldy >= c] of
 *                        `dtype`; 0 <= c <= 48, c = 0: G alone (y_d, B_d, s_d not touched).  The rows are cut into splits of
 *                        SMN_LOWRANK_SPLIT rows; G accumulates each split on the MFMA of `dtype` (f32: the weight rounded to f32,
 *                        w l rounded, then the MFMA), B and s in fp64; the splits are then added in fp64 in ascending order.  No
 *                        floating-point atomics: two calls give the same bits, and the bits depend neither on ldl nor on the
 *                        alignment of L_d (16-byte loads when the base is 16-byte aligned and ldl a multiple of 16 bytes, element
 *                        loads into the same registers otherwise).  Workspace, kept by the context:
 *                        ceil(n / SMN_LOWRANK_SPLIT) blocks of the lower half of G in `dtype`.  No synchronisation.
 *   smn_lowrank_fit      the quantities above from L_d, resid_d [n] (fp64, smn_pchol's residual diagonal; NULL: zeros), lambda > 0,
 *                        fitc in {0, 1} and y_d [n, ldy >= c], 1 <= c <= 48.  A is factored by smn_cholesky in fp64.  quad_h [c],
 *                        *logdet_h; C_d [m, m] (lower, zeros above) and beta_d [m, c], both fp64, stay on the device for
 *                        smn_lowrank_readout.  *info_h: 0, or the failing pivot of A (1-based): quad_h, *logdet_h, C_d and beta_d
 *                        are then NaN and the return is SMN_OK, as smn_lml does.  Synchronises.
 *   smn_lowrank_readout  predictions at t test points from kzt_d [m, ldk >= t] = K(Z, x*) (Z: the pivots' inputs) and
 *                        ktt_d [t] = K(x*, x*), both of `dtype`; R_d [m, ldr >= m] = L[pivots, :] in fp64 (lower triangular,
 *                        K(Z, Z) = R R^T), C_d and beta_d [m, c] from smn_lowrank_fit.  phi = R^-1 K(Z, x*), mean = phi^T beta,
 *                        var = k** - |phi|^2 + |C^-1 phi|^2 (the DTC / FITC predictive of the latent function), computed in fp64
 *                        and written as mean_d [t, c], var_d [t] of `dtype`.  Every sum has a fixed order that does not depend on t:
 *                        a point predicted alone carries the bits it has inside a larger chunk.  No synchronisation. */
#define SMN_LOWRANK_MAX_RANK 4096
#define SMN_LOWRANK_SPLIT 512
int smn_lowrank_gram(smn_ctx* ctx, int dtype, const void* L_d, int64_t n, int64_t m, int64_t ldl, const double* w_d,
                     const void* y_d, int64_t c, int64_t ldy, double* G_d, int64_t ldg, double* B_d, double* s_d);
int smn_lowrank_fit(smn_ctx* ctx, int dtype, const void* L_d, int64_t n, int64_t m, int64_t ldl, const double* resid_d,
                    double lambda, int fitc, const void* y_d, int64_t c, int64_t ldy, double* C_d, double* beta_d, double* quad_h,
                    double* logdet_h, int* info_h);
int smn_lowrank_readout(smn_ctx* ctx, int dtype, const void* kzt_d, int64_t ldk, const void* ktt_d, int64_t t, int64_t m,
                        const double* R_d, int64_t ldr, const double* C_d, const double* beta_d, int64_t c, void* mean_d,
                        void* var_d);

/* smn_lowrank_grad (csrc/lowrank_grad.hip): the analytic hyper-parameter gradient of the low-rank model's log-marginal likelihood
 * at FIXED pivots.  With K^ = Q + diag(mu o (k - q)) + lambda I, Q = K_nP K_PP^-1 K_Pn = L L^T, mu_i = fitc [resid_i > 0] and
 * G = coef alpha alpha^T - c K^^-1 (the convention of smn_lml_grad_terms: d logpdf / d theta = terms / 2),
 *   terms_h[0..2] = sum_ij G_ij dK^_ij / d(w_std, b_std, last_w_std),   terms_h[3] = tr G  (d / d lambda).
 * The pivot SELECTION is not differentiated: the factor must have been built at pivots_h (host, m distinct indices in [0, n)),
 * e.g. by smn_pchol_mlp_at, and x_d [n, ldx >= d], L_d [n, ldl >= m], resid_d [n] (fp64; may be NULL when fitc = 0), lambda,
 * fitc, y_d [n, ldy >= c], C_d [m, m], beta_d [m, c] (smn_lowrank_fit's outputs for these inputs) and R_d [m, ldr >= m] =
 * L[pivots, :] in fp64 must belong together.  net: SMN_NET_MLP or SMN_NET_DENSE_RESNET with NNGP covariance (SMN_NET_NTK:
 * SMN_ENOTSUP); act relu or erf.  coef = 1 (Gaussian) or (df + n c) / ((df + quad / scale) scale) (Student-t).
 * O(n m^2 + n m d) work; workspace kept by the context: two [n, m] matrices of `dtype` (X Z^T / d and U) and O(m^2) fp64.  Everything
 * m x m is fp64 for both dtypes; the per-element tangents run in the arithmetic of `dtype`, every sum that crosses elements in
 * fp64 in a fixed order: two calls give the same bits, and the bits depend neither on ldl, ldx nor on alignment.  b_std == 0:
 * as smn_lml_grad_terms.  An f32 factor under fitc with a small lambda loses digits exactly as smn_lowrank_fit's quad does
 * (pivot rows have weight 1 / lambda and kappa_i = w_i - w_i^2 h_i cancels).  SMN_EINVAL, before anything is allocated or
 * launched: the cases of the block above, a pivot out of range or listed twice, m > n, d < 1, a coef that is not finite, fitc = 1
 * without resid_d.  Synchronises. */
int smn_lowrank_grad(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, double w_std, double b_std, double last_w_std,
                     const void* x_d, int64_t n, int64_t ldx, int64_t d, const int64_t* pivots_h, const void* L_d, int64_t m,
                     int64_t ldl, const double* resid_d, double lambda, int fitc, const void* y_d, int64_t c, int64_t ldy,
                     const double* C_d, const double* beta_d, const double* R_d, int64_t ldr, double coef, double* terms_h);

/* ---- matrix-free exact GP: the kernel matrix applied to vectors, never stored (csrc/kernel_matmul.hip, csrc/pcg.hip) ----
 * smn_kernel_mlp_matmul: out_d [n1, ldo >= t] (fp64 for both dtypes) = K(x1, x2) V, V = v_d [n2, ldv >= t] of `dtype`, K the
 *   kernel of smn_kernel_mlp (SMN_NET_MLP or SMN_NET_DENSE_RESNET, relu or erf; SMN_NET_NTK OR-ed into net: K is Theta).
 *   x2_d == NULL is the symmetric form: n2 and ldx2 are ignored, V has n1 rows, the diagonal of K is the closed-form exact one,
 *   and out = K(x1, x1) V + shift V, the shift added in fp64 after the reduction (never folded into a `dtype` diagonal entry).
 *   In the cross form shift must be 0.  Each 128x128 tile of K is made in registers by the main loop and the epilogue of the
 *   fused build and multiplied by its 128 rows of V on the MFMA of `dtype`; it never reaches memory.  The contraction is cut into
 *   splits of SMN_MATMUL_SPLIT rows of V: one split accumulates in the MFMA's precision, the splits are added in fp64 in ascending
 *   order.  No floating-point atomics: out[i, k] depends on x1, x2, V[:, k] and the hyper-parameters alone -- not on t or the
 *   other columns, not on ldx*, ldv, ldo or the alignment of any base, not on a grid or an earlier call.  Any t >= 1: one pass
 *   holds SMN_MATMUL_PASS columns, further columns go in further passes, each of which recomputes the Gram tiles (cost:
 *   ceil(t / SMN_MATMUL_PASS) builds of the n1 x n2 rectangle; K = K^T is not exploited).  Workspace, kept by the context:
 *   the padded operands, the per-row tables and the split partials [splits, n1, t] in fp64, all acquired before the first
 *   launch.  With b_std == 0, zero rows and duplicate rows give finite values, as the build does.  No synchronisation.
 *   SMN_EINVAL, before anything is allocated or launched: a NULL pointer where one is needed, n1, n2 (cross form), d or t below
 *   1, a leading dimension below its extent, a bad dtype, net or act, a shift that is not finite or not 0 in the cross form.
 *   SMN_ENOTSUP: more than 16 activation layers. */
#define SMN_MATMUL_SPLIT 4096
#define SMN_MATMUL_PASS 16
int smn_kernel_mlp_matmul(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, double w_std, double b_std,
                          double last_w_std, const void* x1_d, int64_t n1, int64_t ldx1, const void* x2_d, int64_t n2,
                          int64_t ldx2, int64_t d, double shift, const void* v_d, int64_t t, int64_t ldv, double* out_d,
                          int64_t ldo);

/* smn_pcg_solve: block preconditioned conjugate gradients on (K(x, x) + lambda I) X = B, K applied by smn_kernel_mlp_matmul (same
 *   net / act / dtype rules), x_d [n, ldx >= d] of `dtype`, b_d [n, ldb >= c] and sol_d [n, lds >= c] fp64, 1 <= c <= 48.
 *   Preconditioner M = L L^T + lambda I with L_d [n, ldl >= m] of `dtype` from smn_pchol_*, 0 <= m <= min(n, SMN_LOWRANK_MAX_RANK);
 *   L_d == NULL or m == 0: M = lambda I.  M^-1 r = (r - L (lambda I + L^T L)^-1 L^T r) / lambda; the m x m matrix is formed once per
 *   call and factored by smn_cholesky in fp64; everything m x m is fp64.
 *   c independent CG recurrences (each column its own alpha and beta) share one K-apply per iteration; the direction is cast to
 *   `dtype` for it, every vector (X, R, Z, P) and every inner product is fp64, summed in a fixed order: two calls give the same
 *   bits.  A column stops when its recurrence residual has |r_k| <= tol |b_k| (its iteration count goes to col_iters_h[k], its
 *   direction leaves the shared K-apply); a zero b_k gives x_k = 0 at iteration 0; the loop ends when every column has stopped or
 *   at max_iter.  warm != 0: sol_d is read as the start.  *iters_h: iterations run.  resid_h [c]: the TRUE relative residuals
 *   |b_k - (K + lambda I) x_k| / |b_k| of the returned solution, from one further K-apply (0 for a zero b_k).  hist_h, if given,
 *   [(max_iter + 1), c]: the recurrence's relative residual per iteration and column (a stopped column keeps its last value;
 *   iterations not run are NaN).  *info_h: 0 every column stopped on tol; 1 max_iter was reached (the solution so far is
 *   returned and finite); 2 breakdown -- p^T K~ p <= 0 or a scalar that is not finite -- and sol_d, resid_h are NaN.  The return
 *   value is SMN_OK in all three cases, as smn_lml does.  SMN_EINVAL as smn_kernel_mlp_matmul, and for lambda not positive and
 *   finite, tol outside (0, 1), max_iter < 1, m < 0, m > n, ldl < m, c < 1; SMN_ENOTSUP for c > 48 and m above
 *   SMN_LOWRANK_MAX_RANK.  Workspace, kept by the context: six [n, c] vectors and the m x m factor.  Synchronises. */
int smn_pcg_solve(smn_ctx* ctx, int dtype, int net, int act, int num_hiddens, double w_std, double b_std, double last_w_std,
                  const void* x_d, int64_t n, int64_t ldx, int64_t d, double lambda, const void* L_d, int64_t m, int64_t ldl,
                  const double* b_d, int64_t c, int64_t ldb, double tol, int max_iter, int warm, double* sol_d, int64_t lds,
                  int* iters_h, int* col_iters_h, double* resid_h, double* hist_h, int* info_h);

#ifdef __cplusplus
}
#endif
#endif /* SMNNGP_H */
