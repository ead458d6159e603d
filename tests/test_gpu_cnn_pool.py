"""GPU tests of the pooled conv-NNGP kernel: smn_kernel_cnn_pool / smn_kernel_cnn_pool_diag (csrc/cnn_pool.hip),
nt_kernels.get_cnn_pool_kernel and the models on top of it, against the fp64 rules of tests/_cnn_pool_rules.py.

Tolerances.  Kernel entries: the project's kernel tolerances, relerr < 2e-3 in fp32 and < 1e-8 in fp64 (RTOL of the other conv
tests).  The fp64 duplicate-image case alone is allowed max(1e-8, 4 x the Flatten kernel's own error on the same images): an
x2 image equal to an x1 image puts c = 1 - O(u) into the pair map of every same-pixel entry, where the map's square root turns
a rounding error u into sqrt(u); the pooled kernel averages entries of that kind in another order.  Losses: 1e-9 (fp64) / 1e-3
(fp32) of max(1, |reference|), solve outputs relerr_norm < 1e-7 in fp64 -- test_gpu_multi.py's and test_gpu_fit.py's for the
conv kernels; the pooled matrices here have cond(K + eps I) <= N max K / eps < 1e6, so a factorisation error of cond x 2^-53
stays three orders below both.

Shapes are the smallest at which the kernel takes each of its paths: one pixel; degenerate rows and columns; offsets whose
quadrants are thinner than their halo (3x4); exactly 64 pixels; 63 / 72 pixels (one and two pixels per lane); the 4- and
16-pixel forms with ragged last pixels (12x10, 9x8); 32x32 = the 1024-pixel limit; 1x1024 (two waves per workgroup: four maps
of 1027 columns do not fit the LDS).  Inputs are fp32-representable, so one reference serves both dtypes."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _cnn_pool_rules as PR  # noqa: E402
import _loo_rules as LO  # noqa: E402
import _multi_rules as M  # noqa: E402
import _svsp_rules as SV  # noqa: E402
from _tol import relerr, relerr_norm  # noqa: E402
from _windows import out_window  # noqa: E402
from oracle import nngp_oracle as O  # noqa: E402

RTOL = {np.float32: 2e-3, np.float64: 1e-8}
DTYPES = [np.float64, np.float32]
W_STD, LW_STD = 1.3, 0.9
DEFAULT_BATCH_BYTES = 48 << 30      # csrc/common.hpp


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@functools.lru_cache(maxsize=None)
def images(n, h, w, c, seed):
    x = np.random.default_rng(seed).standard_normal((n, h, w, c)).astype(np.float32).astype(np.float64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(shape, n2, depth, act, b_std):
    """(sym [n,n], cross [n,n2]) of the rules on images(shape) against itself / against n2 other images."""
    x1 = images(*shape, seed=7)
    x2 = images(n2, *shape[1:], seed=8)
    kw = dict(num_hiddens=depth, act=act, w_std=W_STD, b_std=b_std, last_w_std=LW_STD)
    sym, cross = PR.pool_kernel(x1, None, **kw), PR.pool_kernel(x1, x2, **kw)
    sym.setflags(write=False); cross.setflags(write=False)
    return sym, cross


def pool(L, ctx, x1, x2, depth, act, b_std, dtype, fill=None, out=None, ldk=None):
    """smn_kernel_cnn_pool through the C ABI; returns the [n1, n2] result (or fills `out`, a device pointer, at ldk)."""
    a = ctx.to_device(np.ascontiguousarray(x1, dtype=dtype))
    b = None if x2 is None else ctx.to_device(np.ascontiguousarray(x2, dtype=dtype))
    n1, h, w, c = a.shape
    n2 = n1 if b is None else b.shape[0]
    k = None
    if out is None:
        k = ctx.to_device(np.full((n1, n2), np.nan, dtype))
        out, ldk = k.ptr, n2
    ctx.call("smn_kernel_cnn_pool", L.dtype_code(dtype), L.ACT[act], depth, W_STD, b_std, LW_STD, a.ptr, n1,
             None if b is None else b.ptr, 0 if b is None else n2, h, w, c, L.FILL_FULL if fill is None else fill, out, ldk)
    return None if k is None else k.raw_numpy()


def pool_diag(L, ctx, x, depth, act, b_std, dtype):
    a = ctx.to_device(np.ascontiguousarray(x, dtype=dtype))
    n, h, w, c = a.shape
    d = ctx.to_device(np.full((n,), np.nan, dtype))
    ctx.call("smn_kernel_cnn_pool_diag", L.dtype_code(dtype), L.ACT[act], depth, W_STD, b_std, LW_STD, a.ptr, n, h, w, c, d.ptr)
    return d.raw_numpy()


def assert_rules(what, got, ref, dtype, tol=None):
    tol = RTOL[dtype] if tol is None else tol
    err = relerr(got, ref)
    print("%s %s: relerr %.3g (tolerance %g)" % (what, np.dtype(dtype).name, err, tol))
    assert np.isfinite(got).all(), what
    assert err < tol, (what, err)


# ----------------------------------------------------------------------------------------------- 1. parity with the rules
#        (n, H, W, C)     depth  b_std
CASES = [((3, 1, 1, 3), 1, 0.3),        # one pixel: one unit, one slice
         ((3, 1, 5, 1), 4, 0.0),        # a single row
         ((3, 5, 1, 2), 1, 0.3),        # a single column
         ((4, 3, 4, 2), 4, 0.3),        # quadrants thinner than their halo
         ((4, 3, 4, 2), 0, 0.3),        # no activation layer: the product of the pixel means
         ((12, 8, 8, 1), 1, 0.0),       # exactly 64 pixels: every lane owns one
         ((3, 9, 7, 1), 4, 0.3),        # 63 pixels: one idle lane
         ((3, 9, 8, 1), 1, 0.0),        # 72 pixels: the 4-pixel form, ragged
         ((3, 12, 10, 2), 4, 0.3),      # 120 pixels
         ((3, 32, 32, 3), 2, 0.3),      # 1024 pixels = the limit: the 16-pixel form, 1024 units of 4 slices
         ((2, 1, 1024, 1), 1, 0.0)]     # the other extreme of the limit; two waves per workgroup


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ["relu", "erf"])
@pytest.mark.parametrize("shape,depth,b_std", CASES)
def test_parity_with_the_rules(L, ctx, shape, depth, b_std, act, dtype):
    n2 = 2
    sym, cross = reference(shape, n2, depth, act, b_std)
    x1, x2 = images(*shape, seed=7), images(n2, *shape[1:], seed=8)
    what = "%s depth %d b_std %g %s" % (shape, depth, b_std, act)
    ks = pool(L, ctx, x1, None, depth, act, b_std, dtype)
    assert_rules(what + " symmetric", ks, sym, dtype)
    assert np.array_equal(bits(ks), bits(ks.T)), what + ": the symmetric build is not exactly symmetric"
    kc = pool(L, ctx, x1, x2, depth, act, b_std, dtype)
    assert_rules(what + " cross", kc, cross, dtype)
    d = pool_diag(L, ctx, x1, depth, act, b_std, dtype)
    assert np.array_equal(bits(d), bits(np.diag(ks))), what + ": smn_kernel_cnn_pool_diag differs from the symmetric diagonal"


def test_python_entry_matches_the_abi(L, ctx):
    from smnngp import nt_kernels
    shape, depth, b_std = (4, 3, 4, 2), 4, 0.3
    x1, x2 = images(*shape, seed=7), images(2, *shape[1:], seed=8)
    fn = nt_kernels.get_cnn_pool_kernel(depth, 1, act="erf", w_std=W_STD, b_std=b_std, last_w_std=LW_STD)
    assert np.array_equal(fn(x1).numpy(), pool(L, ctx, x1, None, depth, "erf", b_std, np.float64))
    assert np.array_equal(fn(x1, x2).numpy(), pool(L, ctx, x1, x2, depth, "erf", b_std, np.float64))
    assert np.array_equal(fn.diag(x1).numpy(), np.diag(fn(x1).numpy()))
    lower = fn(x1, None, fill="lower").numpy()
    assert np.array_equal(np.tril(lower), np.tril(fn(x1).numpy()))


# ------------------------------------------------------------------------------------------------------ 2. awkward inputs
@functools.lru_cache(maxsize=None)
def zero_images():
    x = images(4, 8, 8, 1, seed=11).copy()
    x[0, 2:5, 2:5] = 0.0                # an all-zero 3x3 neighbourhood: a zero-variance pixel after the first conv
    x[1] = 0.0                          # a whole zero image
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ["relu", "erf"])
def test_zero_pixels_at_zero_bias(L, ctx, act, dtype):
    x, x2 = zero_images(), images(2, 8, 8, 1, seed=12)
    kw = dict(num_hiddens=2, act=act, w_std=W_STD, b_std=0.0, last_w_std=LW_STD)
    assert_rules("zero pixels symmetric " + act, pool(L, ctx, x, None, 2, act, 0.0, dtype), PR.pool_kernel(x, None, **kw), dtype)
    assert_rules("zero pixels cross " + act, pool(L, ctx, x2, x, 2, act, 0.0, dtype), PR.pool_kernel(x2, x, **kw), dtype)


@pytest.mark.parametrize("act", ["relu", "erf"])
def test_duplicate_image_across_the_two_arguments(L, ctx, act):
    """x2[0] = x1[1] in a cross call: the same-pixel entries of that pair reach the pair map at c = 1 (no per-image shortcut
    in a cross build)."""
    shape, depth, b_std = (3, 6, 5, 2), 3, 0.3
    x1 = images(*shape, seed=21)
    x2 = images(3, *shape[1:], seed=22).copy()
    x2[0] = x1[1]
    kw = dict(num_hiddens=depth, act=act, w_std=W_STD, b_std=b_std, last_w_std=LW_STD)
    ref = PR.pool_kernel(x1, x2, **kw)
    assert_rules("duplicate " + act, pool(L, ctx, x1, x2, depth, act, b_std, np.float32), ref, np.float32)
    # fp64: the Flatten kernel's own error on the same images sets the scale
    a, b = ctx.to_device(np.ascontiguousarray(x1)), ctx.to_device(np.ascontiguousarray(x2))
    kf = ctx.empty((3, 3), np.float64)
    ctx.call("smn_kernel_cnn", L.F64, L.ACT[act], depth, W_STD, b_std, LW_STD, a.ptr, 3, b.ptr, 3, shape[1], shape[2], shape[3],
             L.FILL_FULL, kf.ptr, 3)
    flat_err = relerr(kf.raw_numpy(), O.cnn_kernel(x1, x2, depth, act, W_STD, b_std, LW_STD))
    tol = max(1e-8, 4.0 * flat_err)
    print("duplicate %s: the Flatten kernel's own error %.3g -> tolerance %.3g" % (act, flat_err, tol))
    assert_rules("duplicate " + act, pool(L, ctx, x1, x2, depth, act, b_std, np.float64), ref, np.float64, tol=tol)


# ------------------------------------------------------------------------------------------------------------ 3. structure
@pytest.mark.parametrize("dtype", DTYPES)
def test_fill_lower_leaves_everything_else_untouched(L, ctx, dtype):
    shape, depth, b_std = (5, 3, 4, 2), 2, 0.3
    x = images(*shape, seed=7)
    n = shape[0]
    full = pool(L, ctx, x, None, depth, "relu", b_std, dtype)
    for layout in ("aligned", "unaligned"):
        win = out_window(ctx, n, n, dtype, layout)
        assert win.ld > n
        before = win.initial()
        pool(L, ctx, x, None, depth, "relu", b_std, dtype, fill=L.FILL_LOWER, out=win.ptr, ldk=win.ld)
        got = win.result("FILL_LOWER " + layout)            # guard bands and the row tails behind n2: byte for byte
        low, up = np.tril_indices(n), np.triu_indices(n, 1)
        assert np.array_equal(bits(got[low]), bits(full[low]))
        assert np.array_equal(bits(got[up]), bits(before[up])), "strict upper triangle written under SMN_FILL_LOWER"
    x2 = images(3, *shape[1:], seed=8)
    win = out_window(ctx, n, 3, dtype, "unaligned")
    pool(L, ctx, x, x2, depth, "relu", b_std, dtype, out=win.ptr, ldk=win.ld)
    assert np.array_equal(bits(win.result("cross, ldk > n2")), bits(pool(L, ctx, x, x2, depth, "relu", b_std, dtype)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,depth", [((5, 8, 8, 1), 2), ((4, 12, 10, 2), 1), ((3, 32, 32, 3), 1)])
def test_bits_depend_on_the_pair_alone(L, ctx, shape, depth, dtype):
    """Rows of a cross build against one-row calls, entries of the symmetric build against 1 x 1 cross calls (below the
    diagonal: the diagonal pair of a symmetric build takes its same-pixel entries from the per-image recursion), and a
    second call."""
    b_std, act = 0.3, "erf"
    x1, x2 = images(*shape, seed=7), images(3, *shape[1:], seed=8)
    kc = pool(L, ctx, x1, x2, depth, act, b_std, dtype)
    assert np.array_equal(bits(kc), bits(pool(L, ctx, x1, x2, depth, act, b_std, dtype))), "two calls differ"
    for i in range(shape[0]):
        assert np.array_equal(bits(kc[i:i + 1]), bits(pool(L, ctx, x1[i:i + 1], x2, depth, act, b_std, dtype))), "row %d" % i
    ks = pool(L, ctx, x1, None, depth, act, b_std, dtype)
    assert np.array_equal(bits(ks), bits(pool(L, ctx, x1, None, depth, act, b_std, dtype))), "two symmetric calls differ"
    n = shape[0]
    for (i, j) in [(1, 0), (n - 1, 0), (n - 1, n - 2)]:
        one = pool(L, ctx, x1[i:i + 1], x1[j:j + 1], depth, act, b_std, dtype)
        assert bits(one)[0, 0] == bits(ks)[i, j], "entry (%d, %d) of the symmetric build" % (i, j)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pair_list_cut_into_passes(L, ctx, dtype):
    """The partial sums of 2 pairs per pass (15 pairs: 8 passes, the last of one pair; 10 cross pairs: 5 passes): the bits
    of the one-pass build."""
    shape, depth, b_std = (5, 8, 8, 1), 2, 0.3
    x1, x2 = images(*shape, seed=7), images(2, *shape[1:], seed=8)
    ks, kc = pool(L, ctx, x1, None, depth, "relu", b_std, dtype), pool(L, ctx, x1, x2, depth, "relu", b_std, dtype)
    d = pool_diag(L, ctx, x1, depth, "relu", b_std, dtype)
    ctx.call("smn_debug_batch_bytes", 2 * 64 * 8)
    try:
        ks2, kc2 = pool(L, ctx, x1, None, depth, "relu", b_std, dtype), pool(L, ctx, x1, x2, depth, "relu", b_std, dtype)
        d2 = pool_diag(L, ctx, x1, depth, "relu", b_std, dtype)
    finally:
        ctx.call("smn_debug_batch_bytes", DEFAULT_BATCH_BYTES)
    assert np.array_equal(bits(ks), bits(ks2)) and np.array_equal(bits(kc), bits(kc2)) and np.array_equal(bits(d), bits(d2))


# --------------------------------------------------------------------------------------------------------------- 4. errors
def test_errors_by_name_and_the_context_survives(L, ctx):
    f64, relu = L.F64, L.ACT["relu"]
    x = ctx.to_device(np.zeros((2, 33, 32, 1)))
    out = ctx.empty((2, 2), np.float64)
    hyp = (W_STD, 0.3, LW_STD)

    def fails(code, *args, entry="smn_kernel_cnn_pool"):
        with pytest.raises(L.SmnError) as e:
            ctx.call(entry, *args)
        assert e.value.code == code, str(e.value)
        return str(e.value)

    assert "1024" in fails(L.ENOTSUP, f64, relu, 2, *hyp, x.ptr, 2, None, 0, 33, 32, 1, L.FILL_FULL, out.ptr, 2)
    assert "1024" in fails(L.ENOTSUP, f64, relu, 2, *hyp, x.ptr, 2, 33, 32, 1, out.ptr, entry="smn_kernel_cnn_pool_diag")
    assert "ldk" in fails(L.EINVAL, f64, relu, 2, *hyp, x.ptr, 2, None, 0, 4, 4, 1, L.FILL_FULL, out.ptr, 1)
    assert "ldk" in fails(L.EINVAL, f64, relu, 2, *hyp, x.ptr, 1, x.ptr, 2, 4, 4, 1, L.FILL_FULL, out.ptr, 1)
    fails(L.EINVAL, f64, relu, 2, *hyp, x.ptr, 0, None, 0, 4, 4, 1, L.FILL_FULL, out.ptr, 2)
    fails(L.EINVAL, f64, relu, 2, *hyp, None, 2, None, 0, 4, 4, 1, L.FILL_FULL, out.ptr, 2)
    fails(L.EINVAL, f64, relu, 2, *hyp, x.ptr, 2, None, 0, 4, 4, 1, L.FILL_FULL, None, 2)
    assert "act" in fails(L.EINVAL, f64, 7, 2, *hyp, x.ptr, 2, None, 0, 4, 4, 1, L.FILL_FULL, out.ptr, 2)
    assert "dtype" in fails(L.EINVAL, 5, relu, 2, *hyp, x.ptr, 2, None, 0, 4, 4, 1, L.FILL_FULL, out.ptr, 2)
    assert "fill" in fails(L.EINVAL, f64, relu, 2, *hyp, x.ptr, 2, None, 0, 4, 4, 1, 9, out.ptr, 2)
    fails(L.EINVAL, f64, relu, 2, *hyp, None, 2, 4, 4, 1, out.ptr, entry="smn_kernel_cnn_pool_diag")
    shape = (4, 3, 4, 2)
    got = pool(L, ctx, images(*shape, seed=7), None, 4, "relu", 0.3, np.float64)
    assert np.array_equal(got, pool(L, ctx, images(*shape, seed=7), None, 4, "relu", 0.3, np.float64))
    assert relerr(got, reference(shape, 2, 4, "relu", 0.3)[0]) < 1e-8


# --------------------------------------------------------------------------------------------------------------- 5. models
N, T, NC, DEPTH, HW = 24, 8, 3, 2, 6
HYP = M.HYP                                  # w_std 1.3, b_std 0.4, last_w_std 0.9, eps 1e-3, alpha 1.7, beta 2.4


def model_data(dtype):
    return M.conv_data(N, NC, HW, HW, 1, dtype == np.float32, T)     # x, Y, labels, x_test, Y_test, labels_test


@functools.lru_cache(maxsize=None)
def model_matrices(f32):
    x, _, _, xt, _, _ = M.conv_data(N, NC, HW, HW, 1, f32, T)
    kw = dict(num_hiddens=DEPTH, act="relu", w_std=HYP["w_std"], b_std=HYP["b_std"], last_w_std=HYP["last_w_std"])
    return PR.pool_kernel(x, None, **kw), PR.pool_kernel(xt, x, **kw), PR.pool_kernel(xt, None, **kw)


def make_model(x, y, method, dtype, multi, labels=None):
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood
    from smnngp.spax.models import SPR, MultiSPR
    kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_cnn_pool_kernel(DEPTH, NC, act="relu", w_std=w, b_std=b, last_w_std=l),
                        HYP["w_std"], HYP["b_std"], HYP["last_w_std"])
    lik = GaussianLikelihood() if method == "gp" else StudentTLikelihood(HYP["alpha"], HYP["beta"])
    x = np.asarray(x, dtype=dtype)
    if labels is not None:
        return MultiSPR.from_labels(kernel, lik, x, labels, NC, eps=HYP["eps"])
    if multi:
        return MultiSPR(kernel, lik, x, np.asarray(y, dtype=dtype), eps=HYP["eps"])
    return SPR(kernel, lik, x, np.asarray(y[:, 0], dtype=dtype), 0.0, 1.0, eps=HYP["eps"])


def check_loss(got, ref, dtype):
    print("loss %.15g reference %.15g" % (got, ref))
    assert abs(got - ref) < (1e-9 if dtype == np.float64 else 1e-3) * max(1.0, abs(ref))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", ["gp", "tp"])
def test_losses_match_the_rules(method, dtype):
    x, y, lab = model_data(dtype)[:3]
    kt = model_matrices(dtype == np.float32)[0] + HYP["eps"] * np.eye(N)
    a, b = HYP["alpha"], HYP["beta"]
    y0 = np.asarray(y[:, 0], dtype=np.float64)
    ref = O.mvn_logpdf(y0, kt) if method == "gp" else O.mvt_logpdf(y0, (b / a) * kt, 2.0 * a)
    spr = make_model(x, y, method, dtype, False)
    check_loss(spr.loss(), -ref / N, dtype)
    multi = make_model(x, None, method, dtype, True, labels=lab)
    check_loss(multi.loss(), -M.head(kt, M.label_targets(lab, NC), method, a, b)[0] / N, dtype)
    loo_ref = LO.from_matrix(kt, y0[:, None], method, a, b)["lam"]
    check_loss(spr.loo_loss(), -loo_ref / N, dtype)
    with pytest.raises(NotImplementedError):
        spr.loss_and_grad()
    with pytest.raises(NotImplementedError):
        multi.loss_and_grad()
    with pytest.raises(NotImplementedError):
        spr.loo_loss_and_grad()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", ["gp", "tp"])
def test_predictions_match_the_rules(method, dtype):
    """1e-7 in fp64 and 1e-2 in fp32, test_gpu_multi.py's tolerances for predictions, NLL and variances; the matrices have
    cond(K + ridge) = 8.7e3 and the class means a margin of 0.38 of the largest, so an fp32 error of cond x 2^-24 = 5e-4
    neither reaches the tolerance nor moves a label."""
    tol = 1e-7 if dtype == np.float64 else 1e-2
    x, y, lab, xt, yt, labt = model_data(dtype)
    kdd, ktd, ktt = model_matrices(dtype == np.float32)
    a, b, eps = HYP["alpha"], HYP["beta"], HYP["eps"]
    # SPR.test_nll (oracle.spr_test_nll's steps on the rules' matrices)
    y0, yt0 = np.asarray(y[:, 0]), np.asarray(yt[:, 0])
    mean, cov = O.predict(kdd, ktd, ktt, y0[:, None], diag_reg=eps)
    if method == "gp":
        lp = O.normal_logpdf(yt0, mean.ravel(), np.sqrt(np.diag(cov)))
    else:
        d = 2.0 * a + y0 @ np.linalg.solve((b / a) * kdd + 1e-6 * np.eye(N), y0)
        lp = O.student_t_logpdf(yt0, 2.0 * a + N, mean.ravel(), np.sqrt(np.diag(d / (2.0 * a + N) * (b / a) * cov)))
    spr = make_model(x, y, method, dtype, False)
    nll, ref_nll = spr.test_nll(xt, yt0), -float(np.mean(lp))
    print("SPR.test_nll %.15g reference %.15g" % (nll, ref_nll))
    assert abs(nll - ref_nll) < tol * max(1.0, abs(ref_nll))
    # the classifier: posterior().predict, classify, accuracy; append then remove restores the bits
    multi = make_model(x, None, method, dtype, True, labels=lab)
    rmean, rcov = O.predict(kdd, ktd, ktt, M.label_targets(lab, NC), diag_reg=eps)
    top = np.sort(rmean, axis=1)
    assert np.min(top[:, -1] - top[:, -2]) > 4.0 * tol * np.abs(rmean).max(), "the premise: no class means within the tolerance"
    assert np.array_equal(multi.classify(xt), np.argmax(rmean, axis=1))
    assert multi.accuracy(xt, labt) == float(np.mean(np.argmax(rmean, axis=1) == labt))
    with multi.posterior(capacity=5) as post:               # two chunks of test rows
        pm, pv = post.predict(xt, cov="diag")
        pm0, pv0 = pm.raw_numpy().copy(), pv.raw_numpy().copy()
        em, ev = relerr_norm(pm0, rmean), np.abs(pv0 - np.diag(rcov)).max() / np.abs(rcov).max()
        print("posterior().predict %s: mean err %.3g var err %.3g (tolerance %g)" % (np.dtype(dtype).name, em, ev, tol))
        assert em < tol and ev < tol
        post.append(xt[:3], labt[:3])
        assert post.num_data == N + 3
        post.remove([N, N + 1, N + 2])
        pm1, pv1 = post.predict(xt, cov="diag")
        assert np.array_equal(bits(pm1.raw_numpy()), bits(pm0)) and np.array_equal(bits(pv1.raw_numpy()), bits(pv0))


def test_auto_train_step_falls_back_to_differences():
    from smnngp.train import build_train_step, train_vars
    x, y = model_data(np.float64)[:2]
    model = make_model(x, y, "tp", np.float64, False)
    before = {k: np.array(v.value, copy=True) for k, v in train_vars(model).items()}
    loss0 = model.loss()
    step = build_train_step(model, method="auto")
    assert step(1e-2) == pytest.approx(loss0, rel=1e-12)
    after = {k: np.asarray(v.value) for k, v in train_vars(model).items()}
    assert all(np.isfinite(v).all() for v in after.values()) and any(not np.array_equal(before[k], after[k]) for k in before)
    with pytest.raises(NotImplementedError):
        build_train_step(model, method="analytic")(1e-2)


def test_svsp_evaluation_on_the_pooled_kernel():
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.models import SVSP
    from smnngp.spax.priors import GaussianPrior
    x, _, _, xt, _, labt = model_data(np.float64)
    n_i, eps = 8, 1e-3
    z = np.asarray(x[:n_i])
    rng = np.random.default_rng(3)
    q_mu, q_var = rng.standard_normal((NC, n_i)), 0.5 + rng.random((NC, n_i))
    kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_cnn_pool_kernel(DEPTH, NC, act="relu", w_std=w, b_std=b, last_w_std=l),
                        HYP["w_std"], HYP["b_std"], HYP["last_w_std"])
    model = SVSP(GaussianPrior(), kernel, z, num_latent_gps=NC, eps=eps)
    model.q_mu.assign(q_mu)
    model.q_sqrt.assign(model.q_sqrt.constraint.inverse(q_var))
    mean, var, info, nonpos = model.posterior_moments(xt)
    kw = dict(num_hiddens=DEPTH, act="relu", w_std=HYP["w_std"], b_std=HYP["b_std"], last_w_std=HYP["last_w_std"])
    rm, rv, cond = SV.moments(PR.pool_kernel(z, None, **kw), PR.pool_kernel(z, xt, **kw), np.diag(model_matrices(False)[2]),
                              q_mu, q_var, eps)
    em, ev = relerr_norm(mean.raw_numpy(), rm), relerr_norm(var.raw_numpy(), rv)
    print("SVSP moments on the pooled kernel: cond(K_rel) %.3g  relerr mean %.3g var %.3g" % (cond, em, ev))
    assert info == 0 and nonpos == 0 and em < 1e-7 and ev < 1e-7
    nll, correct = model.test_acc_nll(5, xt, labt, 64)
    assert np.isfinite(nll) and 0 <= correct <= T
    with pytest.raises(NotImplementedError):
        model.loss_and_grad(5, xt, labt, N, 8)
