"""GPU tests of the conv-NNGP predictive gradients: smn_kernel_cnn_input_grad_cross (csrc/cnn_input_grad.hip) and smn_fit_weights
(csrc/fit.hip) against the fp64 rules of tests/_cnn_cross_grad_rules.py and numpy.linalg.solve, and
FittedPosterior.predict_grad over get_cnn_kernel end to end.

Bounds.  The entry, element-wise against S = the same sum over absolute values: 1e-9 S in fp64 and 2e-3 S in fp32 on inputs
rounded to fp32 first -- the bounds of test_gpu_cnn_input_grad.py; 2e-9 S against the symmetric entry on the union (two device
results, each within 1e-9 S of the rules).  smn_fit_weights and the fp64 posterior: relerr_norm <= 1e-8, TOL64 of
test_gpu_input_grad.py.  The fp32 posterior (ridge 1e-2): the yardstick is the same rules fed seeds solved by float32 NumPy on
the float32-rounded K~, the device's error is held to FP32_RATIO times it, and FP32_RATIO x yardstick may not exceed 2e-3.
FP32_RATIO = 4 x the largest ratio measured on an MI355X, rounded up to a power of two (profiles/r27_cnn_predict_grad.txt).
No wall-clock assertion anywhere."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from _tol import relerr_norm  # noqa: E402

import _cnn_cross_grad_rules as X  # noqa: E402
import _cnn_input_grad_rules as G  # noqa: E402

from oracle import nngp_oracle as O  # noqa: E402  (test infrastructure only)

HYP = dict(w_std=1.3, b_std=0.4, last_w_std=0.9)
TOL64 = 1e-8
FP32_TOL = 2e-3
FP32_RATIO = 16.0   # measured ratios up to 3.77 (profiles/r27_cnn_predict_grad.txt): 4 x 3.77 = 15.1, rounded up to a power of two
DEFAULT_BATCH_BYTES = 48 << 30
# (n1, n2, H, W, C, layers): the 1-, 4- and 16-pixels-per-lane forms, ragged and exact; the two most elongated images the pixel
# limit admits; no hidden layer
SHAPES = [(5, 7, 6, 6, 2, 3), (3, 6, 5, 7, 3, 2), (4, 5, 8, 8, 1, 4), (3, 5, 12, 12, 1, 2), (2, 4, 16, 16, 2, 2),
          (2, 3, 20, 20, 1, 2), (2, 3, 32, 32, 3, 2), (2, 3, 3, 50, 1, 2), (1, 2, 1, 1024, 1, 2), (1, 2, 1024, 1, 2, 1),
          (2, 3, 6, 6, 1, 0)]


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def cross(L, ctx, x1, x2, layers, act, hyp, alpha=None, gbar=None, gdiag=None, dtype=np.float64, mean=True, var=True, c=None,
          ldg=None, n1=None, n2=None, raw=False):
    """One call of the entry; outputs prefilled with NaN.  Returns (gmean or None, gvar or None)."""
    m1, h, w, cin = x1.shape
    m2 = x2.shape[0]
    dev = lambda a: None if a is None else ctx.to_device(np.ascontiguousarray(a, dtype=dtype))   # noqa: E731
    x1d, x2d, ad, gd, dd = dev(x1), dev(x2), dev(alpha), dev(gbar), dev(gdiag)
    cc = (0 if alpha is None else alpha.shape[1]) if c is None else c
    cm = max(cc, 1) if alpha is not None else 1
    om = ctx.to_device(np.full((m1, cm, h, w, cin), np.nan, dtype=dtype)) if mean else None
    ov = ctx.to_device(np.full((m1, h, w, cin), np.nan, dtype=dtype)) if var else None
    ptr = lambda a: None if a is None else a.ptr   # noqa: E731
    args = (L.dtype_code(dtype), L.ACT.get(act, act), layers, hyp["w_std"], hyp["b_std"], hyp["last_w_std"], x1d.ptr,
            m1 if n1 is None else n1, x2d.ptr, m2 if n2 is None else n2, h, w, cin, ptr(ad), cc, ptr(gd), m2 if ldg is None else ldg,
            ptr(dd), ptr(om), ptr(ov))
    if raw:
        return args, om, ov
    ctx.call("smn_kernel_cnn_input_grad_cross", *args)
    return (None if om is None else om.raw_numpy()), (None if ov is None else ov.raw_numpy())


def worst_ratio(got, ref, s, rel):
    """max |got - ref| / (rel * S); an element whose S is 0 must be reproduced exactly."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    diff = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(s > 0, diff / (rel * s), np.where(diff == 0, 0.0, np.inf))
    return float(np.max(ratio))


def within(what, got_m, got_v, ref, dtype, rel=None):
    rel = (1e-9 if np.dtype(dtype) == np.float64 else 2e-3) if rel is None else rel
    rm = worst_ratio(got_m, ref["gmean"], ref["smean"], rel) if got_m is not None else 0.0
    rv = worst_ratio(got_v, ref["gvar"], ref["svar"], rel) if got_v is not None else 0.0
    print("%s %s: worst |err| / (%g S): mean seeds %.3g, variance seed %.3g" % (what, np.dtype(dtype).name, rel, rm, rv))
    assert rm <= 1.0 and rv <= 1.0, what


@functools.lru_cache(maxsize=None)
def case(n1, n2, h, w, cin, layers, act, c, f32, with_diag, hyp=tuple(sorted(HYP.items()))):
    """(x1, x2, alpha, gbar, gdiag as the device sees them, the rules' result): computed once and shared."""
    rng = np.random.default_rng([n1, n2, h, w, cin, layers, c])
    dt = np.float32 if f32 else np.float64
    rd = lambda a: a.astype(dt).astype(np.float64)   # noqa: E731
    x1, x2 = rd(rng.standard_normal((n1, h, w, cin))), rd(rng.standard_normal((n2, h, w, cin)))
    alpha, gbar, gdiag = rd(rng.standard_normal((n2, c))), rd(rng.standard_normal((n1, n2))), rd(rng.standard_normal(n1))
    gdiag = gdiag if with_diag else None
    ref = X.cross_input_grad(x1, x2, layers, act, alpha=alpha, gbar=gbar, gdiag=gdiag, **dict(hyp))
    return x1, x2, alpha, gbar, gdiag, ref


# ----------------------------------------------------------------------------- 1. the entry against the rules
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("act", ["relu", "erf"])
@pytest.mark.parametrize("n1,n2,h,w,cin,layers", SHAPES)
def test_entry_against_the_rules(L, ctx, n1, n2, h, w, cin, layers, act, dtype):
    """c = 3 with gdiag and c = 1 without; two calls give the same bits; mean-only and variance-only calls give the bits of the
    joint call."""
    for c, with_diag in ((3, True), (1, False)):
        x1, x2, alpha, gbar, gdiag, ref = case(n1, n2, h, w, cin, layers, act, c, dtype == np.float32, with_diag)
        gm, gv = cross(L, ctx, x1, x2, layers, act, HYP, alpha, gbar, gdiag, dtype)
        within("cross %s %s c=%d diag=%s" % ((n1, n2, h, w, cin, layers), act, c, with_diag), gm, gv, ref, dtype)
        gm2, gv2 = cross(L, ctx, x1, x2, layers, act, HYP, alpha, gbar, gdiag, dtype)
        assert bits(gm) == bits(gm2) and bits(gv) == bits(gv2), "two calls differ in bits"
        gm3, none = cross(L, ctx, x1, x2, layers, act, HYP, alpha, gbar, gdiag, dtype, var=False)
        assert none is None and bits(gm3) == bits(gm), "the mean-only call differs from the joint call"
        none, gv3 = cross(L, ctx, x1, x2, layers, act, HYP, alpha, gbar, gdiag, dtype, mean=False)
        assert none is None and bits(gv3) == bits(gv), "the variance-only call differs from the joint call"
        none, gv4 = cross(L, ctx, x1, x2, layers, act, HYP, None, gbar, gdiag, dtype, mean=False)       # alpha_d NULL, c = 0
        assert bits(gv4) == bits(gv)


# ----------------------------------------------------------------------------- 2. several slices, several seed groups
def test_sliced_partner_lists_and_seed_groups_give_the_same_bits(L, ctx):
    """n1 = 2 rows cannot fill the device: each row's 300 partners are cut into slices added by the per-image pass.  Within the
    bound, and bit-identical when the workspace budget leaves room for one seed per pass over the pairs (c + 1 = 4 passes)."""
    n1, n2, h, w, cin, layers, act, c = 2, 300, 6, 6, 1, 2, "relu", 3
    x1, x2, alpha, gbar, gdiag, ref = case(n1, n2, h, w, cin, layers, act, c, False, True)
    gm, gv = cross(L, ctx, x1, x2, layers, act, HYP, alpha, gbar, gdiag)
    within("cross n2=300", gm, gv, ref, np.float64)
    # slices hold at least 8 partners: 38 per row, and one seed's sums are 2 x 38 x (L + C) x 64 doubles = 114 KB, so 128 KB
    # hold one seed and not two
    ctx.call("smn_debug_batch_bytes", 128 << 10)
    try:
        gm1, gv1 = cross(L, ctx, x1, x2, layers, act, HYP, alpha, gbar, gdiag)
        ctx.call("smn_debug_batch_bytes", 64 << 10)              # less than one seed of both rows: rows in batches as well
        gm2, gv2 = cross(L, ctx, x1, x2, layers, act, HYP, alpha, gbar, gdiag)
    finally:
        ctx.call("smn_debug_batch_bytes", DEFAULT_BATCH_BYTES)
    assert bits(gm1) == bits(gm) and bits(gv1) == bits(gv), "the bits depend on the workspace budget"
    assert bits(gm2) == bits(gm) and bits(gv2) == bits(gv), "the bits depend on the workspace budget (row batches)"


# ----------------------------------------------------------------------------- 3. against the symmetric entry on the union
@pytest.mark.parametrize("act", ["relu", "erf"])
def test_against_the_symmetric_entry_on_the_union(L, ctx, act):
    n1, n2, h, w, cin, layers, c = 5, 7, 6, 6, 2, 3, 3
    x1, x2, alpha, gbar, gdiag, ref = case(n1, n2, h, w, cin, layers, act, c, False, True)
    gm, gv = cross(L, ctx, x1, x2, layers, act, HYP, alpha, gbar, gdiag)
    u = ctx.to_device(np.concatenate([x1, x2]))

    def union(seed, gd):
        g = ctx.to_device(X._union_seed(seed, gd, n1, n2))
        out = ctx.empty((n1, h, w, cin), np.float64)
        ctx.call("smn_kernel_cnn_input_grad", L.F64, L.ACT[act], layers, HYP["w_std"], HYP["b_std"], HYP["last_w_std"], u.ptr,
                 n1 + n2, h, w, cin, g.ptr, n1 + n2, n1, out.ptr)
        return out.raw_numpy()

    sym = {"gmean": np.stack([union(np.broadcast_to(alpha[:, k], (n1, n2)), None) for k in range(c)], axis=1),
           "gvar": union(gbar, gdiag), "smean": ref["smean"], "svar": ref["svar"]}
    within("cross vs symmetric on the union %s" % act, gm, gv, sym, np.float64, rel=2e-9)


# ----------------------------------------------------------------------------- 4. edges
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("act", ["relu", "erf"])
def test_a_row_that_is_a_copy_of_a_partner(L, ctx, act, dtype):
    n1, n2, h, w, cin, layers, c = 4, 6, 6, 6, 2, 3, 2
    rng = np.random.default_rng(21)
    rd = lambda a: a.astype(dtype).astype(np.float64)   # noqa: E731
    x1, x2 = rd(rng.standard_normal((n1, h, w, cin))), rd(rng.standard_normal((n2, h, w, cin)))
    x1[1], x1[3] = x2[4], x2[0]
    alpha, gbar, gdiag = rd(rng.standard_normal((n2, c))), rd(rng.standard_normal((n1, n2))), np.ones(n1)
    ref = X.cross_input_grad(x1, x2, layers, act, alpha=alpha, gbar=gbar, gdiag=gdiag, **HYP)
    gm, gv = cross(L, ctx, x1, x2, layers, act, HYP, alpha, gbar, gdiag, dtype)
    within("copied partner %s" % act, gm, gv, ref, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("b_std", [0.4, 0.0])
@pytest.mark.parametrize("act", ["relu", "erf"])
def test_zero_border_images(L, ctx, act, b_std, dtype):
    """A two-pixel all-zero border; with b_std = 0 exactly the border pixels have zero variance while their neighbourhood stays
    zero and contribute no variance-side term, on the device and in the rules alike.  Finite everywhere, within the bound."""
    rng = np.random.default_rng(11)
    rd = lambda a: a.astype(dtype).astype(np.float64)   # noqa: E731
    x1, x2 = np.zeros((3, 8, 8, 1)), np.zeros((6, 8, 8, 1))
    x1[:, 2:6, 2:6, :], x2[:, 2:6, 2:6, :] = rng.standard_normal((3, 4, 4, 1)), rng.standard_normal((6, 4, 4, 1))
    x1, x2 = rd(x1), rd(x2)
    alpha, gbar, gdiag = rd(rng.standard_normal((6, 2))), rd(rng.standard_normal((3, 6))), np.ones(3)
    hyp = dict(HYP, b_std=b_std)
    ref = X.cross_input_grad(x1, x2, 3, act, alpha=alpha, gbar=gbar, gdiag=gdiag, **hyp)
    gm, gv = cross(L, ctx, x1, x2, 3, act, hyp, alpha, gbar, gdiag, dtype)
    assert np.isfinite(gm).all() and np.isfinite(gv).all()
    within("zero border %s b_std=%g" % (act, b_std), gm, gv, ref, dtype)


# ----------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_outputs_untouched(L, ctx):
    rng = np.random.default_rng(9)
    x1, x2 = rng.standard_normal((2, 8, 8, 1)), rng.standard_normal((3, 8, 8, 1))
    alpha, gbar, gdiag = rng.standard_normal((3, 2)), rng.standard_normal((2, 3)), np.ones(2)
    big1, big2 = rng.standard_normal((2, 40, 40, 1)), rng.standard_normal((3, 40, 40, 1))
    wide = np.zeros((3, 49))

    def refused(code, needle="", x1=x1, x2=x2, **kw):
        kw = dict(dict(alpha=alpha, gbar=gbar, gdiag=gdiag), **kw)
        args, om, ov = cross(L, ctx, x1, x2, 2, kw.pop("act", "relu"), HYP, raw=True, **kw)
        with pytest.raises(L.SmnError) as e:
            ctx.call("smn_kernel_cnn_input_grad_cross", *args)
        assert e.value.code == code and needle in str(e.value), (code, needle, str(e.value))
        for o in (om, ov):
            assert o is None or np.isnan(o.raw_numpy()).all(), "a refused call wrote to an output"

    refused(L.EINVAL, "both NULL", mean=False, var=False)
    refused(L.EINVAL, "alpha_d", alpha=None, c=2)                  # gmean_d without alpha_d
    refused(L.EINVAL, "gbar_d", gbar=None, gdiag=None)             # gvar_d without gbar_d and gdiag_d
    refused(L.EINVAL, "n1", n1=0)
    refused(L.EINVAL, "n2", n2=0)
    refused(L.EINVAL, "ldg", ldg=2)
    refused(L.EINVAL, "act", act=7)
    refused(L.ENOTSUP, "48", alpha=wide)                           # c = 49
    refused(L.ENOTSUP, "1024", x1=big1, x2=big2)
    args, om, ov = cross(L, ctx, x1, x2, 2, "relu", HYP, alpha, gbar, gdiag, raw=True)
    null_x1, null_x2 = list(args), list(args)
    null_x1[6], null_x2[8] = None, None
    for a in (null_x1, null_x2):
        with pytest.raises(L.SmnError) as e:
            ctx.call("smn_kernel_cnn_input_grad_cross", *a)
        assert e.value.code == L.EINVAL
    assert L._lib.smn_kernel_cnn_input_grad_cross(None, *args) == L.EINVAL                          # NULL context
    with pytest.raises(L.SmnError) as e:
        ctx.call("smn_kernel_cnn_input_grad_cross", 5, *args[1:])                                   # bad dtype
    assert e.value.code == L.EINVAL
    assert np.isnan(om.raw_numpy()).all() and np.isnan(ov.raw_numpy()).all()


# ----------------------------------------------------------------------------- 6. smn_fit_weights
class MatrixFit:
    """A raw smn_fit handle: matrix form from K, or fused from x."""

    def __init__(self, L, ctx, y, capacity, ridge, k=None, x=None):
        self.L, self.ctx = L, ctx
        self.n, self.c = y.shape
        self.h, info = C.c_void_p(), C.c_int()
        yd = ctx.to_device(np.ascontiguousarray(y))
        if k is not None:
            kd = ctx.to_device(np.ascontiguousarray(k))
            ctx.call("smn_fit_create_from_kernel", L.F64, kd.ptr, self.n, self.n, yd.ptr, self.c, 0.0, ridge, capacity, C.byref(self.h),
                     None, None, C.byref(info))
        else:
            xd = ctx.to_device(np.ascontiguousarray(x))
            ctx.call("smn_fit_create", L.F64, 0, L.ACT["relu"], 2, 1.3, 0.4, 0.9, xd.ptr, self.n, x.shape[1], x.shape[1], yd.ptr, self.c,
                     0.0, ridge, capacity, C.byref(self.h), None, None, C.byref(info))
        assert info.value == 0

    def nbytes(self):
        b = C.c_size_t()
        self.ctx.call_on("smn_fit_info", self.h, None, None, None, C.byref(b))
        return int(b.value)

    def apply(self, k_td, ktt):
        t = k_td.shape[0]
        kd, dd = self.ctx.to_device(np.ascontiguousarray(k_td)), self.ctx.to_device(np.ascontiguousarray(ktt))
        mean, var = self.ctx.empty((t, self.c), np.float64), self.ctx.empty((t,), np.float64)
        self.ctx.call_on("smn_fit_apply", self.h, kd.ptr, t, self.n, dd.ptr, None, t, mean.ptr, var.ptr, None, t)
        return mean.raw_numpy(), var.raw_numpy()

    def weights(self, k_td=None, alpha=True):
        t = 0 if k_td is None else k_td.shape[0]
        kd = None if k_td is None else self.ctx.to_device(np.ascontiguousarray(k_td))
        u = None if k_td is None else self.ctx.to_device(np.full((t, self.n + 3), np.nan))          # ldu = n + 3
        al = self.ctx.empty((self.n, self.c), np.float64) if alpha else None
        self.ctx.call_on("smn_fit_weights", self.h, None if kd is None else kd.ptr, t, self.n, None if u is None else u.ptr,
                         self.n + 3, None if al is None else al.ptr)
        un = None if u is None else u.raw_numpy()
        assert un is None or np.isnan(un[:, self.n:]).all(), "smn_fit_weights wrote behind column n"
        return (None if un is None else un[:, :self.n]), (None if al is None else al.raw_numpy())

    def destroy(self):
        self.ctx.call_on("smn_fit_destroy", self.h)


@pytest.mark.parametrize("c", [1, 3])
def test_fit_weights_against_numpy_solve(L, ctx, c):
    """n = 130 (two tile rows), capacity 64, t = 70 in two calls; predict's bits before and after; nbytes grows; the same call
    on a fused state agrees with the matrix form."""
    n, t, d, ridge = 130, 70, 7, 1e-3
    rng = np.random.default_rng(40 + c)
    x, xt, y = rng.standard_normal((n, d)), rng.standard_normal((t, d)), rng.standard_normal((n, c))
    kw = dict(num_hiddens=2, act="relu", w_std=1.3, b_std=0.4, last_w_std=0.9)
    k_dd, k_td, ktt = O.mlp_kernel(x, None, **kw), O.mlp_kernel(xt, x, **kw), np.diag(O.mlp_kernel(xt, None, **kw)).copy()
    kt = k_dd + ridge * np.eye(n)
    ref_u, ref_a = np.linalg.solve(kt, k_td.T).T, np.linalg.solve(kt, y)
    f, g = MatrixFit(L, ctx, y, 64, ridge, k=k_dd), MatrixFit(L, ctx, y, 64, ridge, x=x)
    try:
        before, b0 = f.apply(k_td[:64], ktt[:64]), f.nbytes()
        u1, alpha = f.weights(k_td[:64])
        u2, none = f.weights(k_td[64:], alpha=False)
        _, alpha2 = f.weights(None)
        after, b1 = f.apply(k_td[:64], ktt[:64]), f.nbytes()
        u = np.concatenate([u1, u2])
        eu, ea = relerr_norm(u, ref_u), relerr_norm(alpha, ref_a)
        print("smn_fit_weights c=%d: relerr_norm U %.3g, alpha %.3g; nbytes %d -> %d" % (c, eu, ea, b0, b1))
        assert none is None and eu <= TOL64 and ea <= TOL64 and bits(alpha) == bits(alpha2)
        assert bits(before[0]) == bits(after[0]) and bits(before[1]) == bits(after[1]), "predict changed bits"
        assert b1 > b0
        gu, ga = g.weights(k_td[:64])
        assert relerr_norm(gu, u1) <= TOL64 and relerr_norm(ga, alpha) <= TOL64      # (its K is the device's own build)
        with pytest.raises(L.SmnError) as e:
            f.weights(k_td[:65])                                                      # t > capacity
        assert e.value.code == L.EINVAL
    finally:
        f.destroy()
        g.destroy()


# ----------------------------------------------------------------------------- 7. end to end
N, T, IMG, LAYERS, CAP = 40, 9, (6, 6, 2), 2, 4
RIDGE = {np.float64: 1e-3, np.float32: 1e-2}
MW, MB, MLW = 1.2, 0.3, 1.0


@functools.lru_cache(maxsize=None)
def post_data(c, f32):
    rng = np.random.default_rng(70 + c)
    dt = np.float32 if f32 else np.float64
    rd = lambda a: a.astype(dt).astype(np.float64)   # noqa: E731
    return rd(rng.standard_normal((N,) + IMG)), rd(rng.standard_normal((T,) + IMG)), rd(rng.standard_normal((N, c)))


def _model(multi, method, dtype):
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood
    from smnngp.spax.models import SPR, MultiSPR
    c = 3 if multi else 1
    x, xt, y = post_data(c, dtype == np.float32)
    kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_cnn_kernel(LAYERS, 1, act="relu", w_std=w, b_std=b, last_w_std=l), MW, MB, MLW)
    lik = GaussianLikelihood() if method == "gp" else StudentTLikelihood(2.0, 2.0)
    if multi:
        return MultiSPR(kernel, lik, x.astype(dtype), y, eps=RIDGE[dtype]), x, xt, y
    return SPR(kernel, lik, x.astype(dtype), y[:, 0], 0.0, 1.0, eps=RIDGE[dtype]), x, xt, y


def _check(what, got, ref64, ref32, dtype):
    err = relerr_norm(got, ref64)
    if np.dtype(dtype) == np.float64:
        print("%s: fp64 relerr_norm %.3g" % (what, err))
        assert err <= TOL64, what
        return
    yard = relerr_norm(ref32, ref64)
    print("%s: fp32 relerr_norm %.3g, yardstick %.3g, ratio %.3g" % (what, err, yard, err / yard))
    assert FP32_RATIO * yard <= FP32_TOL, "%s: the bound exceeds the fp32 kernel tolerance" % what
    assert err <= FP32_RATIO * yard, what


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("multi", [False, True], ids=["spr", "multi"])
def test_posterior_predict_grad_end_to_end(ctx, multi, method, dtype):
    """N = 40, T = 9 in three chunks of capacity 4; mean-only and variance-only calls give the joint call's bits; after
    append(xt[:3]) / remove of those rows the gradients return bit for bit."""
    model, x, xt, y = _model(multi, method, dtype)
    c = 3 if multi else 1
    with model.posterior(capacity=CAP) as post:
        assert not post.fused and post.info == 0
        b0 = post.nbytes
        dmean, dvar = post.predict_grad(xt.astype(dtype))
        assert dmean.shape == (T, c) + IMG and dvar.shape == (T,) + IMG and post.nbytes > b0
        dmean, dvar = dmean.raw_numpy(), dvar.raw_numpy()
        # the state's ridge: eps tr(K)/N as the device applied it, absolute in the rules (the models take y as it is)
        f32 = dtype == np.float32
        kern = lambda a, b: O.cnn_kernel(a, b, LAYERS, "relu", MW, MB, MLW)   # noqa: E731
        ref = lambda dt: X.predict_grad(kern, x, y, xt, post.ridge, LAYERS, "relu", MW, MB, MLW, dtype=dt)[:2]   # noqa: E731
        m64, v64 = ref(np.float64)
        m32, v32 = ref(np.float32) if f32 else (None, None)
        what = "posterior %s %s" % ("MultiSPR" if multi else "SPR", method)
        _check(what + " dmean", dmean, m64, m32, dtype)
        _check(what + " dvar", dvar, v64, v32, dtype)
        only_m, none = post.predict_grad(xt.astype(dtype), var=False)
        assert none is None and bits(only_m.raw_numpy()) == bits(dmean)
        none, only_v = post.predict_grad(xt.astype(dtype), mean=False)
        assert none is None and bits(only_v.raw_numpy()) == bits(dvar)
        post.append(xt[:3].astype(dtype), np.zeros((3, c)) if multi else np.zeros(3))
        moved = post.predict_grad(xt.astype(dtype))[1].raw_numpy()
        assert post.num_data == N + 3 and np.isfinite(moved).all() and bits(moved) != bits(dvar)
        post.remove(range(N, N + 3))
        m2, v2 = post.predict_grad(xt.astype(dtype))
        assert post.num_data == N and bits(m2.raw_numpy()) == bits(dmean) and bits(v2.raw_numpy()) == bits(dvar)


def test_a_posterior_over_large_images_has_no_gradient(ctx):
    from smnngp import nt_kernels
    from smnngp.posterior import FittedPosterior
    rng = np.random.default_rng(1)
    x, y = rng.standard_normal((4, 40, 40, 1)), rng.standard_normal((4, 1))
    fn = nt_kernels.get_cnn_kernel(1, act="relu", w_std=1.2, b_std=0.3)
    with FittedPosterior(fn, ctx.to_device(x), ctx.to_device(y), ridge_abs=0.1, capacity=4) as post:
        with pytest.raises(NotImplementedError, match="1024"):
            post.predict_grad(x[:2])


def test_cnn_kernel_fn_input_grad(L, ctx):
    from smnngp import nt_kernels
    x1, x2, alpha, gbar, gdiag, _ = case(5, 7, 6, 6, 2, 3, "relu", 3, False, True)
    fn = nt_kernels.get_cnn_kernel(3, act="relu", **HYP)
    ref = X.cross_input_grad(x1, x2, 3, "relu", gbar=gbar, **HYP)
    got = fn.input_grad(x1, x2, gbar).raw_numpy()
    assert got.shape == x1.shape and worst_ratio(got, ref["gvar"], ref["svar"], 1e-9) <= 1.0
