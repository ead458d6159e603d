"""GPU tests of per-feature input scales (ARD) and of the log-marginal likelihood's gradient in the inputs:
smn_kernel_mlp_input_grad_sym, smn_spr_loss_grad_inputs and smn_scale_columns (csrc/input_grad_sym.hip), KernelFn / NNGPKernel /
NTKKernel input_scales, SPR / MultiSPR loss_and_grad and loss_input_grad, FittedPosterior under scales, and training, against the
rules of tests/_ard_rules.py (themselves checked against central differences of the oracle's log-pdf in test_ard_host.py).

Metric of the device entries: _tol.relerr_norm of gx and of feat (sums over N, seeds that are outputs of solves).
  fp64   relerr_norm <= 1e-8, the project's fp64 kernel tolerance (tests/_tol.py).
  fp32   the convention of test_gpu_input_grad.py: the yardstick is the rules evaluated in float32 against float64 on the same
         inputs; the device's error is held to FP32_RATIO times it, and FP32_RATIO * yardstick may not exceed the project's fp32
         kernel tolerance 2e-3.  FP32_RATIO = 4 x the largest ratio measured on an MI355X over the cases below, rounded up to a
         power of two; the ratios per form are in profiles/r26_ard.txt.

Shapes of the entry cases: n in {1, 5, 129, 257} (the pass works on 64 x 64 tiles of the lower triangle, the contraction on 128-row
tiles: one partial tile; several tile rows with off-diagonal tiles, so row-side and column-side partial sums both have more than
one slot), d in {1, 7, 65, 130} (130: two feature tiles in the contraction), c in {1, 3}, 0 / 1 / 3 layers, sparse over net x act x
covariance x dtype; every matrix operand inside a guarded window with a leading dimension above its extent, and the strict upper
triangle of -K~^-1 NaN (the lower triangle is what is read).  The singular cases below assert finiteness for every form and values
for NNGP only; test_gpu_input_probes.py holds smn_kernel_mlp_input_grad_sym pair by pair (every slot of the 64 x 64 pass, both
stores, both slot sides) to a long-double reference, the NTK forms at near-duplicate, duplicate and anti-parallel rows included."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from _tol import relerr_norm  # noqa: E402
from _windows import in_window, out_window  # noqa: E402

import _ard_rules as A  # noqa: E402

W, B, LW = 1.3, 0.4, 0.9
NETS = {"mlp": 0, "resnet": 1}
TOL64 = 1e-8
FP32_TOL = 2e-3
FP32_RATIO = 8.0   # measured ratios up to 1.88 (profiles/r26_ard.txt): 4 x 1.88 = 7.5, rounded up to a power of two
RIDGE = {np.float64: 1e-3, np.float32: 1e-2}
TA, TB = 1.7, 2.4   # the Student-t head's (a, b)


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


def _round(a, dtype):
    return np.asarray(a, dtype=dtype).astype(np.float64)


def _hyp(layers, act, b=B):
    return dict(num_hiddens=layers, act=act, w_std=W, b_std=b, last_w_std=LW)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _check(what, got, ref64, ref32, dtype):
    """fp64: the fixed tolerance; fp32: the device's error against FP32_RATIO x the rules' own float32 error."""
    err = relerr_norm(got, ref64)
    if np.dtype(dtype) == np.float64:
        print("%s: fp64 relerr_norm %.3g" % (what, err))
        assert err <= TOL64, what
        return
    yard = relerr_norm(ref32, ref64)
    print("%s: fp32 relerr_norm %.3g, yardstick %.3g, ratio %.3g" % (what, err, yard, err / yard))
    assert FP32_RATIO * yard <= FP32_TOL, "%s: the bound exceeds the fp32 kernel tolerance" % what
    assert err <= FP32_RATIO * yard, what


def _net_code(L, kind, get):
    return NETS[kind] | (L.NET_NTK if get == "ntk" else 0)


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


# ----------------------------------------------------------------------------- 1. the seeded entry
SYM_CASES = [
    ("mlp", "relu", "nngp", 1, np.float32, 5, 7, 1), ("mlp", "erf", "ntk", 3, np.float32, 129, 65, 3),
    ("resnet", "relu", "ntk", 1, np.float64, 129, 7, 1), ("resnet", "erf", "nngp", 0, np.float64, 1, 1, 1),
    ("mlp", "relu", "ntk", 3, np.float64, 257, 65, 3), ("resnet", "relu", "nngp", 3, np.float32, 257, 130, 1),
    ("mlp", "erf", "nngp", 0, np.float32, 1, 7, 3), ("resnet", "relu", "ntk", 3, np.float32, 5, 130, 1),
    ("mlp", "relu", "nngp", 0, np.float64, 257, 7, 3), ("resnet", "erf", "ntk", 1, np.float32, 5, 1, 3),
    ("mlp", "erf", "nngp", 3, np.float64, 5, 130, 1), ("mlp", "relu", "ntk", 1, np.float32, 257, 7, 1),
    ("resnet", "erf", "nngp", 1, np.float64, 129, 65, 3), ("mlp", "relu", "nngp", 3, np.float32, 129, 7, 3),
    ("mlp", "erf", "ntk", 1, np.float64, 129, 1, 1),
]
# (d = 1 makes every pair of points collinear, u_nm^2 = v_n v_m: beyond a handful of points the fp32 yardstick itself leaves the
# fp32 kernel tolerance, and ReLU sits on its singular points; so d = 1 runs at n = 5 in fp32 and with erf at n = 129 in fp64)


@functools.lru_cache(maxsize=None)
def sym_data(kind, act, get, layers, n, d, c, f32):
    """(x, -K~^-1, A, coef): inputs rounded to the dtype; the seed's parts from the fp64 rules on them, rounded to the dtype."""
    rng = np.random.default_rng(1000 * n + 10 * d + c)
    dt = np.float32 if f32 else np.float64
    x, y = _round(rng.standard_normal((n, d)), dt), rng.standard_normal((n, c))
    ninv, alpha, coef, _, _ = A.posterior_parts(kind, x, y, get, RIDGE[dt], "tp" if c == 3 else "gp", TA, TB, **_hyp(layers, act))
    return x, _round(ninv, dt), _round(alpha, dt), float(_round(coef, dt))


@functools.lru_cache(maxsize=None)
def sym_reference(kind, act, get, layers, n, d, c, f32, as32):
    x, ninv, alpha, coef = sym_data(kind, act, get, layers, n, d, c, f32)
    dt = np.float32 if as32 else np.float64
    return A.seed_input_grad(kind, x, A.g_matrix(ninv, alpha, coef, dt), get, dtype=dt, **_hyp(layers, act))


def _sym_call(L, ctx, kind, act, get, layers, dtype, x, ninv, alpha, coef, layout="aligned", b=B, want_gx=True, want_feat=True):
    """(gx or None, feat or None) of smn_kernel_mlp_input_grad_sym through guarded windows."""
    n, d = x.shape
    alpha = np.asarray(alpha).reshape(n, -1)
    c = alpha.shape[1]
    seed = np.array(ninv, dtype=dtype)
    seed[np.triu_indices(n, 1)] = np.nan
    wx, wk = in_window(ctx, x.astype(dtype), layout), in_window(ctx, seed, layout)
    wa = in_window(ctx, alpha.astype(dtype), "block")
    out = out_window(ctx, n, d, dtype, layout) if want_gx else None
    feat = np.full(d, 7.25)
    ctx.call("smn_kernel_mlp_input_grad_sym", L.dtype_code(dtype), _net_code(L, kind, get), L.ACT[act], layers, W, b, LW, wx.ptr, n,
             wx.ld, d, wk.ptr, wk.ld, wa.ptr, c, coef, out.ptr if want_gx else None, out.ld if want_gx else 0,
             _pd(feat) if want_feat else None)
    if not want_feat:
        assert (feat == 7.25).all()
    return (out.result("gx_d") if want_gx else None), (feat if want_feat else None)


@pytest.mark.parametrize("kind,act,get,layers,dtype,n,d,c", SYM_CASES)
def test_seeded_entry_equals_the_rules(L, ctx, kind, act, get, layers, dtype, n, d, c):
    f32 = dtype == np.float32
    x, ninv, alpha, coef = sym_data(kind, act, get, layers, n, d, c, f32)
    layout = "unaligned" if (n + layers) % 2 else "aligned"
    gx, feat = _sym_call(L, ctx, kind, act, get, layers, dtype, x, ninv, alpha, coef, layout)
    gx64, feat64 = sym_reference(kind, act, get, layers, n, d, c, f32, False)
    gx32, feat32 = sym_reference(kind, act, get, layers, n, d, c, f32, True) if f32 else (None, None)
    what = "sym %s %s %s L%d n%d d%d c%d" % (kind, act, get, layers, n, d, c)
    _check(what + " gx", gx, gx64, gx32, dtype)
    _check(what + " feat", feat, feat64, feat32, dtype)
    again = _sym_call(L, ctx, kind, act, get, layers, dtype, x, ninv, alpha, coef, layout)
    assert np.array_equal(_bits(gx), _bits(again[0])) and np.array_equal(_bits(feat), _bits(again[1])), "two calls differ in bits"
    only_gx, _ = _sym_call(L, ctx, kind, act, get, layers, dtype, x, ninv, alpha, coef, layout, want_feat=False)
    _, only_feat = _sym_call(L, ctx, kind, act, get, layers, dtype, x, ninv, alpha, coef, layout, want_gx=False)
    assert np.array_equal(_bits(gx), _bits(only_gx)), "feat_h = NULL changes gx"
    assert np.array_equal(_bits(feat), _bits(only_feat)), "gx_d = NULL changes feat"


# Every (net, act, covariance, dtype) form of the pass at one small shape: n = 129 (three 64-row tiles: both slot sides, and a
# padded 128-tile in the contraction), d = 7, c = 3, two hidden layers (the ResNet takes its residual step and its last set).
# Held to the file's FP32_RATIO as it stands; the fp32 ratios measured over these forms reach 2.47 (feat, resnet erf nngp;
# profiles/r31_input_tangent.txt), the same before and after the chain moved into csrc/input_tangent.hpp (the bits are equal).
ALL_FORMS = [(kind, act, get, dtype) for kind in ("mlp", "resnet") for act in ("relu", "erf") for get in ("nngp", "ntk")
             for dtype in (np.float32, np.float64)]


@pytest.mark.parametrize("kind,act,get,dtype", ALL_FORMS)
def test_every_form_of_the_seeded_entry_equals_the_rules(L, ctx, kind, act, get, dtype):
    f32 = dtype == np.float32
    x, ninv, alpha, coef = sym_data(kind, act, get, 2, 129, 7, 3, f32)
    gx, feat = _sym_call(L, ctx, kind, act, get, 2, dtype, x, ninv, alpha, coef)
    gx64, feat64 = sym_reference(kind, act, get, 2, 129, 7, 3, f32, False)
    gx32, feat32 = sym_reference(kind, act, get, 2, 129, 7, 3, f32, True) if f32 else (None, None)
    what = "form %s %s %s %s" % (kind, act, get, np.dtype(dtype).name)
    _check(what + " gx", gx, gx64, gx32, dtype)
    _check(what + " feat", feat, feat64, feat32, dtype)
    again = _sym_call(L, ctx, kind, act, get, 2, dtype, x, ninv, alpha, coef)
    assert np.array_equal(_bits(gx), _bits(again[0])) and np.array_equal(_bits(feat), _bits(again[1])), "two calls differ in bits"


# ----------------------------------------------------------------------------- 2. singular points
@pytest.mark.parametrize("kind,get", [("mlp", "nngp"), ("resnet", "ntk"), ("mlp", "ntk"), ("resnet", "nngp")])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_singular_inputs_give_finite_values(L, ctx, kind, get, dtype):
    """Two exactly equal rows in different tiles and an all-zero row with b_std = 0, ReLU, under a random symmetric seed (coef =
    0, a zero alpha: the seed is the matrix itself): every output finite, and the NNGP values equal the guarded fp64 rules to
    4 sqrt(2 u) of the dtype (test_gpu_input_grad.py: at c = 1 the factor sqrt((1 - c)(1 + c)) is known to sqrt(2 u) and no
    better, in the rules as on the device)."""
    f32 = dtype == np.float32
    n, d = 130, 7
    rng = np.random.default_rng(77)
    x = _round(rng.standard_normal((n, d)), dtype)
    x[100] = x[5]
    x[70] = 0.0
    g = rng.standard_normal((n, n))
    g = _round(g + g.T, dtype)
    gx, feat = _sym_call(L, ctx, kind, "relu", get, 2, dtype, x, g, np.zeros((n, 1)), 0.0, b=0.0)
    assert np.isfinite(gx).all() and np.isfinite(feat).all()
    if get == "nngp":
        tol = 4 * np.sqrt(2 * 2.0 ** (-24 if f32 else -53))
        rx, rf = A.seed_input_grad(kind, x, g, get, **_hyp(2, "relu", b=0.0))
        errs = (relerr_norm(gx, rx), relerr_norm(feat, rf))
        print("singular %s %s: gx %.3g feat %.3g (bound %.3g)" % ((kind, np.dtype(dtype).name) + errs + (tol,)))
        assert max(errs) <= tol


# ----------------------------------------------------------------------------- 3. reproducibility
@pytest.mark.parametrize("case", [SYM_CASES[5], SYM_CASES[4]])
def test_rows_do_not_depend_on_leading_dimensions_or_earlier_calls(L, ctx, case):
    kind, act, get, layers, dtype, n, d, c = case
    assert n == 257
    f32 = dtype == np.float32
    x, ninv, alpha, coef = sym_data(kind, act, get, layers, n, d, c, f32)
    gx, feat = _sym_call(L, ctx, kind, act, get, layers, dtype, x, ninv, alpha, coef, "aligned")
    small = sym_data(kind, act, get, layers, 5, 7, 1, f32)
    _sym_call(L, ctx, kind, act, get, layers, dtype, *small)                  # another shape on the same context in between
    gx2, feat2 = _sym_call(L, ctx, kind, act, get, layers, dtype, x, ninv, alpha, coef, "unaligned")
    assert np.array_equal(_bits(gx), _bits(gx2)) and np.array_equal(_bits(feat), _bits(feat2))


# ----------------------------------------------------------------------------- 4. the fused entry
FN, FD_ = 130, 7
FUSED_NETS = {1: ("mlp", "relu", "nngp"), 3: ("resnet", "erf", "ntk")}


@functools.lru_cache(maxsize=None)
def fused_data(c, f32):
    rng = np.random.default_rng(500 + c)
    dt = np.float32 if f32 else np.float64
    return _round(rng.standard_normal((FN, FD_)), dt), _round(rng.standard_normal((FN, c)), dt)


def _fused_call(L, ctx, name, dtype, net, act, x, y, eps, df, scale, inputs):
    n, d = x.shape
    c = y.shape[1]
    xd, yd = ctx.to_device(x.astype(dtype)), ctx.to_device(y.astype(dtype))
    quad, logdet, info = C.c_double(), C.c_double(), C.c_int()
    cols, terms = np.zeros(c), (C.c_double * 4)()
    head = (L.dtype_code(dtype), net, act, 2, W, B, LW, xd.ptr, n, d, d, yd.ptr, c, eps, df, scale, C.byref(quad), _pd(cols),
            C.byref(logdet), C.byref(info), terms)
    if not inputs:
        ctx.call(name, *head)
        return quad.value, cols, logdet.value, info.value, np.array(terms[:]), None, None
    out, feat = out_window(ctx, n, d, dtype), np.full(d, 7.25)
    ctx.call(name, *head, out.ptr, out.ld, _pd(feat))
    return quad.value, cols, logdet.value, info.value, np.array(terms[:]), out, feat


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("c", [1, 3])
def test_fused_entry_is_the_gradient_entry_followed_by_the_seeded_one(L, ctx, c, method, dtype):
    f32 = dtype == np.float32
    kind, act, get = FUSED_NETS[c]
    x, y = fused_data(c, f32)
    net, eps = _net_code(L, kind, get), RIDGE[dtype]
    df, scale = (2 * TA, TB / TA) if method == "tp" else (0.0, 1.0)
    ref = _fused_call(L, ctx, "smn_spr_loss_grad_multi", dtype, net, L.ACT[act], x, y, eps, df, scale, False)
    got = _fused_call(L, ctx, "smn_spr_loss_grad_inputs", dtype, net, L.ACT[act], x, y, eps, df, scale, True)
    assert ref[3] == 0 and got[3] == 0
    for a, b in zip(ref[:5], got[:5]):
        assert np.array_equal(_bits(np.asarray(a, dtype=np.float64)), _bits(np.asarray(b, dtype=np.float64)))
    gx, feat = got[5].result("gx_d"), got[6]
    # the seeded entry fed smn_spr_kinv's outputs and the head's coef (internal.hpp lml_coef, operation by operation)
    xd, yd = ctx.to_device(x.astype(dtype)), ctx.to_device(y.astype(dtype))
    ld = 132
    ninv, alpha = ctx.empty((FN, ld), dtype), ctx.empty((FN, c), dtype)
    ctx.call("smn_spr_kinv", L.dtype_code(dtype), net, L.ACT[act], 2, W, B, LW, xd.ptr, FN, FD_, FD_, yd.ptr, c, eps, ninv.ptr, ld,
             alpha.ptr, None, None)
    coef = (df + float(FN) * float(c)) / ((df + got[0] / scale) * scale) if df > 0.0 else 1.0
    out, feat2 = ctx.empty((FN, FD_), dtype), np.zeros(FD_)
    ctx.call("smn_kernel_mlp_input_grad_sym", L.dtype_code(dtype), net, L.ACT[act], 2, W, B, LW, xd.ptr, FN, FD_, FD_, ninv.ptr, ld,
             alpha.ptr, c, coef, out.ptr, FD_, _pd(feat2))
    assert np.array_equal(_bits(gx), _bits(out.raw_numpy())) and np.array_equal(_bits(feat), _bits(feat2))
    # (the values against the rules on the same data are printed, not asserted: they go through a factorisation in the dtype,
    # which the model tests below hold to the models' tolerances)
    rx, rf = A.lml_input_grad(kind, x, y, get, eps=eps, method=method, a=TA, b=TB, **_hyp(2, act))
    print("fused %s c%d %s: relerr_norm gx %.3g feat %.3g" % (method, c, np.dtype(dtype).name, relerr_norm(gx, rx), relerr_norm(feat, rf)))


def test_fused_entry_reports_a_matrix_that_is_not_positive_definite(L, ctx):
    x, y = fused_data(1, True)
    x = x.copy()
    x[9] = x[3]
    got = _fused_call(L, ctx, "smn_spr_loss_grad_inputs", np.float32, 0, L.ACT["relu"], x, y, 0.0, 0.0, 1.0, True)
    assert got[3] != 0 and np.isnan(got[0]) and np.isnan(got[4]).all()
    got[5].result("gx_d")                      # the guard check; and the window itself still holds its pattern
    assert np.array_equal(_bits(got[5].inside(got[5].download())), _bits(got[5].initial()))
    assert (got[6] == 7.25).all()


# ----------------------------------------------------------------------------- 5. the models
HYP = dict(w_std=1.3, b_std=0.4, last_w_std=0.9, eps=5e-2, alpha=1.7, beta=2.4)   # test_gpu_cnn_grad.py's
MN, MD, MC, MLAYERS = 40, 5, 3, 2


@functools.lru_cache(maxsize=None)
def model_data(multi):
    """(x, y, s, x_test, y_test), every array exact in float32 (one reference serves both dtypes)."""
    rng = np.random.default_rng(31 + multi)
    c = MC if multi else 1
    x, xt = _round(rng.standard_normal((MN, MD)), np.float32), _round(rng.standard_normal((9, MD)), np.float32)
    y, yt = _round(rng.standard_normal((MN, c)), np.float32), _round(rng.standard_normal((9, c)), np.float32)
    s = _round(np.exp(0.5 * rng.standard_normal(MD)), np.float32)
    return x, (y if multi else y[:, 0]), s, xt, (yt if multi else yt[:, 0])


def make_model(multi, kind, get, act, method, dtype, x, y, scales, hyp=HYP):
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NNGPKernel, NTKKernel
    from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood
    from smnngp.spax.models import SPR, MultiSPR
    factory = nt_kernels.get_mlp_kernel if kind == "mlp" else nt_kernels.get_dense_resnet_kernel
    kernel = (NTKKernel if get == "ntk" else NNGPKernel)(
        lambda w, b, l: factory(MLAYERS, act=act, w_std=w, b_std=b, last_w_std=l), hyp["w_std"], hyp["b_std"], hyp["last_w_std"],
        input_scales=scales)
    lik = GaussianLikelihood() if method == "gp" else StudentTLikelihood(hyp["alpha"], hyp["beta"])
    model = (MultiSPR if multi else SPR)(kernel, lik, np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype), 0.0, 1.0, eps=hyp["eps"])
    vmap = {"w_std": kernel.w_std, "b_std": kernel.b_std, "last_w_std": kernel.last_w_std, "eps": model.eps}
    if method == "tp":
        vmap.update(alpha=lik.a, beta=lik.b)
    return model, vmap


def _ref_loss(multi, kind, get, act, method, s=None, x=None, **over):
    x0, y, s0 = model_data(multi)[:3]
    h = dict(HYP, **over)
    return A.loss(kind, x0 if x is None else x, s0 if s is None else s, y, get, eps=h["eps"], method=method, a=h["alpha"],
                  b=h["beta"], **_hyp(MLAYERS, act) | dict(w_std=h["w_std"], b_std=h["b_std"], last_w_std=h["last_w_std"]))


@functools.lru_cache(maxsize=None)
def model_reference(multi, kind, get, act, method):
    """(loss, {scalar key: d loss / d constrained value}, d loss / d s [d]) by central differences of the oracle loss on x * s:
    relative step 1e-5 for the scalars (_multi_rules.loss_fd), 1e-6 s_j for the scales."""
    x, y, s = model_data(multi)[:3]
    keys = ("w_std", "b_std", "last_w_std", "eps") + (("alpha", "beta") if method == "tp" else ())
    fd = {}
    for k in keys:
        step = 1e-5 * HYP[k]
        fd[k] = (_ref_loss(multi, kind, get, act, method, **{k: HYP[k] + step})
                 - _ref_loss(multi, kind, get, act, method, **{k: HYP[k] - step})) / (2 * step)
    ds = np.empty(MD)
    for j in range(MD):
        up, dn = s.copy(), s.copy()
        up[j] += 1e-6 * s[j]
        dn[j] -= 1e-6 * s[j]
        ds[j] = (_ref_loss(multi, kind, get, act, method, s=up) - _ref_loss(multi, kind, get, act, method, s=dn)) / (2e-6 * s[j])
    return _ref_loss(multi, kind, get, act, method), fd, ds


@functools.lru_cache(maxsize=None)
def input_reference(multi, kind, get, act, method):
    """d loss / d x [N, d] by central differences (step 1e-6) of the oracle loss on x * s, at all N d entries."""
    x = model_data(multi)[0]
    out = np.empty_like(x)
    for i in range(MN):
        for j in range(MD):
            up, dn = x.copy(), x.copy()
            up[i, j] += 1e-6
            dn[i, j] -= 1e-6
            out[i, j] = (_ref_loss(multi, kind, get, act, method, x=up) - _ref_loss(multi, kind, get, act, method, x=dn)) / 2e-6
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("act", ["relu", "erf"])
@pytest.mark.parametrize("get", ["nngp", "ntk"])
@pytest.mark.parametrize("kind", ["mlp", "resnet"])
@pytest.mark.parametrize("multi", [False, True])
def test_model_gradients_match_central_differences_of_the_oracle(multi, kind, get, act, method, dtype):
    """check_against_reference's measure and tolerances (test_gpu_cnn_grad.py): 2e-6 (fp64) / 1e-2 (fp32) of max(largest
    reference gradient, |reference|), over the scalar variables AND every component of input_scales together."""
    f64 = dtype == np.float64
    x, y, s = model_data(multi)[:3]
    model, vmap = make_model(multi, kind, get, act, method, dtype, x, y, s)
    loss, grads = model.loss_and_grad()
    rl, fd, ds = model_reference(multi, kind, get, act, method)
    tol = 2e-6 if f64 else 1e-2
    assert abs(loss - rl) < (1e-9 if f64 else 1e-3) * max(1.0, abs(rl))
    assert abs(loss - model.loss()) < (1e-10 if f64 else 1e-4) * max(1.0, abs(rl))
    assert set(grads) == set(model.vars())
    names = {id(v): k for k, v in model.vars().items()}
    scale = max(max(abs(v) for v in fd.values()), float(np.abs(ds).max()))
    worst = 0.0
    for k, ref in fd.items():
        var = vmap[k]
        got = grads[names[id(var)]] / float(var.constraint.grad(var.value))     # undo the softplus chain rule
        err = abs(got - ref) / max(scale, abs(ref))
        worst = max(worst, err)
        assert err < tol, (k, got, ref)
    var = model.kernel.input_scales
    got = np.asarray(grads[names[id(var)]]) / var.constraint.grad(var.value)
    assert got.shape == (MD,) and np.isfinite(got).all()
    err = float(np.max(np.abs(got - ds) / np.maximum(scale, np.abs(ds))))
    print("model %s %s %s %s %s %s: scalars %.3g scales %.3g (tol %g)" % ("multi" if multi else "spr", kind, get, act, method,
                                                                          np.dtype(dtype).name, worst, err, tol))
    assert err < tol, (got, ds)
    if f64:
        loss2, gx = model.loss_input_grad()
        ref = input_reference(multi, kind, get, act, method)
        got = gx.raw_numpy()
        assert got.shape == (MN, MD) and abs(loss2 - loss) <= 1e-12 * max(1.0, abs(loss))
        err = float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref).max(), np.abs(ref))))
        print("  loss_input_grad: %.3g" % err)
        assert err < tol


def test_loss_input_grad_without_scales(ctx):
    x, y, s = model_data(False)[:3]
    model, _ = make_model(False, "mlp", "nngp", "relu", "tp", np.float64, x * s, y, None)
    loss, gx = model.loss_input_grad()
    ref = input_reference(False, "mlp", "nngp", "relu", "tp") / s     # d/d(x s) = (d/dx) / s
    assert abs(loss - model.loss()) <= 1e-10 * max(1.0, abs(loss))
    assert float(np.max(np.abs(gx.raw_numpy() - ref) / np.maximum(np.abs(ref).max(), np.abs(ref)))) < 2e-6


# ----------------------------------------------------------------------------- 6. bits
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("method", ["gp", "tp"])
def test_all_ones_scales_give_the_unscaled_models_bits(method, dtype):
    x, y, _, xt, yt = model_data(False)
    plain, _ = make_model(False, "mlp", "nngp", "relu", method, dtype, x, y, None)
    ones, _ = make_model(False, "mlp", "nngp", "relu", method, dtype, x, y, np.ones(MD))
    assert plain.loss() == ones.loss()
    (l0, g0), (l1, g1) = plain.loss_and_grad(), ones.loss_and_grad()
    assert l0 == l1 and set(g1) - set(g0) == {"(SPR).kernel(NNGPKernel).input_scales"}
    for k, v in g0.items():
        assert np.array_equal(_bits(np.float64(v)), _bits(np.float64(g1[k]))), k
    for a, b in zip(plain.predict(xt), ones.predict(xt)):
        assert np.array_equal(_bits(a.raw_numpy()), _bits(b.raw_numpy()))
    assert plain.test_nll(xt, yt) == ones.test_nll(xt, yt)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("multi,kind,get,act,method", [(False, "mlp", "nngp", "relu", "tp"), (True, "resnet", "ntk", "erf", "gp"),
                                                       (False, "resnet", "nngp", "erf", "gp"), (True, "mlp", "ntk", "relu", "tp")])
def test_scaled_models_are_the_unscaled_models_on_prescaled_inputs(multi, kind, get, act, method, dtype):
    x, y, s, xt, yt = model_data(multi)
    scaled, _ = make_model(multi, kind, get, act, method, dtype, x, y, s)
    # the model's scales are the constrained values of its variable, softplus(softplus^-1(s)): s up to an ulp in fp64
    sd = scaled.kernel.get_input_scales().astype(dtype)
    pre = lambda a: np.asarray(a, dtype=dtype) * sd     # noqa: E731  (the product in the storage dtype)
    plain, _ = make_model(multi, kind, get, act, method, dtype, pre(x), y, None)
    same = lambda a, b: np.array_equal(_bits(a.raw_numpy()), _bits(b.raw_numpy()))   # noqa: E731
    assert scaled.loss() == plain.loss()
    assert all(same(a, b) for a, b in zip(scaled.predict(xt.astype(dtype)), plain.predict(pre(xt))))
    assert scaled.test_nll(xt.astype(dtype), yt) == plain.test_nll(pre(xt), yt)
    assert scaled.loo_loss() == plain.loo_loss()
    assert same(scaled.sample_posterior(3, xt.astype(dtype), 4, jitter=1e-3), plain.sample_posterior(3, pre(xt), 4, jitter=1e-3))
    if multi:
        assert np.array_equal(scaled.classify(xt.astype(dtype)), plain.classify(pre(xt)))
    fs, fp = scaled.kernel.get_kernel_fn(), plain.kernel.get_kernel_fn()
    assert same(fs(x.astype(dtype), xt.astype(dtype), get=get), fp(pre(x), pre(xt), get=get))
    ps, pp = scaled.posterior(capacity=64), plain.posterior(capacity=64)
    try:
        assert all(same(a, b) for a, b in zip(ps.predict(xt.astype(dtype)), pp.predict(pre(xt))))
        assert ps.test_nll(xt.astype(dtype), yt) == pp.test_nll(pre(xt), yt)
        gs, gp = ps.predict_grad(xt.astype(dtype)), pp.predict_grad(pre(xt))
        assert np.array_equal(_bits(gs[0].raw_numpy()), _bits(gp[0].raw_numpy() * sd))       # s o the prescaled model's gradient
        assert np.array_equal(_bits(gs[1].raw_numpy()), _bits(gp[1].raw_numpy() * sd))
        ps.append(xt[:4].astype(dtype), yt[:4])
        pp.append(pre(xt[:4]), yt[:4])
        assert all(same(a, b) for a, b in zip(ps.predict(xt[4:].astype(dtype)), pp.predict(pre(xt[4:]))))
        assert np.array_equal(np.asarray(ps.x_train)[:MN], x.astype(dtype))                  # x_train: what was handed in
    finally:
        ps.close()
        pp.close()


# ----------------------------------------------------------------------------- 7. training
def test_training_the_scales_finds_the_relevant_features():
    """The issue's case: y depends on features 0 and 1 of 6; 40 Adam steps on input_scales alone from all-ones, Student-t
    2-layer ReLU NNGP in fp64.  Every step returns model.loss() before the step; the loss falls by at least half of what
    the rules reach under the same procedure on the CPU; the relevant scales end above twice the irrelevant ones."""
    from smnngp.spax.base import ConstraintTrainVar
    from smnngp.spax.bijectors import positive
    from smnngp.train import Adam, build_train_step
    rng = np.random.default_rng(0)
    x = rng.standard_normal((48, 6))
    y = np.sin(2 * x[:, 0]) + 0.5 * x[:, 1] + 0.05 * rng.standard_normal(48)
    hyp = dict(w_std=1.3, b_std=0.4, last_w_std=0.9, eps=5e-2, alpha=1.7, beta=2.4)
    model, _ = make_model(False, "mlp", "nngp", "relu", "tp", np.float64, x, y, np.ones(6), hyp)
    name = "(SPR).kernel(NNGPKernel).input_scales"
    step = build_train_step(model, variables={name: model.kernel.input_scales})
    before = model.vars()
    kept = {k: np.array(v.value) for k, v in before.items() if k != name}
    losses = []
    for _ in range(40):
        expect = model.loss()
        losses.append(step(0.05))
        assert abs(losses[-1] - expect) <= 1e-10 * max(1.0, abs(expect))
    final = model.loss()
    assert all(np.array_equal(kept[k], before[k].value) for k in kept)          # only the scales moved
    # the same procedure on the rules
    rules = dict(eps=5e-2, method="tp", a=1.7, b=2.4, **_hyp(MLAYERS, "relu"))
    var = ConstraintTrainVar(np.ones(6), positive())
    opt = Adam({"s": var})
    for _ in range(40):
        sv = var.constraint(var.value)
        _, feat = A.lml_input_grad("mlp", x * sv, y, "nngp", **rules)
        opt(0.05, {"s": -(feat / sv) / 48 * var.constraint.grad(var.value)})
    r0, r1 = A.loss("mlp", x, np.ones(6), y, "nngp", **rules), A.loss("mlp", x, var.constraint(var.value), y, "nngp", **rules)
    s = model.kernel.get_input_scales()
    print("training: device loss %.4f -> %.4f, rules %.4f -> %.4f, scales %s" % (losses[0], final, r0, r1, np.round(s, 3)))
    assert losses[0] - final >= 0.5 * (r0 - r1) > 0.0
    assert min(s[0], s[1]) > 2.0 * max(s[2:])
