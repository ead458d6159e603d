"""GPU tests of the predictive gradients: smn_kernel_mlp_input_grad and smn_fit_predict_grad (csrc/input_grad.hip, csrc/fit.hip),
KernelFn.input_grad and FittedPosterior.predict_grad, against the fp64 rules of tests/_input_grad_rules.py.

Metric: _tol.relerr_norm per output array (sums over N, outputs of solves).  Inputs are standard normal rows rounded to the
dtype under test (no near-duplicates; the singular cases below assert finiteness for every form and values for NNGP only),
hyper-parameters (1.3, 0.4, 0.9).  What a norm over a whole gx cannot see -- one wrong pair, F_2 beside F_1, near-duplicate,
duplicate and anti-parallel rows, where the NTK forms are held to the guarded rules' values -- is in test_gpu_input_probes.py,
which holds both kernel entries pair by pair to a long-double reference.

  fp64   relerr_norm <= 1e-8, the project's fp64 kernel tolerance (tests/_tol.py).
  fp32   the yardstick is the rules evaluated in float32 against float64 on the same inputs; the device's error is held to
         FP32_RATIO times it, and FP32_RATIO * yardstick may not exceed the project's fp32 kernel tolerance 2e-3.  FP32_RATIO
         = 4 x the largest ratio measured on an MI355X over the cases below, rounded up to a power of two (4 x because the
         inputs are a handful of seeds); the ratios per form are in profiles/r21_input_grad.txt.

Shapes: n1 in {1, 5, 129}, n2 in {3, 130, 257} (one partial tile, tile boundaries, three tile columns), d in {1, 7, 65}, every
operand inside a guarded window with a leading dimension above its extent; 0 / 1 / 3 layers; sparse over net x act x covariance x
dtype.  The posterior cases: N = 130, T = 150, capacity 64 (three chunks), c in {1, 3, 9} (the read-out's column groups)."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from _tol import relerr_norm  # noqa: E402
from _windows import in_window, out_window  # noqa: E402

import _input_grad_rules as R  # noqa: E402

W, B, LW = 1.3, 0.4, 0.9
NETS = {"mlp": 0, "resnet": 1}
TOL64 = 1e-8
FP32_TOL = 2e-3
FP32_RATIO = 16.0   # measured ratios up to 2.07 (profiles/r21_input_grad.txt): 4 x 2.07 = 8.3, rounded up to a power of two


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


# ----------------------------------------------------------------------------- 1. the kernel entry
ENTRY_CASES = [
    ("mlp", "relu", "nngp", 1, np.float32, 5, 130, 7), ("mlp", "erf", "ntk", 3, np.float32, 129, 257, 65),
    ("resnet", "relu", "ntk", 1, np.float64, 129, 130, 7), ("resnet", "erf", "nngp", 0, np.float64, 1, 3, 1),
    ("mlp", "relu", "ntk", 3, np.float64, 5, 257, 65), ("resnet", "relu", "nngp", 3, np.float32, 129, 3, 1),
    ("mlp", "erf", "nngp", 0, np.float32, 1, 257, 7), ("resnet", "erf", "ntk", 3, np.float32, 5, 130, 65),
    ("mlp", "relu", "nngp", 0, np.float64, 129, 257, 7), ("resnet", "relu", "ntk", 3, np.float32, 5, 257, 7),
    ("mlp", "erf", "nngp", 3, np.float64, 5, 130, 65), ("mlp", "relu", "ntk", 1, np.float32, 129, 130, 7),
]


@functools.lru_cache(maxsize=None)
def entry_data(n1, n2, d, f32):
    rng = np.random.default_rng(100 * n1 + 10 * n2 + d)
    dt = np.float32 if f32 else np.float64
    return tuple(_round(rng.standard_normal(s), dt) for s in ((n1, d), (n2, d), (n1, n2)))


def _entry_call(L, ctx, kind, act, get, layers, dtype, x1, x2, g, layout="aligned", b=B):
    n1, d = x1.shape
    n2 = x2.shape[0]
    w1, w2, wg = in_window(ctx, x1.astype(dtype), layout), in_window(ctx, x2.astype(dtype), layout), in_window(ctx, g.astype(dtype), layout)
    out = out_window(ctx, n1, d, dtype, layout)
    ctx.call("smn_kernel_mlp_input_grad", L.dtype_code(dtype), _net_code(L, kind, get), L.ACT[act], layers, W, b, LW, w1.ptr, n1,
             w1.ld, w2.ptr, n2, w2.ld, d, wg.ptr, wg.ld, out.ptr, out.ld)
    return out.result("gx_d")


@pytest.mark.parametrize("kind,act,get,layers,dtype,n1,n2,d", ENTRY_CASES)
def test_kernel_input_grad_equals_the_rules(L, ctx, kind, act, get, layers, dtype, n1, n2, d):
    x1, x2, g = entry_data(n1, n2, d, dtype == np.float32)
    layout = "unaligned" if (n1 + layers) % 2 else "aligned"
    got = _entry_call(L, ctx, kind, act, get, layers, dtype, x1, x2, g, layout)
    ref64 = R.input_grad(kind, x1, x2, g, get, **_hyp(layers, act))
    ref32 = R.input_grad(kind, x1, x2, g, get, dtype=np.float32, **_hyp(layers, act)) if dtype == np.float32 else None
    _check("entry %s %s %s L%d" % (kind, act, get, layers), got, ref64, ref32, dtype)
    again = _entry_call(L, ctx, kind, act, get, layers, dtype, x1, x2, g, layout)
    assert np.array_equal(got.view(np.uint8), again.view(np.uint8)), "two calls differ in bits"


# Every (net, act, covariance, dtype) form of the hot kernel at one small shape: n1 = 5, n2 = 130 (two column tiles: the
# tile-order row sums, padding on both sides), d = 7, two hidden layers (the ResNet takes its residual step and its last set).
# The fp32 ratios measured over these forms reach 1.24 (profiles/r31_input_tangent.txt).
ALL_FORMS = [(kind, act, get, dtype) for kind in ("mlp", "resnet") for act in ("relu", "erf") for get in ("nngp", "ntk")
             for dtype in (np.float32, np.float64)]


@pytest.mark.parametrize("kind,act,get,dtype", ALL_FORMS)
def test_every_form_of_the_entry_equals_the_rules(L, ctx, kind, act, get, dtype):
    x1, x2, g = entry_data(5, 130, 7, dtype == np.float32)
    got = _entry_call(L, ctx, kind, act, get, 2, dtype, x1, x2, g)
    ref64 = R.input_grad(kind, x1, x2, g, get, **_hyp(2, act))
    ref32 = R.input_grad(kind, x1, x2, g, get, dtype=np.float32, **_hyp(2, act)) if dtype == np.float32 else None
    _check("form %s %s %s %s" % (kind, act, get, np.dtype(dtype).name), got, ref64, ref32, dtype)
    again = _entry_call(L, ctx, kind, act, get, 2, dtype, x1, x2, g)
    assert np.array_equal(got.view(np.uint8), again.view(np.uint8)), "two calls differ in bits"


def test_kernel_fn_input_grad_defaults_to_the_covariance_mode(ctx):
    from smnngp import nt_kernels
    x1, x2, g = entry_data(5, 130, 7, False)
    fn = nt_kernels.get_dense_resnet_kernel(1, act="erf", w_std=W, b_std=B, last_w_std=LW).with_cov("ntk")
    got = fn.input_grad(x1, x2, g).raw_numpy()
    assert relerr_norm(got, R.input_grad("resnet", x1, x2, g, "ntk", **_hyp(1, "erf"))) <= TOL64
    got = fn.input_grad(x1, x2, g, get="nngp").raw_numpy()
    assert relerr_norm(got, R.input_grad("resnet", x1, x2, g, "nngp", **_hyp(1, "erf"))) <= TOL64


# ----------------------------------------------------------------------------- 2. the fitted posterior
N, T, D, CAP = 130, 150, 7, 64
RIDGE = {np.float64: 1e-3, np.float32: 1e-2}
POST_CASES = [
    ("mlp", "relu", "nngp", 1, np.float32, 1, "rel"), ("resnet", "erf", "ntk", 3, np.float64, 3, "abs"),
    ("mlp", "erf", "nngp", 3, np.float64, 9, "rel"), ("resnet", "relu", "ntk", 1, np.float32, 9, "abs"),
    ("mlp", "relu", "ntk", 3, np.float64, 1, "abs"), ("resnet", "relu", "nngp", 0, np.float32, 3, "rel"),
    ("mlp", "erf", "ntk", 1, np.float32, 3, "rel"), ("mlp", "relu", "nngp", 0, np.float64, 9, "abs"),
]


@functools.lru_cache(maxsize=None)
def post_data(c, f32):
    rng = np.random.default_rng(40 + c)
    dt = np.float32 if f32 else np.float64
    return tuple(_round(rng.standard_normal(s), dt) for s in ((N, D), (T, D), (N, c)))


@functools.lru_cache(maxsize=None)
def post_reference(kind, act, get, layers, c, f32, ridge_kind, as32):
    x, xt, y = post_data(c, f32)
    eps = RIDGE[np.float32 if f32 else np.float64]
    return R.predict_grad(kind, x, y, xt, get, diag_reg=eps, absolute=ridge_kind == "abs",
                          dtype=np.float32 if as32 else np.float64, **_hyp(layers, act))


class Fit:
    """A raw fused smn_fit handle."""

    def __init__(self, L, ctx, kind, act, get, layers, dtype, x, y, capacity, ridge_kind="rel", eps=None, b=B):
        self.L, self.ctx, self.dtype = L, ctx, np.dtype(dtype)
        self.xd, self.yd = ctx.to_device(np.ascontiguousarray(x, dtype=dtype)), ctx.to_device(np.ascontiguousarray(y, dtype=dtype))
        n, self.d = x.shape
        self.c = y.shape[1]
        eps = RIDGE[self.dtype.type] if eps is None else eps
        self.h, info = C.c_void_p(), C.c_int()
        ctx.call("smn_fit_create", L.dtype_code(dtype), _net_code(L, kind, get), L.ACT[act], layers, W, b, LW, self.xd.ptr, n, self.d,
                 self.d, self.yd.ptr, self.c, eps if ridge_kind == "rel" else 0.0, eps if ridge_kind == "abs" else 0.0, capacity,
                 C.byref(self.h), None, None, C.byref(info))
        self.info = info.value

    def predict(self, xt):
        xd = self.ctx.to_device(np.ascontiguousarray(xt, dtype=self.dtype))
        t = xd.shape[0]
        mean, var = self.ctx.empty((t, self.c), self.dtype), self.ctx.empty((t,), self.dtype)
        self.ctx.call_on("smn_fit_predict", self.h, xd.ptr, t, self.d, mean.ptr, var.ptr, None, t)
        return mean.raw_numpy(), var.raw_numpy()

    def predict_grad(self, xt, mean=True, var=True):
        """Through guarded windows: the inputs with ldxt > d, the outputs as blocks."""
        t = xt.shape[0]
        wx = in_window(self.ctx, np.ascontiguousarray(xt, dtype=self.dtype))
        om = out_window(self.ctx, t, self.c * self.d, self.dtype, "block") if mean else None
        ov = out_window(self.ctx, t, self.d, self.dtype, "block") if var else None
        self.ctx.call_on("smn_fit_predict_grad", self.h, wx.ptr, t, wx.ld, om.ptr if mean else None, ov.ptr if var else None)
        return (om.result("dmean_d").reshape(t, self.c, self.d) if mean else None), (ov.result("dvar_d") if var else None)

    def destroy(self):
        if self.h:
            self.ctx.call_on("smn_fit_destroy", self.h)
            self.h = None


@pytest.mark.parametrize("kind,act,get,layers,dtype,c,ridge_kind", POST_CASES)
def test_predict_grad_equals_the_rules(L, ctx, kind, act, get, layers, dtype, c, ridge_kind):
    f32 = dtype == np.float32
    x, xt, y = post_data(c, f32)
    f = Fit(L, ctx, kind, act, get, layers, dtype, x, y, CAP, ridge_kind)
    try:
        assert f.info == 0
        dmean, dvar = f.predict_grad(xt)
    finally:
        f.destroy()
    m64, v64 = post_reference(kind, act, get, layers, c, f32, ridge_kind, False)
    m32, v32 = post_reference(kind, act, get, layers, c, f32, ridge_kind, True) if f32 else (None, None)
    what = "posterior %s %s %s L%d c%d %s" % (kind, act, get, layers, c, ridge_kind)
    _check(what + " dmean", dmean, m64, m32, dtype)
    _check(what + " dvar", dvar, v64, v32, dtype)


# ----------------------------------------------------------------------------- 3. row independence, repeatability
@pytest.mark.parametrize("kind,act,get,dtype,c", [("mlp", "relu", "nngp", np.float32, 3), ("resnet", "erf", "ntk", np.float64, 1)])
def test_rows_do_not_depend_on_their_call(L, ctx, kind, act, get, dtype, c):
    """Rows predicted alone, across a chunk boundary, only one of the two outputs asked for, and by a state whose capacity
    holds all T rows, carry the bits of the chunked call; two calls give identical bits."""
    x, xt, y = post_data(c, dtype == np.float32)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint8)   # noqa: E731
    f = Fit(L, ctx, kind, act, get, 2, dtype, x, y, CAP)
    g = Fit(L, ctx, kind, act, get, 2, dtype, x, y, 256)
    try:
        dmean, dvar = f.predict_grad(xt)
        again = f.predict_grad(xt)
        assert np.array_equal(bits(dmean), bits(again[0])) and np.array_equal(bits(dvar), bits(again[1]))
        for rows in ([0], [63, 64], [149], list(range(60, 70))):
            m, v = f.predict_grad(xt[rows])
            assert np.array_equal(bits(m), bits(dmean[rows])) and np.array_equal(bits(v), bits(dvar[rows])), rows
        assert np.array_equal(bits(f.predict_grad(xt, var=False)[0]), bits(dmean))
        assert np.array_equal(bits(f.predict_grad(xt, mean=False)[1]), bits(dvar))
        m, v = g.predict_grad(xt)
        assert np.array_equal(bits(m), bits(dmean)) and np.array_equal(bits(v), bits(dvar))
    finally:
        f.destroy()
        g.destroy()


# ----------------------------------------------------------------------------- 4. consistency with the state's own predictions
@pytest.mark.parametrize("kind,act,get,layers,c", [("mlp", "relu", "nngp", 2, 3), ("resnet", "erf", "ntk", 1, 1)])
def test_fp64_gradients_are_the_slopes_of_the_states_own_predictions(L, ctx, kind, act, get, layers, c):
    """(predict(x + h v) - predict(x - h v)) / 2h against dmean . v and dvar . v, h = 1e-5, one random direction per row.
    Bound: 10 x what the same check gives for the rules against oracle.predict on the CPU at these inputs (printed; recorded in
    profiles/r21_input_grad.txt)."""
    x, xt, y = post_data(c, False)
    h = 1e-5
    v = np.random.default_rng(3).standard_normal(xt.shape)
    eps = RIDGE[np.float64]
    hyp = _hyp(layers, act)
    mu, vu = R.predict_mean_var(kind, x, y, xt + h * v, get, diag_reg=eps, **hyp)
    md, vd = R.predict_mean_var(kind, x, y, xt - h * v, get, diag_reg=eps, **hyp)
    rm, rv = R.predict_grad(kind, x, y, xt, get, diag_reg=eps, **hyp)
    cpu_m = relerr_norm(np.einsum("rke,re->rk", rm, v), (mu - md) / (2 * h))
    cpu_v = relerr_norm(np.einsum("re,re->r", rv, v), (vu - vd) / (2 * h))
    f = Fit(L, ctx, kind, act, get, layers, np.float64, x, y, CAP)
    try:
        dmean, dvar = f.predict_grad(xt)
        (mu, vu), (md, vd) = f.predict(xt + h * v), f.predict(xt - h * v)
    finally:
        f.destroy()
    dev_m = relerr_norm(np.einsum("rke,re->rk", dmean, v), (mu - md) / (2 * h))
    dev_v = relerr_norm(np.einsum("re,re->r", dvar, v), (vu - vd) / (2 * h))
    print("%s %s %s: slope check dmean device %.3g cpu %.3g, dvar device %.3g cpu %.3g" % (kind, act, get, dev_m, cpu_m, dev_v, cpu_v))
    assert dev_m <= 10 * cpu_m and dev_v <= 10 * cpu_v


# ----------------------------------------------------------------------------- 5. singular inputs
@pytest.mark.parametrize("kind,act,get", [("mlp", "relu", "nngp"), ("resnet", "relu", "ntk"), ("mlp", "erf", "nngp"), ("mlp", "relu", "ntk")])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_singular_inputs_give_finite_values(L, ctx, kind, act, get, dtype):
    """A test row bit-equal to a training row and an all-zero row with b_std = 0: every output finite, and the NNGP values
    equal the guarded fp64 rules to 4 sqrt(2 u) of the dtype, 6.0e-8 in fp64 and 1.4e-3 in fp32 (below the fp32 kernel tolerance
    2e-3) -- at c = 1 the factor sqrt((1 - c)(1 + c)) of phi_1 is known to sqrt(2 u) and no better once c carries one rounding
    error, in the rules as on the device.  Measured errors: profiles/r21_input_grad.txt."""
    f32 = dtype == np.float32
    x, xt, y = post_data(3, f32)
    xt = xt[:9].copy()
    xt[2] = x[5]
    xt[4] = 0.0
    g = entry_data(129, 130, 7, f32)[2][:9]
    got = _entry_call(L, ctx, kind, act, get, 2, dtype, xt, x, g, b=0.0)
    assert np.isfinite(got).all()
    f = Fit(L, ctx, kind, act, get, 2, dtype, x, y, CAP, b=0.0)
    try:
        dmean, dvar = f.predict_grad(xt)
    finally:
        f.destroy()
    assert np.isfinite(dmean).all() and np.isfinite(dvar).all()
    if get == "nngp":
        tol = 4 * np.sqrt(2 * 2.0 ** (-24 if f32 else -53))
        rm, rv = R.predict_grad(kind, x, y, xt, get, diag_reg=RIDGE[dtype], **_hyp(2, act, b=0.0))
        errs = (relerr_norm(got, R.input_grad(kind, xt, x, g, get, **_hyp(2, act, b=0.0))), relerr_norm(dmean, rm), relerr_norm(dvar, rv))
        print("singular %s %s %s: entry %.3g dmean %.3g dvar %.3g (bound %.3g)" % ((kind, act, np.dtype(dtype).name) + errs + (tol,)))
        assert max(errs) <= tol


# ----------------------------------------------------------------------------- 6. other contracts
def _last_error(L, ctx):
    buf = C.create_string_buffer(512)
    L._lib.smn_last_error(ctx.handle, buf, 512)
    return buf.value.decode()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_state_that_is_not_positive_definite_gives_nan_gradients(L, ctx, dtype):
    x, xt, y = post_data(3, dtype == np.float32)
    f = Fit(L, ctx, "mlp", "relu", "nngp", 1, dtype, x, y, CAP, "abs", eps=-50.0)
    try:
        assert f.info > 0
        dmean, dvar = f.predict_grad(xt[:70])             # SMN_OK, guards intact
        assert np.isnan(dmean).all() and np.isnan(dvar).all()
    finally:
        f.destroy()


def test_refusals_name_the_argument(L, ctx):
    x1, x2, g = entry_data(5, 130, 7, False)
    a, b, gd = ctx.to_device(x1), ctx.to_device(x2), ctx.to_device(g)
    out = ctx.empty((5, 7), np.float64)
    raw = L._lib.smn_kernel_mlp_input_grad
    good = dict(dtype=L.F64, net=0, act=0, layers=1, x2=b.ptr, ldx1=7, ldx2=7, ldg=130, ldgx=7)
    for change, word in ((dict(dtype=7), "dtype"), (dict(net=5), "net"), (dict(net=0x200), "net"), (dict(act=3), "act"),
                         (dict(x2=None), "x2_d"), (dict(ldx1=6), "ldx1"), (dict(ldx2=6), "ldx2"), (dict(ldg=129), "ldg"),
                         (dict(ldgx=6), "ldgx")):
        p = dict(good, **change)
        rc = raw(ctx.handle, p["dtype"], p["net"], p["act"], p["layers"], W, B, LW, a.ptr, 5, p["ldx1"], p["x2"], 130, p["ldx2"], 7,
                 gd.ptr, p["ldg"], out.ptr, p["ldgx"])
        assert rc == L.EINVAL and word in _last_error(L, ctx), (change, _last_error(L, ctx))
    x, xt, y = post_data(1, False)
    f = Fit(L, ctx, "mlp", "relu", "nngp", 1, np.float64, x, y, CAP)
    try:
        xd = ctx.to_device(xt)
        dm, dv = ctx.empty((T, 1, D), np.float64), ctx.empty((T, D), np.float64)
        raw = L._lib.smn_fit_predict_grad
        assert raw(f.h, None, T, D, dm.ptr, dv.ptr) == L.EINVAL and "xt_d" in _last_error(L, ctx)
        assert raw(f.h, xd.ptr, T, D, None, None) == L.EINVAL and "both NULL" in _last_error(L, ctx)
        assert raw(f.h, xd.ptr, 0, D, dm.ptr, dv.ptr) == L.EINVAL and "t = 0" in _last_error(L, ctx)
        assert raw(f.h, xd.ptr, T, D - 1, dm.ptr, dv.ptr) == L.EINVAL and "ldxt" in _last_error(L, ctx)
    finally:
        f.destroy()
    k = np.eye(8)
    h = C.c_void_p()
    yd = ctx.to_device(np.ones((8, 1)))
    ctx.call("smn_fit_create_from_kernel", L.F64, ctx.to_device(k).ptr, 8, 8, yd.ptr, 1, 0.0, 0.0, 4, C.byref(h), None, None, None)
    try:
        assert L._lib.smn_fit_predict_grad(h, yd.ptr, 1, 1, yd.ptr, None) == L.EINVAL and "kernel matrix" in _last_error(L, ctx)
    finally:
        ctx.call_on("smn_fit_destroy", h)


def test_fitted_posterior_predict_grad_in_model_units(ctx):
    """FittedPosterior.predict_grad: shapes, the rules' values, nbytes grown by the gradient state, closed -> ValueError."""
    from smnngp import nt_kernels
    from smnngp.posterior import FittedPosterior
    x, xt, y = post_data(3, False)
    fn = nt_kernels.get_mlp_kernel(1, act="relu", w_std=W, b_std=B, last_w_std=LW)
    post = FittedPosterior(fn, ctx.to_device(x), ctx.to_device(y), ridge_rel=1e-3, capacity=CAP, ctx=ctx)
    before = post.nbytes
    dmean, dvar = post.predict_grad(xt)
    assert dmean.shape == (T, 3, D) and dvar.shape == (T, D) and post.nbytes > before
    rm, rv = R.predict_grad("mlp", x, y, xt, "nngp", diag_reg=1e-3, **_hyp(1, "relu"))
    assert relerr_norm(dmean.raw_numpy(), rm) <= TOL64 and relerr_norm(dvar.raw_numpy(), rv) <= TOL64
    only_mean, none = post.predict_grad(xt[:5], var=False)
    assert none is None and np.array_equal(only_mean.raw_numpy(), dmean.raw_numpy()[:5])
    post.close()
    with pytest.raises(ValueError, match="closed"):
        post.predict_grad(xt)


import test_gpu_fit as TF  # noqa: E402  (the existing smn_fit_predict cases: their data, shapes, capacities, ridges and Fit)


@pytest.mark.parametrize("cap", TF.CAPS)
@pytest.mark.parametrize("shape", TF.SHAPES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["nngp", "ntk"])
@pytest.mark.parametrize("act", ["relu", "erf"])
@pytest.mark.parametrize("net", ["mlp", "resnet"])
def test_predictions_keep_their_bits_after_a_gradient_call(L, ctx, net, act, kind, dtype, shape, cap):
    """Every case of test_gpu_fit.py::test_fused_form_against_the_oracle, on its own data and state: the outputs of its two
    smn_fit_predict calls -- mean, var and (t <= capacity) the full covariance; then the mean alone -- carry the same bits before
    and after a smn_fit_predict_grad call (mean and variance gradients) on that state."""
    n, t, c = shape
    x, xt, y = TF.data(n, t, c, dtype == np.float32)
    f = TF.Fit(L, ctx, dtype, c, cap, x=x, y=y, net=net, act=act, ntk=kind == "ntk", eps=TF.RIDGE[dtype])
    try:
        assert f.info == 0
        calls = lambda: f.predict(xt, var=True, cov=t <= cap) + f.predict(xt, var=False, cov=False)[:1]   # noqa: E731
        before = calls()
        xd = ctx.to_device(np.ascontiguousarray(xt, dtype=dtype))
        dm, dv = ctx.empty((t, c, TF.D), dtype), ctx.empty((t, TF.D), dtype)
        ctx.call_on("smn_fit_predict_grad", f.h, xd.ptr, t, TF.D, dm.ptr, dv.ptr)
        assert np.isfinite(dm.raw_numpy()).all() and np.isfinite(dv.raw_numpy()).all()
        after = calls()
    finally:
        f.destroy()
    assert before[2] is not None or t > cap
    for a, b in zip(before, after):
        assert (a is None and b is None) or np.array_equal(a.view(np.uint8), b.view(np.uint8))
