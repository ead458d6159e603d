"""GPU tests of the conv-NNGP analytic gradient: SPR.loss_and_grad with get_cnn_kernel (csrc/cnn_grad.hip) against
central differences of the fp64 reference loss, the contraction alone against the NumPy forward-mode rules
(tests/_cnn_grad_rules.py), the edge cases of the C ABI and the training step.  No wall-clock assertion anywhere."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import nngp_oracle as O  # noqa: E402  (test infrastructure only)

import _cnn_grad_rules as R  # noqa: E402

HYP = dict(w_std=1.3, b_std=0.4, last_w_std=0.9, eps=5e-2, alpha=1.7, beta=2.4)
# the issue's shapes, then one more per form the launcher can pick that they do not reach (4 pixels per lane, ragged and
# exact; 16 pixels per lane, ragged)
SHAPES = [(24, 6, 6, 2, 3), (20, 5, 7, 3, 2), (12, 8, 8, 1, 4), (12, 32, 32, 3, 2), (12, 32, 32, 1, 4),
          (12, 12, 12, 1, 2), (12, 16, 16, 2, 2), (10, 20, 20, 1, 2)]
# for the contraction alone: a ragged 4-per-lane image whose row stride does not divide 64 (the dummy slot of the wave's LDS
# map), and the two most elongated images the pixel limit admits, whose padded maps are the largest (the per-image pass
# needs 153 888 bytes of LDS there)
MAP_SHAPES = [(6, 3, 50, 1, 2), (5, 1, 1024, 1, 2), (5, 1024, 1, 2, 2)]


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


def make_model(x, y, layers, act, method, dtype, hyp=HYP):
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood
    from smnngp.spax.models import SPR
    with np.errstate(divide="ignore"):      # b_std = 0 is stored as raw = -inf (softplus-inverse of 0)
        kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_cnn_kernel(layers, 1, act=act, w_std=w, b_std=b, last_w_std=l),
                            hyp["w_std"], hyp["b_std"], hyp["last_w_std"])
    lik = GaussianLikelihood() if method == "gp" else StudentTLikelihood(hyp["alpha"], hyp["beta"])
    model = SPR(kernel, lik, x.astype(dtype), y.astype(dtype), 0.0, 1.0, eps=hyp["eps"])
    vmap = {"w_std": kernel.w_std, "b_std": kernel.b_std, "last_w_std": kernel.last_w_std, "eps": model.eps}
    if method == "tp":
        vmap.update(alpha=lik.a, beta=lik.b)
    return model, vmap


def keys_of(method):
    return ("w_std", "b_std", "last_w_std", "eps") + (("alpha", "beta") if method == "tp" else ())


def check_against_reference(model, vmap, x, y, layers, act, method, dtype, hyp, skip=()):
    """Test 4's comparison: gradients 2e-6 (fp64) / 1e-2 (fp32) of max(largest reference gradient, |reference|), loss
    against the reference 1e-9 / 1e-3, against model.loss() 1e-10 / 1e-4 (tests/test_gpu_parity.py:1251-1263)."""
    f64 = dtype == np.float64
    loss, grads = model.loss_and_grad()
    keys = keys_of(method)
    ref = R.ref_grad_fd(x, y, layers, act, method, keys, **hyp)
    rl = R.ref_loss(x, y, layers, act, method, **hyp)
    tol = 2e-6 if f64 else 1e-2
    print("loss %.15g reference %.15g model.loss %.15g" % (loss, rl, model.loss()))
    assert abs(loss - rl) < (1e-9 if f64 else 1e-3) * max(1.0, abs(rl))
    assert abs(loss - model.loss()) < (1e-10 if f64 else 1e-4) * max(1.0, abs(rl))
    assert set(grads) == set(model.vars())
    names = {id(v): k for k, v in model.vars().items()}
    scale = max(abs(v) for v in ref.values())
    for k in keys:
        var = vmap[k]
        assert np.isfinite(grads[names[id(var)]])
        if k in skip:
            continue
        got = grads[names[id(var)]] / float(var.constraint.grad(var.value))     # undo the softplus chain rule
        err = abs(got - ref[k]) / max(scale, abs(ref[k]))
        print("%s got %.12g ref %.12g err %.3g (tol %g)" % (k, got, ref[k], err, tol))
        assert err < tol, (k, got, ref[k])
    return loss, grads


def data(n, h, w, c, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, h, w, c))
    y = np.sin(x[:, 0, 0, 0]) + 0.3 * rng.standard_normal(n)
    return x, y


# ----------------------------------------------------------------------------- 4. loss_and_grad against the reference
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("act", ["relu", "erf"])
@pytest.mark.parametrize("n,h,w,c,layers", SHAPES)
def test_conv_loss_and_grad_matches_finite_differences_of_the_reference(n, h, w, c, layers, act, method, dtype):
    x, y = data(n, h, w, c, 100 * n + layers)
    x = x.astype(dtype).astype(np.float64)      # the reference sees the values the device sees
    y = y.astype(dtype).astype(np.float64)
    model, vmap = make_model(x, y, layers, act, method, dtype)
    check_against_reference(model, vmap, x, y, layers, act, method, dtype, HYP)


# ----------------------------------------------------------------------------- 6. the contraction alone
def device_terms(L, ctx, x, layers, act, hyp, nkinv, al, coef, dtype=np.float64):
    n, h, w, c = x.shape
    xd = ctx.to_device(np.ascontiguousarray(x, dtype=dtype))
    kd = ctx.to_device(np.ascontiguousarray(nkinv, dtype=dtype))
    ad = ctx.to_device(np.ascontiguousarray(al, dtype=dtype))
    terms = (C.c_double * 4)()
    ctx.call("smn_kernel_cnn_grad_terms", L.dtype_code(dtype), L.ACT[act], layers, hyp["w_std"], hyp["b_std"],
             hyp["last_w_std"], xd.ptr, n, h, w, c, kd.ptr, n, ad.ptr, coef, terms)
    return np.array(list(terms))


@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("act", ["relu", "erf"])
@pytest.mark.parametrize("n,h,w,c,layers", SHAPES + MAP_SHAPES)
def test_contraction_alone_against_the_numpy_rules(L, ctx, n, h, w, c, layers, act, method):
    """smn_kernel_cnn_grad_terms fed -K~^-1 and alpha computed in NumPy, fp64: each term within 1e-9 * sum |G| |dK/d theta|
    -- the forward conv kernel's per-entry bound (1e-9 relative, tests/test_golden.py:108) carried through a sum whose
    terms may cancel; not a bound relative to the result."""
    x, y = data(n, h, w, c, 7 * n + layers)
    k, kw, kb = R.tangent_matrices(x, layers, act, HYP["w_std"], HYP["b_std"], HYP["last_w_std"])
    g, al, nkinv, coef = R.g_matrix(k, y, HYP["eps"], method, HYP["alpha"], HYP["beta"])[:4]
    ref, bound = R.terms_from(g, k, kw, kb, HYP["w_std"], HYP["b_std"], HYP["last_w_std"])
    got = device_terms(L, ctx, x, layers, act, HYP, nkinv, al, coef)
    for i in range(4):
        print("term %d got %.15g ref %.15g err %.3g bound %.3g" % (i, got[i], ref[i], abs(got[i] - ref[i]), 1e-9 * bound[i]))
        assert abs(got[i] - ref[i]) <= 1e-9 * bound[i], (i, got[i], ref[i])


# ----------------------------------------------------------------------------- 5. the XCD-tiled pair order
def test_contraction_in_the_tiled_pair_order_is_right_and_reproducible(L, ctx):
    """n = 1531 images of 6x6x1 (1.17 M pairs; the launcher's threshold is 256 pairs per resident workgroup, at most
    524288): the tiled pair order with ragged last tiles and half-empty diagonal tiles.  Checked as the contraction
    alone, the NumPy rules evaluated in row blocks of 128 images; a second call returns the same bits."""
    n, h, w, c, layers, act = 1531, 6, 6, 1, 2, "relu"
    hyp = dict(HYP, w_std=1.3, b_std=0.2, last_w_std=0.9)
    x, y = data(n, h, w, c, 3)
    k, kw, kb = R.tangent_matrices(x, layers, act, hyp["w_std"], hyp["b_std"], hyp["last_w_std"], block=128)
    g, al, nkinv, coef = R.g_matrix(k, y, hyp["eps"], "tp", hyp["alpha"], hyp["beta"])[:4]
    ref, bound = R.terms_from(g, k, kw, kb, hyp["w_std"], hyp["b_std"], hyp["last_w_std"])
    got = device_terms(L, ctx, x, layers, act, hyp, nkinv, al, coef)
    again = device_terms(L, ctx, x, layers, act, hyp, nkinv, al, coef)
    for i in range(4):
        print("term %d got %.15g ref %.15g err %.3g bound %.3g" % (i, got[i], ref[i], abs(got[i] - ref[i]), 1e-9 * bound[i]))
        assert abs(got[i] - ref[i]) <= 1e-9 * bound[i], (i, got[i], ref[i])
    assert got.tobytes() == again.tobytes()


# ----------------------------------------------------------------------------- 7. zero borders and b_std -> 0
def bordered(n=16, seed=11):
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 8, 8, 1))
    x[:, 2:6, 2:6, :] = rng.standard_normal((n, 4, 4, 1))      # MNIST-like: a two-pixel all-zero border
    y = np.sin(x[:, 3, 3, 0]) + 0.3 * rng.standard_normal(n)
    return x, y


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("act", ["relu", "erf"])
def test_zero_border_images(act, dtype):
    x, y = bordered()
    x, y = x.astype(dtype).astype(np.float64), y.astype(dtype).astype(np.float64)
    hyp = dict(HYP, b_std=0.3)
    model, vmap = make_model(x, y, 3, act, "tp", dtype, hyp)
    check_against_reference(model, vmap, x, y, 3, act, "tp", dtype, hyp)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("act", ["relu", "erf"])
def test_zero_border_images_with_b_std_exactly_zero(L, ctx, act, dtype):
    """b_std = 0: pixels whose neighbourhood is all zero have zero variance, where the ReLU map is not differentiable.
    Every returned value is finite and the b_std gradient is exactly 0 (no 0 * inf)."""
    x, y = bordered()
    hyp = dict(HYP, b_std=0.0)
    model, vmap = make_model(x, y, 3, act, "tp", dtype, hyp)
    assert model.kernel.b_std.safe_value == 0.0
    loss, grads = model.loss_and_grad()
    names = {id(v): k for k, v in model.vars().items()}
    assert np.isfinite(loss) and all(np.isfinite(g) for g in grads.values()), (loss, grads)
    assert grads[names[id(vmap["b_std"])]] == 0.0
    # and at the C ABI: the term itself, before any chain rule
    n = x.shape[0]
    xd, yd = ctx.to_device(x.astype(dtype)), ctx.to_device(y.astype(dtype))
    quad, logdet, info = C.c_double(), C.c_double(), C.c_int()
    terms = (C.c_double * 4)()
    ctx.call("smn_spr_cnn_loss_grad", L.dtype_code(dtype), L.ACT[act], 3, hyp["w_std"], 0.0, hyp["last_w_std"], xd.ptr, n, 8, 8, 1,
             yd.ptr, hyp["eps"], 2.0 * hyp["alpha"], hyp["beta"] / hyp["alpha"], C.byref(quad), C.byref(logdet), C.byref(info), terms)
    assert info.value == 0 and terms[1] == 0.0
    assert all(np.isfinite(t) for t in terms) and np.isfinite(quad.value) and np.isfinite(logdet.value)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("act", ["relu", "erf"])
def test_zero_border_images_with_the_default_b_std(act, dtype):
    """b_std = 1e-8 (the reference's default, regression/train.py:43): every value finite, the other gradients within
    tolerance; the reference's relative step is useless for b_std there, so that one is not compared."""
    x, y = bordered()
    x, y = x.astype(dtype).astype(np.float64), y.astype(dtype).astype(np.float64)
    hyp = dict(HYP, b_std=1e-8)
    model, vmap = make_model(x, y, 3, act, "tp", dtype, hyp)
    check_against_reference(model, vmap, x, y, 3, act, "tp", dtype, hyp, skip=("b_std",))


# ----------------------------------------------------------------------------- 8. not positive definite
def test_non_pd_matrix_gives_nan_and_ok(L, ctx):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((12, 6, 6, 2))
    x = np.concatenate([x, x, x], axis=0).astype(np.float32)          # duplicated images: K is singular
    y = rng.standard_normal(36).astype(np.float32)
    model, _ = make_model(x, y, 2, "relu", "gp", np.float32, dict(HYP, eps=1e-12))
    loss, grads = model.loss_and_grad()                               # SMN_OK: no exception
    assert np.isnan(loss) and set(grads) == set(model.vars()) and all(np.isnan(g) for g in grads.values())
    xd, yd = ctx.to_device(x), ctx.to_device(y)
    quad, logdet, info = C.c_double(), C.c_double(), C.c_int()
    terms = (C.c_double * 4)()
    ctx.call("smn_spr_cnn_loss_grad", L.F32, L.ACT["relu"], 2, 1.3, 0.4, 0.9, xd.ptr, 36, 6, 6, 2, yd.ptr, 1e-12, 0.0, 1.0,
             C.byref(quad), C.byref(logdet), C.byref(info), terms)
    assert info.value > 0 and all(np.isnan(t) for t in terms)


# ----------------------------------------------------------------------------- 9. the training step
def test_train_step_uses_the_analytic_conv_gradient():
    from smnngp import train
    n, h, w, c, layers, act, method = 24, 6, 6, 2, 3, "relu", "tp"
    x, y = data(n, h, w, c, 42)
    model, vmap = make_model(x, y, layers, act, method, np.float64)
    keys = keys_of(method)
    ref = R.ref_grad_fd(x, y, layers, act, method, keys, **HYP)
    names = {id(v): k for k, v in model.vars().items()}
    before = {k: float(v.value) for k, v in model.vars().items()}
    # the update Adam makes from the reference differences (chain rule to the raw values), on stand-in variables
    from smnngp.spax.base import TrainVar
    shadow = {k: TrainVar(v) for k, v in before.items()}
    ref_raw = {names[id(vmap[k])]: ref[k] * float(vmap[k].constraint.grad(vmap[k].value)) for k in keys}
    train.Adam(shadow)(1e-2, ref_raw)
    step = train.build_train_step(model, method="analytic")
    value = step(1e-2)
    assert abs(value - R.ref_loss(x, y, layers, act, method, **HYP)) < 1e-9 * max(1.0, abs(value))
    for k, v in model.vars().items():
        got, want = float(v.value) - before[k], float(shadow[k].value) - before[k]
        print("%s update %.12g reference %.12g" % (k, got, want))
        assert abs(got - want) < 2e-6 * max(abs(want), 1e-2), (k, got, want)
    # method="auto" takes the same route: no forward kernel build is called from Python, i.e. no finite differences
    model2, _ = make_model(x, y, layers, act, method, np.float64)
    ctx = model2.x_data.ctx
    calls, orig = [], ctx.call

    def counting(name, *args):
        calls.append(name)
        return orig(name, *args)

    ctx.call = counting
    try:
        train.build_train_step(model2, method="auto")(1e-2)
    finally:
        del ctx.call
    assert "smn_spr_cnn_loss_grad" in calls and "smn_kernel_cnn" not in calls, calls
    for k, v in model2.vars().items():
        assert float(v.value) == float(model.vars()[k].value)


# ----------------------------------------------------------------------------- 10. above the limit
def test_images_above_the_limit_are_refused_and_auto_falls_back(L, ctx):
    """H*W > SMN_CNN_GRAD_MAX_PIXELS (1024; the forward kernel goes to 4096): SMN_ENOTSUP with a message that names the
    limit, NotImplementedError from loss_and_grad, and build_train_step(method="auto") falls back to differences."""
    from smnngp import train
    n, h, w, c = 6, 40, 40, 1
    x, y = data(n, h, w, c, 9)
    xd, yd = ctx.to_device(x), ctx.to_device(y)
    quad, logdet, info = C.c_double(), C.c_double(), C.c_int()
    terms = (C.c_double * 4)()
    with pytest.raises(L.SmnError) as e:
        ctx.call("smn_spr_cnn_loss_grad", L.F64, L.ACT["relu"], 2, 1.3, 0.4, 0.9, xd.ptr, n, h, w, c, yd.ptr, 5e-2, 0.0, 1.0,
                 C.byref(quad), C.byref(logdet), C.byref(info), terms)
    assert e.value.code == L.ENOTSUP and "1024" in str(e.value)
    with pytest.raises(L.SmnError) as e:
        ctx.call("smn_kernel_cnn_grad_terms", L.F64, L.ACT["relu"], 2, 1.3, 0.4, 0.9, xd.ptr, n, h, w, c, xd.ptr, n, yd.ptr,
                 1.0, terms)
    assert e.value.code == L.ENOTSUP
    model, _ = make_model(x, y, 2, "relu", "gp", np.float64)
    with pytest.raises(NotImplementedError):
        model.loss_and_grad()
    with pytest.raises(NotImplementedError):
        train.build_train_step(model, method="analytic")(1e-2)
    before = {k: float(v.value) for k, v in model.vars().items()}
    value = train.build_train_step(model, method="auto")(1e-2)
    assert np.isfinite(value) and any(float(v.value) != before[k] for k, v in model.vars().items())
    # bad arguments: SMN_EINVAL with a message
    with pytest.raises(L.SmnError) as e:
        ctx.call("smn_kernel_cnn_grad_terms", L.F64, 7, 2, 1.3, 0.4, 0.9, xd.ptr, n, 8, 8, 1, xd.ptr, n, yd.ptr, 1.0, terms)
    assert e.value.code == L.EINVAL
