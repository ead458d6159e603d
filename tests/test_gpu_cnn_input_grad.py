"""GPU tests of the inducing-image gradient: smn_kernel_cnn_input_grad (csrc/cnn_input_grad.hip) against the NumPy reverse-mode
rules (tests/_cnn_input_grad_rules.py), its reproducibility, edge cases and limits, SVSP.loss_and_grad(inducing_grad=True)
against the rules applied to the ELBO rules' Gbar, and train_svsp with the inducing images among the variables.

Bounds.  The entry alone, element-wise against S = the same sum over absolute values (the terms may cancel): 1e-9 * S in fp64,
the bound test_gpu_cnn_grad.py uses for the same per-pixel factors; 2e-3 * S in fp32 on inputs rounded to fp32 first, the
project's fp32 kernel tolerance (tests/_tol.py).  The model: 1e-9 * S + C_F64 cond^2 2^-52 * max|reference|, the second term
being the bound test_gpu_svsp_elbo.py puts on Gbar itself.  No wall-clock assertion anywhere."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _cnn_input_grad_rules as G  # noqa: E402
import _svsp_elbo_rules as E  # noqa: E402
import _svsp_rules as R  # noqa: E402

HYP = dict(w_std=1.3, b_std=0.4, last_w_std=0.9)
# the shapes of test_gpu_cnn_grad.py: together they reach every pixels-per-lane form (1, 4, 16; ragged and exact)
SHAPES = [(24, 6, 6, 2, 3), (20, 5, 7, 3, 2), (12, 8, 8, 1, 4), (12, 32, 32, 3, 2), (12, 32, 32, 1, 4),
          (12, 12, 12, 1, 2), (12, 16, 16, 2, 2), (10, 20, 20, 1, 2)]
# beyond them: no hidden layer (only the first and last lines of each pass remain), and the two most elongated images the
# pixel limit admits, whose padded maps are the largest (3 x 1026 and 1026 x 3 elements)
EXTRA_SHAPES = [(9, 5, 5, 2, 0), (7, 12, 12, 1, 0), (5, 1, 1024, 1, 2), (5, 1024, 1, 2, 2)]
KW = dict(num_hiddens=3, act="relu", w_std=1.2, b_std=0.1, last_w_std=1.0)     # the kernel of test_gpu_svsp_elbo.py
C_F64 = 100.0
U = 2.0 ** -52


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


def data(n, h, w, c, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, h, w, c))
    g = rng.standard_normal((n, n))
    return x, g + g.T


def device_gx(L, ctx, x, g, layers, act, hyp, n_grad, dtype=np.float64, ldg=None):
    n, h, w, c = x.shape
    xd = ctx.to_device(np.ascontiguousarray(x, dtype=dtype))
    gd = ctx.to_device(np.ascontiguousarray(g, dtype=dtype))
    out = ctx.empty((max(n_grad, 1), h, w, c), dtype)
    ctx.call("smn_kernel_cnn_input_grad", L.dtype_code(dtype), L.ACT.get(act, act), layers, hyp["w_std"], hyp["b_std"],
             hyp["last_w_std"], xd.ptr, n, h, w, c, gd.ptr, n if ldg is None else ldg, n_grad, out.ptr)
    return out.raw_numpy()


def worst_ratio(got, ref, s, rel):
    """max |got - ref| / (rel * S); an element whose S is 0 must be reproduced exactly."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    diff = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(s > 0, diff / (rel * s), np.where(diff == 0, 0.0, np.inf))
    return float(np.max(ratio))


# ----------------------------------------------------------------------------- 4. the entry alone against the rules
_REF = {}


def reference(n, h, w, c, layers, act, dtype):
    """(x, g as the device sees them, gx, S) for all n images, computed once per case and shared by both n_grad."""
    key = (n, h, w, c, layers, act, np.dtype(dtype).name)
    if key not in _REF:
        x, g = data(n, h, w, c, 7 * n + layers)
        x, g = x.astype(dtype).astype(np.float64), g.astype(dtype).astype(np.float64)
        _REF[key] = (x, g) + G.input_grad(g, x, layers, act, HYP["w_std"], HYP["b_std"], HYP["last_w_std"])
    return _REF[key]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("part", [False, True], ids=["all", "third"])
@pytest.mark.parametrize("act", ["relu", "erf"])
@pytest.mark.parametrize("n,h,w,c,layers", SHAPES + EXTRA_SHAPES)
def test_entry_alone_against_the_numpy_rules(L, ctx, n, h, w, c, layers, act, part, dtype):
    x, g, ref, s = reference(n, h, w, c, layers, act, dtype)
    n_grad = n // 3 if part else n
    got = device_gx(L, ctx, x, np.tril(g), layers, act, HYP, n_grad, dtype)     # only the lower triangle is read
    rel = 1e-9 if dtype == np.float64 else 2e-3
    ratio = worst_ratio(got, ref[:n_grad], s[:n_grad], rel)
    print("input grad %s %s n_grad=%d %s: worst |err| / (%g S) = %.3g" % ((n, h, w, c, layers), act, n_grad,
                                                                          np.dtype(dtype).name, rel, ratio))
    assert ratio <= 1.0


# ----------------------------------------------------------------------------- 5. reproducibility with a split partner range
def test_split_partner_range_is_right_and_reproducible(L, ctx):
    """n = 300 images of 6x6x1, 40 of them differentiated: 40 owners cannot fill the device, so every owner's 299 partners
    are cut into slices summed by the second stage.  Against the rules, and a second call returns the same bytes."""
    n, h, w, c, layers, act, n_grad = 300, 6, 6, 1, 2, "relu", 40
    hyp = dict(HYP, b_std=0.2)
    x, g = data(n, h, w, c, 3)
    ref, s = G.input_grad(g, x, layers, act, hyp["w_std"], hyp["b_std"], hyp["last_w_std"], n_grad=n_grad)
    got = device_gx(L, ctx, x, g, layers, act, hyp, n_grad)
    again = device_gx(L, ctx, x, g, layers, act, hyp, n_grad)
    ratio = worst_ratio(got, ref, s, 1e-9)
    print("input grad n=300 n_grad=40: worst |err| / (1e-9 S) = %.3g" % ratio)
    assert ratio <= 1.0
    assert got.tobytes() == again.tobytes()


# ----------------------------------------------------------------------------- 6. finiteness
def bordered(n=16, seed=11):
    """The zero-border images of test_gpu_cnn_grad.py (MNIST-like: a two-pixel all-zero border)."""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 8, 8, 1))
    x[:, 2:6, 2:6, :] = rng.standard_normal((n, 4, 4, 1))
    g = rng.standard_normal((n, n))
    return x, g + g.T


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("b_std", [0.3, 0.0])
@pytest.mark.parametrize("act", ["relu", "erf"])
def test_zero_border_images(L, ctx, act, b_std, dtype):
    """b_std = 0 exactly: the border pixels have zero variance in every layer their neighbourhood stays zero, where the ReLU
    map is not differentiable; such pixels contribute no variance-side term on the device and in the rules alike.  Every
    output is finite (the border included) and within the bound of the rules."""
    x, g = bordered()
    x, g = x.astype(dtype).astype(np.float64), g.astype(dtype).astype(np.float64)
    hyp = dict(HYP, b_std=b_std)
    ref, s = G.input_grad(g, x, 3, act, hyp["w_std"], b_std, hyp["last_w_std"], n_grad=6)
    got = device_gx(L, ctx, x, g, 3, act, hyp, 6, dtype)
    assert np.isfinite(got).all() and np.isfinite(got[:, :2]).all() and np.isfinite(got[:, :, 6:]).all()
    rel = 1e-9 if dtype == np.float64 else 2e-3
    ratio = worst_ratio(got, ref, s, rel)
    print("zero border %s b_std=%g %s: worst |err| / (%g S) = %.3g" % (act, b_std, np.dtype(dtype).name, rel, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("act", ["relu", "erf"])
def test_partner_that_is_a_copy_of_a_differentiated_image(L, ctx, act, dtype):
    """The inducing images are initialised from the training set, so a batch image may equal one of them bit for bit: an
    off-diagonal pair with correlation 1."""
    n, h, w, c, layers, n_grad = 14, 6, 6, 2, 3, 5
    x, g = data(n, h, w, c, 21)
    x[n - 2] = x[1]
    x[n - 1] = x[4]
    x, g = x.astype(dtype).astype(np.float64), g.astype(dtype).astype(np.float64)
    ref, s = G.input_grad(g, x, layers, act, HYP["w_std"], HYP["b_std"], HYP["last_w_std"], n_grad=n_grad)
    got = device_gx(L, ctx, x, g, layers, act, HYP, n_grad, dtype)
    rel = 1e-9 if dtype == np.float64 else 2e-3
    ratio = worst_ratio(got, ref, s, rel)
    print("copied partner %s %s: worst |err| / (%g S) = %.3g" % (act, np.dtype(dtype).name, rel, ratio))
    assert ratio <= 1.0


# ----------------------------------------------------------------------------- 7. limits and bad arguments
def test_limits_and_bad_arguments(L, ctx):
    def err(fn):
        with pytest.raises(L.SmnError) as e:
            fn()
        return e.value

    x, g = data(6, 40, 40, 1, 9)
    e = err(lambda: device_gx(L, ctx, x, g, 2, "relu", HYP, 6))
    assert e.code == L.ENOTSUP and "1024" in str(e)
    x, g = data(6, 8, 8, 1, 9)
    assert err(lambda: device_gx(L, ctx, x, g, 2, 7, HYP, 6)).code == L.EINVAL          # bad act
    assert err(lambda: device_gx(L, ctx, x, g, 2, "relu", HYP, 0)).code == L.EINVAL     # n_grad = 0
    assert err(lambda: device_gx(L, ctx, x, g, 2, "relu", HYP, 7)).code == L.EINVAL     # n_grad > n
    assert err(lambda: device_gx(L, ctx, x, g, 2, "relu", HYP, 6, ldg=5)).code == L.EINVAL
    assert str(err(lambda: device_gx(L, ctx, x, g, 2, "relu", HYP, 6, ldg=5)))
    xd, gd, out = ctx.to_device(x), ctx.to_device(g), ctx.empty(x.shape, np.float64)
    with pytest.raises(L.SmnError) as e2:
        ctx.call("smn_kernel_cnn_input_grad", 5, 0, 2, 1.3, 0.4, 0.9, xd.ptr, 6, 8, 8, 1, gd.ptr, 6, 6, out.ptr)   # bad dtype
    assert e2.value.code == L.EINVAL
    assert L._lib.smn_kernel_cnn_input_grad(ctx.handle, L.F64, 0, 2, 1.3, 0.4, 0.9, xd.ptr, 6, 8, 8, 1, None, 6, 6,
                                            out.ptr) == L.EINVAL                                                  # NULL pointer


# ----------------------------------------------------------------------------- 8. the model
def _model(fx, method, eps=1e-3, z=None):
    """The model of test_gpu_svsp_elbo.py (get_cnn_kernel, 3 layers, relu, 4 classes)."""
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.models import SVSP
    from smnngp.spax.priors import GaussianPrior, InverseGammaPrior
    kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_cnn_kernel(3, 4, "relu", w_std=w, b_std=b, last_w_std=l), 1.2, 0.1, 1.0)
    prior = GaussianPrior() if method == "svgp" else InverseGammaPrior(2.0, 3.0)
    model = SVSP(prior, kernel, fx["z"] if z is None else z, num_latent_gps=4, dtype=np.float64, eps=eps)
    model.q_mu.assign(fx["q_mu"])
    model.q_sqrt.assign(model.q_sqrt.constraint.inverse(fx["q_var"]))
    if method == "svtp":
        model.prior.a.assign(model.prior.a.constraint.inverse(1.7))
        model.prior.b.assign(model.prior.b.constraint.inverse(2.3))
    return model


def _device_variates(ctx, seed, df, point0, B, Cn, S):
    out, dout = ctx.empty((B, Cn, S), np.float64), ctx.empty((B, Cn, S), np.float64)
    ctx.call("smn_rng_variates_ddf", out.dcode, seed, df, point0, B, Cn, S, out.ptr, dout.ptr)
    return out.raw_numpy().transpose(1, 0, 2).copy(), dout.raw_numpy().transpose(1, 0, 2).copy()


def _rules_gradient(ctx, model, method, z, x, y, N, S, seed, p0):
    """(d loss / d Z, S scale, cond(K_abs)) from the ELBO rules' Gbar and the reverse-mode rules, at the model's parameters."""
    student = method == "svtp"
    pt = E.prior_terms(model.prior.a.safe_value, model.prior.b.safe_value, 2.0, 3.0) if student else E.prior_terms()
    xi, dxi = _device_variates(ctx, seed, pt["df"], p0, len(y), 4, S)
    w, b, lw = model.kernel.get_params()
    u = np.concatenate([z, x])
    K = R.kernel_fn("cnn", num_hiddens=3, act="relu", w_std=w, b_std=b, last_w_std=lw)(u)
    ref = E.elbo(K, len(z), np.asarray(model.q_mu.value), np.asarray(model.q_sqrt.constraint(model.q_sqrt.value)),
                 model.eps.safe_value, pt["s"], N, y, xi, pt["scale"], dxi if student else None)
    gz, s = G.input_grad(ref["gbar"], u, 3, "relu", w, b, lw, n_grad=len(z))
    return gz, s, ref["cond"]


def _inducing_key(grads):
    keys = [k for k in grads if "inducing_variable" in k]
    assert len(keys) == 1, list(grads)
    return keys[0]


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


@pytest.mark.parametrize("method", ["svgp", "svtp"])
def test_model_inducing_gradient_against_the_rules(ctx, fx, method):
    I, B, S, N, seed, p0 = 40, 64, 16, 5000, 4242, 128
    x, y = fx["x"][:B], fx["y"][:B]
    model = _model(fx, method)
    value, grads, gbar = model.loss_and_grad((seed, p0), x, y, N, S, inducing_grad=True, return_gbar=True)
    key = _inducing_key(grads)
    got = grads[key]
    assert got.shape == (I, 8, 8, 1) and got.dtype == np.float64 and gbar.shape == (I + B, I + B)
    ref, s, cond = _rules_gradient(ctx, model, method, fx["z"], x, y, N, S, seed, p0)
    bound = C_F64 * cond ** 2 * U
    tol = 1e-9 * s + bound * np.max(np.abs(ref))
    ratio = float(np.max(np.abs(got - ref) / tol))
    print("model %s: inducing gradient max|ref| %.3e, worst |err| / (1e-9 S + %.2e max|ref|) = %.3g" % (method, np.max(np.abs(ref)),
                                                                                                     bound, ratio))
    assert np.isfinite(got).all() and ratio <= 1.0
    # everything else is the bits of the call without it, with kernel_grads either way
    value0, grads0 = model.loss_and_grad((seed, p0), x, y, N, S)
    assert value0 == value and set(grads) - set(grads0) == {key}
    for k, v in grads0.items():
        assert np.array_equal(np.asarray(v), np.asarray(grads[k])), k
    value1, grads1 = model.loss_and_grad((seed, p0), x, y, N, S, kernel_grads=False, inducing_grad=True)
    assert value1 == value and np.array_equal(grads1[key], got)
    assert not any(k.split(".")[-1] in ("w_std", "b_std", "last_w_std") for k in grads1)


def test_singular_inducing_kernel_gives_a_nan_array_and_no_exception(fx):
    z = fx["z"].copy(); z[1] = z[0]                                   # two equal inducing images: K_ZZ singular (no jitter)
    model = _model(fx, "svgp", eps=1e-300, z=z)
    value, grads = model.loss_and_grad(1, fx["x"][:16], fx["y"][:16], 1000, 8, inducing_grad=True)
    got = grads[_inducing_key(grads)]
    assert np.isnan(value) and got.shape == z.shape and np.isnan(got).all()


def test_conv_resnet_has_no_inducing_gradient(fx):
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.models import SVSP
    from smnngp.spax.priors import GaussianPrior
    kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_conv_resnet_kernel(1, 4, "relu", w_std=w, b_std=b, last_w_std=l),
                        1.2, 0.1, 1.0)
    model = SVSP(GaussianPrior(), kernel, fx["z"], num_latent_gps=4)
    with pytest.raises(NotImplementedError):
        model.loss_and_grad(1, fx["x"][:16], fx["y"][:16], 1000, 8, kernel_grads=False, inducing_grad=True)


# ----------------------------------------------------------------------------- 9. the trainer
@pytest.fixture(scope="module")
def fx_train():
    return R.fixture(num_test=512)


def _fresh(fx2, method):
    model = _model(fx2, method)
    model.q_mu.assign(np.zeros_like(fx2["q_mu"]))
    model.q_sqrt.assign(model.q_sqrt.constraint.inverse(np.ones_like(fx2["q_var"])))
    return model


@pytest.mark.parametrize("method", ["svgp", "svtp"])
def test_training_moves_the_inducing_images_and_lowers_the_elbo(fx_train, method):
    """The synthetic problem of test_gpu_svsp_elbo.py's training test (256 points, batches of 64, S = 32, lr 1e-2, from
    q_mu = 0, q_sqrt = 1) with the inducing images among the variables: three epochs move them, keep them finite, and the mean
    nELBO of the last epoch is below the first's."""
    from smnngp import train_svsp as TS
    xt, yt = fx_train["x"][:256], fx_train["y"][:256]
    model = _fresh(fx_train, method)
    variables = TS.svsp_train_vars(model, inducing=True)
    assert any("inducing_variable" in k for k in variables)
    step = TS.build_svsp_train_step(model, variables, num_train=256, num_samples=32)
    z0 = np.array(model.inducing_variable.value)
    epochs = [TS.train_epoch(step, xt, yt, 64, 1e-2, seed=1, epoch=e) for e in range(3)]
    z1 = np.asarray(model.inducing_variable.value)
    print("%s with inducing images: nELBO per epoch %s; max |dZ| %.3e" % (method, ["%.4f" % v for v in epochs],
                                                                         np.max(np.abs(z1 - z0))))
    assert z1.shape == z0.shape and np.isfinite(z1).all() and not np.array_equal(z0, z1)
    assert all(np.isfinite(epochs)) and epochs[-1] < epochs[0]


def test_first_step_takes_the_adam_step_of_the_rules_gradient(ctx, fx_train):
    """The first update of Z against ArrayAdam fed the rules' gradient, every pixel to 2e-6 relative: the assertion of
    test_train_step_uses_the_analytic_conv_gradient, |got - want| < 2e-6 max(|want|, 1e-2), element by element."""
    from smnngp import train_svsp as TS
    method, N, S, seed, p0, lr = "svgp", 256, 32, 5, 64, 1e-2
    x, y = fx_train["x"][:64], fx_train["y"][:64]
    model = _fresh(fx_train, method)
    z0 = np.array(model.inducing_variable.value)
    ref, _, _ = _rules_gradient(ctx, model, method, z0, x, y, N, S, seed, p0)
    want = TS.ArrayAdam().step({"z": z0}, {"z": ref}, lr)["z"] - z0
    step = TS.build_svsp_train_step(model, TS.svsp_train_vars(model, inducing=True), num_train=N, num_samples=S)
    step((seed, p0), x, y, lr)
    got = np.asarray(model.inducing_variable.value) - z0
    ratio = np.abs(got - want) / (2e-6 * np.maximum(np.abs(want), 1e-2))
    print("first step of Z: max |update| %.3e, max difference from the rules' Adam step %.3e (worst |err| / bound %.3g), "
          "norm-wise relative %.3e" % (np.max(np.abs(want)), np.max(np.abs(got - want)), np.max(ratio), E.relerr_norm(got, want)))
    assert np.isfinite(got).all() and np.all(ratio < 1.0)
