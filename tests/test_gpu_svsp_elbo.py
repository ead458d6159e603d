"""GPU tests of the sparse variational classifier's training path: the correlated Monte-Carlo softmax head with its backward
pass (smn_svsp_head_grad), the df-derivative of the variates (smn_rng_variates_ddf), the negative ELBO and its reverse pass
(smn_svsp_elbo_grad), SVSP.loss_and_grad and train_svsp, against the fp64 rules of tests/_svsp_elbo_rules.py.

Tolerances.  fp64 against the rules: norm-wise, C_F64 * cond^2 * 2^-52 -- the gradient passes through a factorisation
and two solves, hence the square; cond is cond(K_abs) for the ELBO and the largest cond(scale cov[c]) for the head alone.
fp32 head: (S + 64) * 2^-23, the bound of the evaluation head (tests/test_gpu_svsp.py), absolute on ll and relative to
max|reference| on every gradient.  Every test prints observed error / bound; profiles/r09_svsp_train.txt keeps the values."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _svsp_elbo_rules as E  # noqa: E402
import _svsp_rules as R  # noqa: E402

KW = dict(num_hiddens=3, act="relu", w_std=1.2, b_std=0.1, last_w_std=1.0)
C_F64 = 100.0
U = 2.0 ** -52


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


def _labels_ptr(y):
    return y.ctypes.data_as(C.POINTER(C.c_int))


def _report(tag, pairs, bound_of):
    """pairs: name -> (got, want, denominator or None for |want|-norm).  Prints error / bound, returns the worst ratio."""
    worst = 0.0
    for name, (got, want, kind) in pairs.items():
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        if kind == "abs":
            err = float(np.max(np.abs(got - want)))
        elif kind == "max":
            err = float(np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-300))
        else:
            err = E.relerr_norm(got, want)
        b = bound_of(name)
        print("%s %-8s err %.3e bound %.3e ratio %.3g" % (tag, name, err, b, err / b))
        worst = max(worst, err / b)
        assert np.isfinite(got).all(), name
    return worst


# ----------------------------------------------------------------------------- 1. the head with given noise
def _head_case(B, Cn, S, student, seed=0):
    rng = np.random.default_rng([B, Cn, S, int(student), seed])
    mean = rng.standard_normal((Cn, B))
    w = rng.standard_normal((Cn, B, B + 3))
    cov = w @ w.transpose(0, 2, 1) / (B + 3) + 0.3 * np.eye(B)[None]
    y = rng.integers(0, Cn, B).astype(np.int32)
    xi = rng.standard_t(4.0, (Cn, B, S)) if student else rng.standard_normal((Cn, B, S))
    dxi = rng.standard_normal((Cn, B, S)) if student else None
    return mean, cov, y, xi, dxi


def _head_device(ctx, dtype, mean, cov, y, S, df, scale, seed=0, point0=0, xi=None, dxi=None):
    Cn, B = mean.shape
    md, cd = ctx.to_device(mean), ctx.to_device(cov)
    gm, gc = ctx.empty((Cn, B), np.float64), ctx.empty((Cn, B, B), np.float64)
    nd = None if xi is None else ctx.to_device(np.ascontiguousarray(xi, dtype=dtype))
    dd = None if dxi is None else ctx.to_device(np.ascontiguousarray(dxi, dtype=dtype))
    ll, gs, dt, info = C.c_double(), C.c_double(), C.c_double(), C.c_int()
    ctx.call("smn_svsp_head_grad", 1 if np.dtype(dtype) == np.float64 else 0, md.ptr, cd.ptr, _labels_ptr(y), B, Cn, S, df, scale,
             seed, point0, None if nd is None else nd.ptr, None if dd is None else dd.ptr, C.byref(ll), gm.ptr, gc.ptr,
             C.byref(gs), C.byref(dt), C.byref(info))
    return dict(ll=ll.value, gmean=gm.raw_numpy(), gcov=gc.raw_numpy(), gscale=gs.value, dfterm=dt.value, info=info.value)


def _head_compare(tag, dtype, got, ref, S, cond, student):
    f64 = np.dtype(dtype) == np.float64
    bound = C_F64 * cond * cond * U if f64 else (S + 64) * 2.0 ** -23
    pairs = dict(ll=(got["ll"], ref["ll"], "abs"), gmean=(got["gmean"], ref["gmean"], None if f64 else "max"),
                 gcov=(got["gcov"], ref["gcov"], None if f64 else "max"), gscale=(got["gscale"], ref["gscale"], None if f64 else "max"))
    if student:
        pairs["dfterm"] = (got["dfterm"], ref["dfterm"], None if f64 else "max")
    assert got["info"] == 0
    assert np.array_equal(got["gcov"], got["gcov"].transpose(0, 2, 1))
    return _report(tag, pairs, lambda name: bound)


@pytest.mark.parametrize("student", [False, True], ids=["normal", "t4"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("S", [1, 7, 100])
@pytest.mark.parametrize("Cn", [1, 4, 10])
@pytest.mark.parametrize("B", [1, 37, 100, 256])
def test_head_with_given_noise(ctx, B, Cn, S, dtype, student):
    mean, cov, y, xi, dxi = _head_case(B, Cn, S, student)
    scale, df = (1.3, 4.0) if student else (1.0, 0.0)
    xi = xi.astype(dtype).astype(np.float64)                 # the values the device reads
    dxi = None if dxi is None else dxi.astype(dtype).astype(np.float64)
    ref = E.head(mean, cov, y, xi, scale, dxi)
    cond = max(np.linalg.cond(scale * cov[c]) for c in range(Cn))
    got = _head_device(ctx, dtype, mean, cov, y, S, df, scale, xi=xi, dxi=dxi)
    worst = _head_compare("head B=%d C=%d S=%d %s %s:" % (B, Cn, S, np.dtype(dtype).name, "t4" if student else "normal"),
                          dtype, got, ref, S, cond, student)
    assert worst <= 1.0


# ----------------------------------------------------------------------------- 2. the generator inside the head
def _device_variates(ctx, dtype, seed, df, point0, B, Cn, S, ddf=False):
    out = ctx.empty((B, Cn, S), dtype)
    if ddf:
        dout = ctx.empty((B, Cn, S), dtype)
        ctx.call("smn_rng_variates_ddf", out.dcode, seed, df, point0, B, Cn, S, out.ptr, dout.ptr)
        return out.raw_numpy().transpose(1, 0, 2).copy(), dout.raw_numpy().transpose(1, 0, 2).copy()
    ctx.call("smn_rng_variates", out.dcode, seed, df, point0, B, Cn, S, out.ptr)
    return out.raw_numpy().transpose(1, 0, 2).copy()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("df", [0.0, 4.0, 1.5])
def test_variates_with_df_derivative(ctx, dtype, df):
    """The companion returns the bits of smn_rng_variates; in fp64 its derivative is the rules' (1e-11 of max(|d|, 1e-3|t|):
    a few units of roundoff through log, expm1 and sqrt)."""
    seed, p0, B, Cn, S = 77, 1000, 5, 6, 40
    xi = _device_variates(ctx, dtype, seed, df, p0, B, Cn, S)
    xi2, dxi = _device_variates(ctx, dtype, seed, df, p0, B, Cn, S, ddf=True)
    assert np.array_equal(xi, xi2)
    if df <= 0:
        assert not dxi.any()
        return
    assert np.isfinite(dxi).all() and dxi.any()
    if np.dtype(dtype) != np.float64:
        return                                               # fp32 draws from fewer bits of each word: no common reference
    rxi, rdxi = E.variates(seed, df, p0, B, Cn, S)
    tol = 1e-11
    err_t = np.max(np.abs(xi - rxi) / np.maximum(np.abs(rxi), 1e-3))
    err_d = np.max(np.abs(dxi - rdxi) / np.maximum(np.abs(rdxi), 1e-3 * np.abs(rxi) + 1e-6))
    print("variates df=%g %s: t err %.3e, d/ddf err %.3e (tol %g)" % (df, np.dtype(dtype).name, err_t, err_d, tol))
    assert err_t < tol and err_d < tol


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("student", [False, True], ids=["normal", "t4"])
def test_fused_variates_equal_given_noise(ctx, dtype, student):
    B, Cn, S, seed, p0 = 37, 4, 50, 31337, 123456
    mean, cov, y, _, _ = _head_case(B, Cn, S, student)
    scale, df = (1.3, 4.0) if student else (1.0, 0.0)
    if student:
        xi, dxi = _device_variates(ctx, dtype, seed, df, p0, B, Cn, S, ddf=True)
    else:
        xi, dxi = _device_variates(ctx, dtype, seed, df, p0, B, Cn, S), None
    fused = _head_device(ctx, dtype, mean, cov, y, S, df, scale, seed=seed, point0=p0)
    given = _head_device(ctx, dtype, mean, cov, y, S, df, scale, xi=xi, dxi=dxi)
    tol = 1e-12 if np.dtype(dtype) == np.float64 else (S + 64) * 2.0 ** -23
    for k in ("ll", "gmean", "gcov", "gscale", "dfterm"):
        a, b = np.asarray(fused[k]), np.asarray(given[k])
        err = float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)) if k != "ll" else float(abs(a - b))
        print("fused vs given %s %s %-7s %.3e (tol %.3g)" % (np.dtype(dtype).name, "t4" if student else "normal", k, err, tol))
        assert err <= tol, k
    ref = E.head(mean, cov, y, xi.astype(np.float64), scale, None if dxi is None else dxi.astype(np.float64))
    cond = max(np.linalg.cond(scale * cov[c]) for c in range(Cn))
    assert _head_compare("fused head %s:" % np.dtype(dtype).name, dtype, fused, ref, S, cond, student) <= 1.0


# ----------------------------------------------------------------------------- 3. the ELBO entry with K from the oracle
def _elbo_device(ctx, dtype, K, I, q_mu, q_var, eps, s, N, y, S, df, scale, seed=0, point0=0, xi=None, dxi=None):
    Un = K.shape[0]
    B, Cn = Un - I, q_mu.shape[0]
    kd, qm, qv = ctx.to_device(K), ctx.to_device(q_mu), ctx.to_device(q_var)
    gm, gv, gb = ctx.empty((Cn, I), np.float64), ctx.empty((Cn, I), np.float64), ctx.empty((Un, Un), np.float64)
    nd = None if xi is None else ctx.to_device(np.ascontiguousarray(xi, dtype=dtype))
    dd = None if dxi is None else ctx.to_device(np.ascontiguousarray(dxi, dtype=dtype))
    out = [C.c_double() for _ in range(6)]
    info = C.c_int()
    ctx.call("smn_svsp_elbo_grad", 1 if np.dtype(dtype) == np.float64 else 0, kd.ptr, Un, I, B, Cn, qm.ptr, qv.ptr, eps, s, float(N),
             _labels_ptr(y), S, df, scale, seed, point0, None if nd is None else nd.ptr, None if dd is None else dd.ptr,
             C.byref(out[0]), C.byref(out[1]), gm.ptr, gv.ptr, C.byref(out[2]), C.byref(out[3]), C.byref(out[4]), C.byref(out[5]),
             gb.ptr, Un, C.byref(info))
    return dict(nll=out[0].value, kl_n=out[1].value, g_q_mu=gm.raw_numpy(), g_q_var=gv.raw_numpy(), g_eps=out[2].value,
                gscale=out[3].value, g_s=out[4].value, dfterm=out[5].value, gbar=gb.raw_numpy(), info=info.value)


@pytest.fixture(scope="module")
def union_kernels(fx):
    """K over [Z; 64 batch images] from the oracle: plain, and with the first 8 batch images replaced by inducing images."""
    ofn = R.kernel_fn("cnn", **KW)
    x = fx["x"][:64].copy()
    plain = ofn(np.concatenate([fx["z"], x]))
    x[:8] = fx["z"][5:13]
    return {False: plain, True: ofn(np.concatenate([fx["z"], x]))}


@pytest.mark.parametrize("student", [False, True], ids=["svgp", "svtp"])
@pytest.mark.parametrize("overlap", [False, True], ids=["disjoint", "overlap8"])
@pytest.mark.parametrize("eps", [1e-3, 1e-6])
def test_elbo_entry_with_the_oracle_kernel(ctx, fx, union_kernels, eps, overlap, student):
    I, B, S, N, seed, p0 = 40, 64, 16, 5000, 9, 640
    K, y = union_kernels[overlap], fx["y"][:64].copy()
    pt = E.prior_terms(1.7, 2.3, 2.0, 3.0) if student else E.prior_terms()
    if student:
        xi, dxi = _device_variates(ctx, np.float64, seed, pt["df"], p0, B, 4, S, ddf=True)
    else:
        xi, dxi = _device_variates(ctx, np.float64, seed, 0.0, p0, B, 4, S), None
    ref = E.elbo(K, I, fx["q_mu"], fx["q_var"], eps, pt["s"], N, y, xi, pt["scale"], dxi)
    got = _elbo_device(ctx, np.float64, K, I, fx["q_mu"], fx["q_var"], eps, pt["s"], N, y, S, pt["df"], pt["scale"], seed, p0)
    assert got["info"] == 0
    assert np.array_equal(got["gbar"], got["gbar"].T)
    bound = C_F64 * ref["cond"] ** 2 * U
    pairs = {k: (got[k], ref[k], None) for k in ("nll", "kl_n", "g_q_mu", "g_q_var", "g_eps", "gbar", "gscale", "g_s")}
    if student:
        pairs["dfterm"] = (got["dfterm"], ref["dfterm"], None)
    worst = _report("elbo eps=%g %s %s cond %.0f:" % (eps, "overlap8" if overlap else "disjoint", "svtp" if student else "svgp",
                                                      ref["cond"]), pairs, lambda name: bound)
    assert worst <= 1.0


# ----------------------------------------------------------------------------- 4. the model
def _model(fx, method, dtype=np.float64, eps=1e-3, network="cnn", z=None):
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.models import SVSP
    from smnngp.spax.priors import GaussianPrior, InverseGammaPrior
    if network == "cnn":
        get = lambda w, b, l: nt_kernels.get_cnn_kernel(3, 4, "relu", w_std=w, b_std=b, last_w_std=l)   # noqa: E731
    else:
        get = lambda w, b, l: nt_kernels.get_conv_resnet_kernel(1, 4, "relu", w_std=w, b_std=b, last_w_std=l)   # noqa: E731
    kernel = NNGPKernel(get, 1.2, 0.1, 1.0)
    prior = GaussianPrior() if method == "svgp" else InverseGammaPrior(2.0, 3.0)
    model = SVSP(prior, kernel, fx["z"] if z is None else z, num_latent_gps=4, dtype=dtype, eps=eps)
    model.q_mu.assign(fx["q_mu"])
    model.q_sqrt.assign(model.q_sqrt.constraint.inverse(fx["q_var"]))
    if method == "svtp":
        model.prior.a.assign(model.prior.a.constraint.inverse(1.7))
        model.prior.b.assign(model.prior.b.constraint.inverse(2.3))
    return model


def _short(grads):
    return {k.split(".")[-1]: v for k, v in grads.items()}


@pytest.mark.parametrize("method", ["svgp", "svtp"])
def test_model_loss_and_grad_against_the_rules(ctx, fx, method):
    I, B, S, N, seed, p0, eps = 40, 64, 16, 5000, 4242, 128, 1e-3
    x, y = fx["x"][:B], fx["y"][:B]
    model = _model(fx, method, eps=eps)
    value, grads, nll, kl_n, gbar = model.loss_and_grad((seed, p0), x, y, N, S, aux=True, return_gbar=True)
    assert all("inducing_variable" not in k for k in grads)
    g = _short(grads)
    student = method == "svtp"
    a, b = (model.prior.a.safe_value, model.prior.b.safe_value) if student else (None, None)
    pt = E.prior_terms(a, b, 2.0, 3.0) if student else E.prior_terms()
    if student:
        xi, dxi = _device_variates(ctx, np.float64, seed, pt["df"], p0, B, 4, S, ddf=True)
    else:
        xi, dxi = _device_variates(ctx, np.float64, seed, 0.0, p0, B, 4, S), None
    u = np.concatenate([fx["z"], x])
    K = R.kernel_fn("cnn", **KW)(u)
    eps_v = model.eps.safe_value
    ref = E.elbo(K, I, fx["q_mu"], model.q_sqrt.constraint(model.q_sqrt.value), eps_v, pt["s"], N, y, xi, pt["scale"], dxi)
    bound = C_F64 * ref["cond"] ** 2 * U
    sp = model.q_sqrt.constraint
    want = dict(q_mu=ref["g_q_mu"], q_sqrt=ref["g_q_var"] * sp.grad(model.q_sqrt.value),
                eps=ref["g_eps"] * sp.grad(model.eps.value))
    if student:
        g_a, g_b = E.prior_grads(ref, pt, a, b, N)
        want.update(a=g_a * sp.grad(model.prior.a.value), b=g_b * sp.grad(model.prior.b.value))
    pairs = {k: (g[k], v, None) for k, v in want.items()}
    pairs.update(nll=(nll, ref["nll"], None), kl_n=(kl_n, ref["kl_n"] + pt["kl_extra"] / N, None),
                 value=(value, ref["nll"] + ref["kl_n"] + pt["kl_extra"] / N, None), gbar=(gbar.raw_numpy(), ref["gbar"], None))
    worst = _report("model %s:" % method, pairs, lambda name: bound)
    assert worst <= 1.0
    # kernel hyper-parameters: sum Gbar (rules) * central-difference dK of the oracle kernel.  The reference itself carries the
    # truncation and rounding error of a central difference with h = 1e-5 (~1e-10 per entry), the device tangents the forward conv
    # kernel's per-entry bound of 1e-9 (tests/test_golden.py): 2e-9 * sum |Gbar| |dK/d theta|, plus the fp64 bound above.
    h = 1e-5
    for name in ("w_std", "b_std", "last_w_std"):
        dk = (R.kernel_fn("cnn", **{**KW, name: KW[name] + h})(u) - R.kernel_fn("cnn", **{**KW, name: KW[name] - h})(u)) / (2 * h)
        var = getattr(model.kernel, name)
        chain = float(sp.grad(var.value))
        want_t = float(np.sum(ref["gbar"] * dk)) * chain
        tol = (2e-9 * float(np.sum(np.abs(ref["gbar"]) * np.abs(dk))) + bound * abs(want_t / chain)) * chain
        print("model %s: %-10s got % .12e want % .12e err %.3e bound %.3e ratio %.3g" % (method, name, g[name], want_t,
                                                                                          abs(g[name] - want_t), tol, abs(g[name] - want_t) / tol))
        assert abs(g[name] - want_t) <= tol, name
    # kernel_grads=False: the remaining entries, bit for bit; aux
    value2, grads2 = model.loss_and_grad((seed, p0), x, y, N, S, kernel_grads=False)
    assert value2 == value and set(grads) - set(grads2) == {k for k in grads if k.split(".")[-1] in ("w_std", "b_std", "last_w_std")}
    for k, v in grads2.items():
        assert np.array_equal(np.asarray(v), np.asarray(grads[k])), k
    assert value == nll + kl_n


def test_conv_resnet_needs_kernel_grads_off(fx):
    model = _model(fx, "svgp", network="resnet")
    x, y = fx["x"][:16], fx["y"][:16]
    with pytest.raises(NotImplementedError):
        model.loss_and_grad(1, x, y, 1000, 8)
    value, grads = model.loss_and_grad(1, x, y, 1000, 8, kernel_grads=False)
    assert np.isfinite(value) and set(_short(grads)) == {"q_mu", "q_sqrt", "eps"}
    assert all(np.isfinite(np.asarray(v)).all() for v in grads.values())


def test_fp32_model_head(ctx, fx):
    """dtype float32 selects the head's arithmetic only: -ll against the rules fed the device's fp32 variates within the head
    bound (S + 64) 2^-23; kl / N is the fp64 value."""
    I, B, S, N, seed = 40, 64, 16, 5000, 3
    x, y = fx["x"][:B], fx["y"][:B]
    model = _model(fx, "svgp", dtype=np.float32)
    value, grads, nll, kl_n = model.loss_and_grad(seed, x, y, N, S, aux=True)
    xi = _device_variates(ctx, np.float32, seed, 0.0, 0, B, 4, S).astype(np.float64)
    K = R.kernel_fn("cnn", **KW)(np.concatenate([fx["z"], x]))
    ref = E.elbo(K, I, fx["q_mu"], fx["q_var"], model.eps.safe_value, 1.0, N, y, xi, 1.0)
    tol = (S + 64) * 2.0 ** -23
    print("fp32 model: -ll %.9f rules %.9f diff %.3e (tol %.3g); kl/N diff %.3e" % (nll, ref["nll"], abs(nll - ref["nll"]), tol,
                                                                                   abs(kl_n - ref["kl_n"])))
    assert abs(nll - ref["nll"]) <= tol and abs(kl_n - ref["kl_n"]) <= C_F64 * ref["cond"] ** 2 * U * abs(ref["kl_n"])
    g = _short(grads)
    assert np.max(np.abs(g["q_mu"] - ref["g_q_mu"])) <= tol * np.max(np.abs(ref["g_q_mu"]))


# ----------------------------------------------------------------------------- 5. robustness
def test_two_calls_are_bit_identical_and_seeds_differ(ctx, fx):
    x, y = fx["x"][:64], fx["y"][:64]
    for method in ("svgp", "svtp"):
        model = _model(fx, method)
        v1, g1 = model.loss_and_grad(7, x, y, 5000, 32)
        v2, g2 = model.loss_and_grad(7, x, y, 5000, 32)
        v3, _ = model.loss_and_grad(8, x, y, 5000, 32)
        assert v1 == v2 and v1 != v3
        for k in g1:
            assert np.array_equal(np.asarray(g1[k]), np.asarray(g2[k])), k
    mean, cov, yy, xi, dxi = _head_case(100, 10, 100, True)
    a = _head_device(ctx, np.float64, mean, cov, yy, 100, 4.0, 1.3, seed=5)
    b = _head_device(ctx, np.float64, mean, cov, yy, 100, 4.0, 1.3, seed=5)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_non_positive_definite_inputs_give_info_and_nan(ctx, fx, union_kernels):
    mean, cov, y, xi, _ = _head_case(37, 4, 7, False)
    cov[2, 5, 5] = -1.0
    got = _head_device(ctx, np.float64, mean, cov, y, 7, 0.0, 1.0, xi=xi)
    assert got["info"] > 0 and np.isnan(got["ll"]) and np.isnan(got["gmean"]).all() and np.isnan(got["gcov"]).all()
    K = union_kernels[False].copy()
    K[3, 3] = -1.0
    got = _elbo_device(ctx, np.float64, K, 40, fx["q_mu"], fx["q_var"], 1e-3, 1.0, 5000, fx["y"][:64].copy(), 8, 0.0, 1.0)
    assert got["info"] > 0 and np.isnan(got["nll"]) and np.isnan(got["kl_n"]) and np.isnan(got["g_q_mu"]).all()
    assert np.isnan(got["gbar"]).all() and np.isnan(got["g_eps"])
    z = fx["z"].copy(); z[1] = z[0]                                   # two equal inducing images: K_ZZ singular (no jitter)
    model = _model(fx, "svgp", eps=1e-300, z=z)
    value, grads = model.loss_and_grad(1, fx["x"][:16], fx["y"][:16], 1000, 8)
    assert np.isnan(value) and all(np.isnan(np.asarray(v)).all() for v in grads.values())


def test_bad_arguments(ctx, L):
    mean, cov, y, xi, _ = _head_case(4, 3, 5, False)

    def code(fn):
        with pytest.raises(L.SmnError) as e:
            fn()
        return e.value.code

    assert code(lambda: _head_device(ctx, np.float64, mean, cov, y, 0, 0.0, 1.0)) == L.EINVAL                 # S = 0
    assert code(lambda: _head_device(ctx, np.float64, mean, cov, y, 5, 0.0, 0.0)) == L.EINVAL                 # scale = 0
    assert code(lambda: _head_device(ctx, np.float64, mean, cov, y, 5, float("nan"), 1.0)) == L.EINVAL        # df NaN
    bad = y.copy(); bad[1] = 3
    assert code(lambda: _head_device(ctx, np.float64, mean, cov, bad, 5, 0.0, 1.0)) == L.EINVAL               # label out of range
    big = 257
    assert code(lambda: _head_device(ctx, np.float64, np.zeros((2, big)), np.tile(np.eye(big), (2, 1, 1)),
                                     np.zeros(big, np.int32), 2, 0.0, 1.0)) == L.ENOTSUP                      # B > SMN_SVSP_MAX_BATCH
    assert code(lambda: _head_device(ctx, np.float64, np.zeros((129, 2)), np.tile(np.eye(2), (129, 1, 1)),
                                     np.zeros(2, np.int32), 2, 0.0, 1.0)) == L.EINVAL                         # C > 128
    K = np.eye(7)
    q = np.ones((3, 3))
    assert code(lambda: _elbo_device(ctx, np.float64, K, 3, q, q, -1.0, 1.0, 10, y, 5, 0.0, 1.0)) == L.EINVAL  # eps < 0
    assert code(lambda: _elbo_device(ctx, np.float64, K, 3, q, q, 1e-3, 1.0, 0, y, 5, 0.0, 1.0)) == L.EINVAL   # num_train = 0


# ----------------------------------------------------------------------------- 6. training
S_EVAL = 1000


def _held_out_nll_and_se(model, x, y):
    """evaluate() on the held-out points and the standard error of its nll, computed as test_gpu_svsp's
    test_end_to_end_against_the_rules does: the rules' moments at the model's parameters, per-point sd / (p sqrt(S))."""
    nll, acc = model.evaluate(x, y, S_EVAL, seed=10)
    w, b, lw = model.kernel.get_params()
    ofn = R.kernel_fn("cnn", num_hiddens=3, act="relu", w_std=w, b_std=b, last_w_std=lw)
    q_var = np.asarray(model.q_sqrt.constraint(model.q_sqrt.value))
    mean, var = R.moments_diag(ofn, np.asarray(model.inducing_variable.value), x, np.asarray(model.q_mu.value), q_var,
                               model.eps.safe_value)
    df, scale = model.prior.head_params()
    rng = np.random.default_rng(99)
    xi = rng.standard_normal(mean.shape + (S_EVAL,)) if df <= 0 else rng.standard_t(df, mean.shape + (S_EVAL,))
    _, _, p, sd = R.head_statistics(mean, np.sqrt(scale * var), y, xi)
    t = len(y)
    se = sd / (p * np.sqrt(S_EVAL))
    return nll, acc, float(np.sqrt(np.sum(se[np.arange(t), y] ** 2)) / t)


@pytest.mark.parametrize("method", ["svgp", "svtp"])
def test_training_lowers_the_elbo_and_the_held_out_nll(tmp_path, method):
    """Z fixed; 4 epochs of batches of 64, S = 32, lr 1e-2, from the constructor's q_mu = 0, q_sqrt = 1: the mean nELBO of the last
    epoch is below the first's, the held-out NLL drops by more than 5 standard errors (of the difference), and the trained model
    survives a Checkpointer / restore_svsp round trip."""
    from smnngp import checkpoint as CK
    from smnngp import train_svsp as TS
    fx2 = R.fixture(num_test=512)
    xt, yt, xv, yv = fx2["x"][:256], fx2["y"][:256], fx2["x"][256:], fx2["y"][256:]
    model = _model(fx2, method, eps=1e-3)
    model.q_mu.assign(np.zeros_like(fx2["q_mu"]))
    model.q_sqrt.assign(model.q_sqrt.constraint.inverse(np.ones_like(fx2["q_var"])))
    step = TS.build_svsp_train_step(model, num_train=256, num_samples=32)
    names = {k.split(".")[-1] for k in step.variables}
    assert "inducing_variable" not in names and (("last_w_std" in names) == (method == "svgp"))
    nll0, acc0, se0 = _held_out_nll_and_se(model, xv, yv)
    z0 = np.array(model.inducing_variable.value)
    ck = CK.Checkpointer(str(tmp_path / "run"))
    sched = TS.PlateauSchedule(1e-2)
    epochs = []
    for e in range(4):
        epochs.append(TS.train_epoch(step, xt, yt, 64, sched.lr, seed=1, epoch=e))
        TS.valid_epoch(model, xv, yv, 100, schedule=sched, checkpointer=ck, index=e)
    nll1, acc1, se1 = _held_out_nll_and_se(model, xv, yv)
    se = float(np.hypot(se0, se1))
    print("%s: nELBO per epoch %s; held-out nll %.4f -> %.4f (drop %.1f standard errors, se %.3g); accuracy %.1f -> %.1f %%"
          % (method, ["%.4f" % v for v in epochs], nll0, nll1, (nll0 - nll1) / se, se, acc0, acc1))
    assert epochs[-1] < epochs[0]
    assert nll0 - nll1 > 5 * se
    assert np.array_equal(z0, model.inducing_variable.value)
    d = str(tmp_path / "final")
    CK.Checkpointer(d).save(4, model.vars())
    CK.save_svsp_meta(d, dict(method=method, network="cnn", num_hiddens=3, activation="relu", alpha=2.0, beta=3.0, last_w_std=1.0))
    restored, _ = CK.restore_svsp(d, eps="stored")
    for k, v in model.vars().items():
        assert np.array_equal(np.asarray(v.value), np.asarray(restored.vars()[k].value)), k
    assert restored.evaluate(xv, yv, 100, seed=10) == model.evaluate(xv, yv, 100, seed=10)
    assert os.path.exists(os.path.join(str(tmp_path / "run"), "000.npz"))
