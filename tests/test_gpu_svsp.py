"""GPU tests of the sparse variational classifier's evaluation path: the per-image kernel diagonal, the posterior moments,
the Monte-Carlo softmax head (with given and with generated variates), the device generator, SVSP.test_acc_nll /
evaluate end to end against the fp64 rules of tests/_svsp_rules.py, and the checkpoint round trip."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _svsp_rules as R  # noqa: E402
from _tol import relerr, relerr_norm  # noqa: E402
from test_gpu_parity import RTOL  # noqa: E402  (the kernel tolerance of the parity tests)

KW = dict(num_hiddens=3, act="relu", w_std=1.2, b_std=0.1, last_w_std=1.0)


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


def _device_kernel(network, **kw):
    from smnngp import nt_kernels
    if network == "cnn":
        return nt_kernels.get_cnn_kernel(kw["num_hiddens"], act=kw["act"], w_std=kw["w_std"], b_std=kw["b_std"], last_w_std=kw["last_w_std"])
    return nt_kernels.get_conv_resnet_kernel(kw["num_hiddens"], 1, act=kw["act"], w_std=kw["w_std"], b_std=kw["b_std"], last_w_std=kw["last_w_std"])


def _conv_diag(ctx, kfn, x):
    d = ctx.empty((x.shape[0],), x.dtype)
    act, depth, w, b, lw = kfn.params
    ctx.call("smn_kernel_conv_diag", d.dcode, 0 if kfn.entry == "smn_kernel_cnn" else 1, act, depth, w, b, lw, x.ptr,
             x.shape[0], x.shape[1], x.shape[2], x.shape[3], d.ptr)
    return d


# ----------------------------------------------------------------------------- 1. diagonal
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("network,shape,depth,act", [("cnn", (40, 8, 8, 1), 3, "relu"), ("cnn", (6, 32, 32, 3), 4, "relu"),
                                                     ("cnn", (9, 12, 10, 2), 2, "erf"), ("resnet", (12, 8, 8, 1), 1, "relu"),
                                                     ("resnet", (5, 16, 16, 3), 2, "erf")])
def test_conv_diag_is_the_diagonal_of_the_symmetric_build(ctx, dtype, network, shape, depth, act):
    kw = dict(num_hiddens=depth, act=act, w_std=1.2, b_std=0.1, last_w_std=0.9)
    x = np.random.default_rng(1).standard_normal(shape).astype(dtype)
    kfn = _device_kernel(network, **kw)
    xd = ctx.to_device(x)
    full = kfn(xd, xd).numpy()
    diag = _conv_diag(ctx, kfn, xd).numpy()
    assert diag.dtype == dtype and np.array_equal(diag, np.diag(full))                 # bit-identical
    ref = np.array([R.kernel_fn(network, **kw)(x[i:i + 1].astype(np.float64))[0, 0] for i in range(shape[0])])
    err = relerr(diag, ref)
    print("conv diag %s %s %s: relerr %.3g" % (network, shape, np.dtype(dtype).name, err))
    assert err < RTOL[dtype]


def test_conv_diag_rejects_bad_arguments(ctx, L):
    kfn = _device_kernel("cnn", **KW)
    xd = ctx.to_device(np.zeros((2, 8, 8, 1)))
    d = ctx.empty((2,), np.float64)
    with pytest.raises(L.SmnError):
        ctx.call("smn_kernel_conv_diag", d.dcode, 2, 0, 3, 1.0, 0.1, 1.0, xd.ptr, 2, 8, 8, 1, d.ptr)      # kind
    with pytest.raises(L.SmnError):
        ctx.call("smn_kernel_conv_diag", d.dcode, 1, 0, 1, 1.0, 0.1, 1.0, xd.ptr, 2, 12, 12, 1, d.ptr)    # resnet: multiples of 8
    assert kfn.entry == "smn_kernel_cnn"


# ----------------------------------------------------------------------------- 2. moments
def _moments(ctx, k_zz, k_zt, ktt, q_mu, q_var, eps, dtype):
    n_i, t = k_zt.shape
    c = q_mu.shape[0]
    mean, var = ctx.empty((t, c), dtype), ctx.empty((t, c), dtype)
    info, nonpos = C.c_int(-1), C.c_int64(-1)
    qm, qv = ctx.to_device(q_mu.astype(np.float64)), ctx.to_device(q_var.astype(np.float64))     # always fp64
    ctx.call("smn_svsp_moments", mean.dcode, k_zz.ptr, k_zt.ptr, ktt.ptr, qm.ptr, qv.ptr, n_i, t, c, eps, mean.ptr, var.ptr,
             C.byref(info), C.byref(nonpos))
    return mean.numpy(), var.numpy(), info.value, nonpos.value


@pytest.mark.parametrize("eps", [1e-3, 1e-6])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_moments_against_the_rules(ctx, fx, dtype, eps):
    kfn, ofn = _device_kernel("cnn", **KW), R.kernel_fn("cnn", **KW)
    z64 = ctx.to_device(fx["z"])
    k_zz = kfn(z64, None)                                                               # always fp64
    zd, xd = ctx.to_device(fx["z"].astype(dtype)), ctx.to_device(fx["x"].astype(dtype))
    k_zt = kfn(zd, xd)
    ktt = _conv_diag(ctx, kfn, xd)
    mean, var, info, nonpos = _moments(ctx, k_zz, k_zt, ktt, fx["q_mu"], fx["q_var"], eps, dtype)
    rm, rv = R.moments_diag(ofn, fx["z"], fx["x"], fx["q_mu"], fx["q_var"], eps)
    cond = R.moments(ofn(fx["z"]), ofn(fx["z"], fx["x"][:1]), np.ones(1), fx["q_mu"], fx["q_var"], eps)[2]
    tol = 1e-7 if dtype == np.float64 else 8 * cond * 2.0 ** -23
    em, ev = relerr_norm(mean, rm), relerr_norm(var, rv)
    print("moments %s eps %g: cond(K_rel) %.1f  relerr mean %.3g var %.3g  (tol %.3g)" % (np.dtype(dtype).name, eps, cond, em, ev, tol))
    assert info == 0 and nonpos == 0 and mean.dtype == dtype
    assert em < tol and ev < tol


def test_moments_count_nonpositive_variances(ctx, fx):
    """K_tt understated by the caller: var <= 0 is reported, not clamped."""
    kfn = _device_kernel("cnn", **KW)
    z64, xd = ctx.to_device(fx["z"]), ctx.to_device(fx["x"][:16])
    k_zz, k_zt = kfn(z64, None), kfn(z64, xd)
    ktt = np.asarray(_conv_diag(ctx, kfn, xd).numpy())
    ktt[3] = -5.0
    _, var, info, nonpos = _moments(ctx, k_zz, k_zt, ctx.to_device(ktt), fx["q_mu"], fx["q_var"], 1e-3, np.float64)
    assert info == 0 and nonpos == 4 and (var[3] < 0).all() and (np.delete(var, 3, axis=0) > 0).all()


def test_moments_not_positive_definite(ctx, fx):
    z = fx["z"].copy()
    z[7] = z[3]                                                                         # a duplicated inducing image, no jitter
    kfn = _device_kernel("cnn", **KW)
    z64, xd = ctx.to_device(z), ctx.to_device(fx["x"][:32])
    mean, var, info, _ = _moments(ctx, kfn(z64, None), kfn(z64, xd), _conv_diag(ctx, kfn, xd), fx["q_mu"], fx["q_var"], 0.0,
                                  np.float64)                                           # no SmnError: SMN_OK
    assert info > 0 and np.isnan(mean).all() and np.isnan(var).all()


# ----------------------------------------------------------------------------- 3. head with given noise
def _head(ctx, L, mean, sigma, labels, S, dtype, df=0.0, seed=0, point0=0, noise=None, want_score=True):
    t, c = mean.shape
    md, sd = ctx.to_device(mean.astype(dtype)), ctx.to_device(sigma.astype(dtype))
    nd = None if noise is None else (noise if isinstance(noise, L.DeviceArray) else ctx.to_device(noise.astype(dtype)))
    ll, score = ctx.empty((t,), np.float64), ctx.empty((t, c), np.float64)
    pred_d = C.c_void_p()
    ctx.call("smn_malloc", max(4 * t, 16), C.byref(pred_d))
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    try:
        ctx.call("smn_mc_softmax", md.dcode, md.ptr, sd.ptr, labels.ctypes.data_as(C.POINTER(C.c_int)), t, c, S, df, seed, point0,
                 None if nd is None else nd.ptr, ll.ptr, pred_d, score.ptr if want_score else None)
        pred = np.empty(t, dtype=np.int32)
        ctx.call("smn_memcpy_d2h", pred.ctypes.data_as(C.c_void_p), pred_d, 4 * t)
    finally:
        ctx.call("smn_free", pred_d)
    return ll.numpy(), (score.numpy() if want_score else None), pred


def _head_tol(dtype, S, ref):
    if dtype == np.float64:
        return 1e-10 * np.maximum(1.0, np.abs(ref))
    return (S + 64) * 2.0 ** -23 * np.ones_like(ref)


def _check_pred(pred, ref_score, tol):
    """Equal to the reference's argmax wherever its two best scores are further apart than both tolerances."""
    top = np.sort(ref_score, axis=1)
    clear = np.ones(len(pred), bool) if ref_score.shape[1] == 1 else (top[:, -1] - top[:, -2]) > 2 * np.max(tol)
    assert np.array_equal(pred[clear], np.argmax(ref_score, axis=1)[clear])
    best = ref_score[np.arange(len(pred)), pred]
    assert (top[:, -1] - best <= 2 * np.max(tol)).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T,Cn,S", list(itertools.product([1, 255, 256], [1, 4, 10, 100], [1, 7, 1000])))
def test_head_with_given_noise(ctx, L, dtype, T, Cn, S):
    rng = np.random.default_rng(1000 * T + 10 * Cn + S)
    mean = rng.uniform(-40.0, 40.0, (T, Cn)).astype(dtype)
    sigma = rng.uniform(0.1, 3.0, (T, Cn)).astype(dtype)
    noise = rng.standard_normal((T, Cn, S)).astype(dtype)
    labels = rng.integers(0, Cn, T)
    ll, score, pred = _head(ctx, L, mean, sigma, labels, S, dtype, noise=noise)
    rll, rscore, _ = R.head(mean, sigma, labels, noise)                                 # fp64 arithmetic on the same inputs
    e_ll, e_sc = np.max(np.abs(ll - rll) / _head_tol(dtype, S, rll)), np.max(np.abs(score - rscore) / _head_tol(dtype, S, rscore))
    print("head %s T %d C %d S %d: error / tolerance  ll %.3g  score %.3g" % (np.dtype(dtype).name, T, Cn, S, e_ll, e_sc))
    assert e_ll <= 1.0 and e_sc <= 1.0
    _check_pred(pred, rscore, _head_tol(dtype, S, rscore))
    if Cn == 1:
        assert np.all(ll == 0.0)
    ll2, none, pred2 = _head(ctx, L, mean, sigma, labels, S, dtype, noise=noise, want_score=False)     # score_d is optional
    assert none is None and np.array_equal(ll2, ll) and np.array_equal(pred2, pred)


def test_head_validates_its_arguments(ctx, L):
    mean, sigma = np.zeros((4, 3)), np.ones((4, 3))
    for bad in ([0, 1, 3, 0], [0, -1, 2, 0]):
        with pytest.raises(L.SmnError) as e:
            _head(ctx, L, mean, sigma, bad, 8, np.float64)
        assert e.value.code == L.EINVAL
    with pytest.raises(L.SmnError):
        _head(ctx, L, np.zeros((2, 129)), np.ones((2, 129)), [0, 0], 8, np.float64)                    # SMN_SVSP_MAX_CLASSES
    with pytest.raises(L.SmnError):
        _head(ctx, L, mean, sigma, [0, 0, 0, 0], 0, np.float64)


def test_head_negative_variance_gives_nan_for_that_point_only(ctx, L):
    mean, sigma = np.zeros((3, 4)), np.ones((3, 4))
    sigma[1, 2] = np.nan                                                                # sqrt of a negative variance
    ll, score, _ = _head(ctx, L, mean, sigma, [0, 1, 2], 64, np.float64, seed=3)
    assert np.isnan(ll[1]) and np.isfinite(ll[[0, 2]]).all() and np.isfinite(score[[0, 2]]).all()


# ----------------------------------------------------------------------------- 4. generator
def test_philox_known_answers_on_the_device(ctx):
    for ctr, key, want in R.PHILOX_KAT:
        out = (C.c_uint32 * 4)()
        ctx.call("smn_debug_philox", (C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), out)
        assert tuple(out) == want, [hex(v) for v in out]


def _variates(ctx, dtype, seed, df, point0, npoints, c, s):
    out = ctx.empty((npoints, c, s), dtype)
    ctx.call("smn_rng_variates", out.dcode, seed, df, point0, npoints, c, s, out.ptr)
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("df", [0.0, 1.0, 4.0, 9.3])
def test_variates_follow_their_distribution_and_are_uncorrelated(ctx, dtype, df):
    xi = _variates(ctx, dtype, 20240229, df, 0, 64, 4, 4096).numpy()
    n, d, cors = R.variate_statistics(xi, df)
    print("variates %s df %g: KS D sqrt(N) = %.3f" % (np.dtype(dtype).name, df, d * np.sqrt(n)),
          {k: round(float(v * np.sqrt(n)), 3) for k, v in cors.items()})
    assert n == 2 ** 20 and np.isfinite(xi).all()
    assert d < 1.95 / np.sqrt(n)
    for name, c in cors.items():
        assert c < 5 / np.sqrt(n), (name, c)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("df", [0.0, 4.0])
def test_variates_are_keyed_by_global_point_index(ctx, dtype, df):
    whole = _variates(ctx, dtype, 77, df, 0, 256, 5, 64).numpy()
    part = _variates(ctx, dtype, 77, df, 100, 8, 5, 64).numpy()
    assert np.array_equal(part, whole[100:108])
    fewer = _variates(ctx, dtype, 77, df, 100, 8, 3, 64).numpy()                        # nor by the number of classes
    assert np.array_equal(fewer, whole[100:108, :3])
    assert not np.array_equal(_variates(ctx, dtype, 78, df, 100, 8, 5, 64).numpy(), part)
    big = (1 << 40) + 77                                                                # the high seed word is part of the key
    assert not np.array_equal(_variates(ctx, dtype, big, df, 100, 8, 5, 64).numpy(), part)


# ----------------------------------------------------------------------------- 5. fused equals given
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("df", [0.0, 4.0])
@pytest.mark.parametrize("Cn", [4, 10, 20])
def test_fused_head_equals_the_head_on_its_own_variates(ctx, L, dtype, df, Cn):
    T, S, seed, point0 = 64, 500, 991, 1000
    rng = np.random.default_rng(Cn)
    mean, sigma = rng.uniform(-5.0, 5.0, (T, Cn)), rng.uniform(0.1, 2.0, (T, Cn))
    labels = rng.integers(0, Cn, T)
    xi = _variates(ctx, dtype, seed, df, point0, T, Cn, S)
    ll_g, sc_g, pred_g = _head(ctx, L, mean, sigma, labels, S, dtype, noise=xi)
    ll_f, sc_f, pred_f = _head(ctx, L, mean, sigma, labels, S, dtype, df=df, seed=seed, point0=point0)
    tol = (lambda v: 1e-12 * np.ones_like(v)) if dtype == np.float64 else (lambda v: _head_tol(dtype, S, v))
    print("fused - given %s df %g C %d: ll %.3g score %.3g" % (np.dtype(dtype).name, df, Cn, np.max(np.abs(ll_f - ll_g)),
                                                               np.max(np.abs(sc_f - sc_g))))
    assert (np.abs(ll_f - ll_g) <= tol(ll_g)).all() and (np.abs(sc_f - sc_g) <= tol(sc_g)).all()
    _check_pred(pred_f, sc_g, tol(sc_g))
    # and the whole thing against the rules on the downloaded variates
    rll, rscore, _ = R.head(mean.astype(dtype), sigma.astype(dtype), labels, xi.numpy())
    assert (np.abs(ll_f - rll) <= _head_tol(dtype, S, rll)).all() and (np.abs(sc_f - rscore) <= _head_tol(dtype, S, rscore)).all()


# ----------------------------------------------------------------------------- 6. end to end
S_EVAL, S_REF = 1024, 65536


def _model(fx, method, dtype=np.float64, eps=None):
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.models import SVSP
    from smnngp.spax.priors import GaussianPrior, InverseGammaPrior
    kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_cnn_kernel(3, 4, "relu", w_std=w, b_std=b, last_w_std=l), 1.2, 0.1, 1.0)
    prior = GaussianPrior() if method == "svgp" else InverseGammaPrior(2.0, 2.0)
    kw = {} if eps is None else dict(eps=eps)
    model = SVSP(prior, kernel, fx["z"], num_latent_gps=4, dtype=dtype, **kw)
    model.q_mu.assign(fx["q_mu"])
    model.q_sqrt.assign(model.q_sqrt.constraint.inverse(fx["q_var"]))
    return model


def _reference(fx, method, eps):
    """The rules on the host at S_REF draws of NumPy's generator: ll [T], score [T,C], p, sd (per-draw mean and spread)."""
    ofn = R.kernel_fn("cnn", **KW)
    mean, var = R.moments_diag(ofn, fx["z"], fx["x"], fx["q_mu"], fx["q_var"], eps)
    rng = np.random.default_rng(99)
    out = []
    for i0 in range(0, len(mean), 32):                                                  # chunks of points: memory only
        shape = (len(mean[i0:i0 + 32]), mean.shape[1], S_REF)
        xi = rng.standard_normal(shape) if method == "svgp" else rng.standard_t(4.0, shape)     # a = b = 2: t_4, scale 1
        out.append(R.head_statistics(mean[i0:i0 + 32], np.sqrt(var[i0:i0 + 32]), fx["y"][i0:i0 + 32], xi))
    return [np.concatenate(v) for v in zip(*out)]


@pytest.fixture(scope="module")
def reference(fx):
    return {m: _reference(fx, m, 1e-6) for m in ("svgp", "svtp")}


@pytest.mark.parametrize("method", ["svgp", "svtp"])
def test_end_to_end_against_the_rules(fx, reference, method):
    model = _model(fx, method)
    ll, pred, score = model.predict_scores(4242, fx["x"], fx["y"], S_EVAL)
    nll, correct = model.test_acc_nll(4242, fx["x"], fx["y"], S_EVAL)
    assert nll == pytest.approx(-np.mean(ll), abs=1e-15) and correct == int(np.sum(pred == fx["y"]))
    rll, rscore, p, sd = reference[method]
    t = len(rll)
    se = sd / (p * np.sqrt(S_EVAL))                                                     # of log mean_S p, per point and class
    se_nll = np.sqrt(np.sum(se[np.arange(t), fx["y"]] ** 2)) / t
    ref_nll, ref_pred = -np.mean(rll), np.argmax(rscore, axis=1)
    order = np.argsort(rscore, axis=1)
    i1, i2 = order[:, -1], order[:, -2]
    gap = rscore[np.arange(t), i1] - rscore[np.arange(t), i2]
    ambiguous = gap < 5 * np.sqrt(se[np.arange(t), i1] ** 2 + se[np.arange(t), i2] ** 2)
    print("%s: nll %.6f reference %.6f: %.2f standard errors (se %.3g); accuracy %.2f %% reference %.2f %%; ambiguous %.1f %%; "
          "differing predictions %d" % (method, nll, ref_nll, abs(nll - ref_nll) / se_nll, se_nll, 100.0 * correct / t,
                                        100.0 * np.mean(ref_pred == fx["y"]), 100.0 * np.mean(ambiguous), int(np.sum(pred != ref_pred))))
    assert abs(nll - ref_nll) < 5 * se_nll
    assert np.mean(ambiguous) <= 0.05
    assert np.array_equal(pred[~ambiguous], ref_pred[~ambiguous])
    assert np.mean(ref_pred == fx["y"]) > 0.9


def test_fp32_model_agrees_with_fp64_within_the_sampling_error(fx, reference):
    """The fp32 head draws from the same Philox words in fp32 arithmetic (close to the fp64 variates, not equal to them): the
    two results differ by far less than the sampling error either of them carries."""
    rll, _, p, sd = reference["svgp"]
    t = len(rll)
    se_nll = np.sqrt(np.sum((sd / (p * np.sqrt(S_EVAL)))[np.arange(t), fx["y"]] ** 2)) / t
    n64, c64 = _model(fx, "svgp").test_acc_nll(5, fx["x"], fx["y"], S_EVAL)
    n32, c32 = _model(fx, "svgp", dtype=np.float32).test_acc_nll(5, fx["x"], fx["y"], S_EVAL)
    print("fp32 nll %.6f fp64 %.6f (se %.3g); correct %d / %d" % (n32, n64, se_nll, c32, c64))
    assert abs(n32 - n64) < 5 * np.sqrt(2.0) * se_nll and abs(c32 - c64) <= 0.05 * t


# ----------------------------------------------------------------------------- 7. batch invariance
@pytest.mark.parametrize("method", ["svgp", "svtp"])
def test_evaluate_does_not_depend_on_the_batching(fx, method):
    model = _model(fx, method)
    S, seed = 256, 10
    n64, a64 = model.evaluate(fx["x"], fx["y"], S, seed=seed, batch=64)
    n256, a256 = model.evaluate(fx["x"], fx["y"], S, seed=seed, batch=256)
    parts = [model.test_acc_nll((seed, i0), fx["x"][i0:i0 + 100], fx["y"][i0:i0 + 100], S) + (len(fx["y"][i0:i0 + 100]),)
             for i0 in range(0, 256, 100)]
    nll = sum(p[0] * p[2] for p in parts) / 256
    acc = sum(p[1] for p in parts) * 100.0 / 256
    assert abs(n64 - n256) <= 1e-12 and abs(nll - n256) <= 1e-12 and a64 == a256 == acc
    assert model.evaluate(fx["x"], fx["y"], S, seed=seed + 1)[0] != n256                # another seed: other variates


# ----------------------------------------------------------------------------- 8. checkpoint, surface
@pytest.mark.parametrize("method", ["svgp", "svtp"])
def test_restore_svsp_round_trip(tmp_path, fx, method):
    from smnngp import checkpoint as CK
    model = _model(fx, method)
    if method == "svtp":
        model.prior.a.assign(model.prior.a.constraint.inverse(2.5))
    d = str(tmp_path / "run")
    CK.Checkpointer(d).save(3, model.vars())
    CK.save_svsp_meta(d, dict(method=method, network="cnn", num_hiddens=3, activation="relu", alpha=2.0, beta=2.0, last_w_std=1.0))
    restored, context = CK.restore_svsp(d)
    assert context["method"] == method
    want = model.test_acc_nll(31, fx["x"][:64], fx["y"][:64], 128)
    assert restored.test_acc_nll(31, fx["x"][:64], fx["y"][:64], 128) == want
    with pytest.raises(ValueError):
        restored.test_acc_nll(31, np.zeros((4, 16, 16, 1)), np.zeros(4, int), 8)        # resizing is the caller's job


def test_training_side_raises_and_sample_f_iid_serves_device_variates(ctx, fx):
    from smnngp.spax.priors import GaussianPrior, InverseGammaPrior
    model = _model(fx, "svtp")
    with pytest.raises(NotImplementedError):
        model.loss(0, fx["x"], fx["y"], 256, 8)
    for prior in (GaussianPrior(), InverseGammaPrior(2.0, 3.0)):
        with pytest.raises(NotImplementedError):
            prior.sample_f(0, None, None, 8)
        with pytest.raises(NotImplementedError):
            prior.kl_divergence(None, None, None, None, 40, 4)
        df, scale = prior.head_params()
        mean, var = np.arange(6.0).reshape(2, 3), np.full((2, 3), 4.0)
        f = prior.sample_f_iid((9, 50), mean, var, 16).numpy()                          # [C,B,S]
        xi = _variates(ctx, np.float64, 9, df, 50, 3, 2, 16).numpy()                    # [B,C,S]
        assert f.shape == (2, 3, 16)
        assert np.allclose(f, mean[..., None] + np.sqrt(scale * 4.0) * xi.transpose(1, 0, 2), rtol=0, atol=1e-13)
        cov = np.stack([np.diag(v) + 0.3 * (1 - np.eye(3)) for v in var])               # only the diagonal is read
        assert np.array_equal(prior.sample_f_iid((9, 50), mean, cov, 16).numpy(), f)


def test_mlp_kernels_are_not_wired(fx):
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.models import SVSP
    from smnngp.spax.priors import GaussianPrior
    kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_mlp_kernel(2, w_std=w, b_std=b, last_w_std=l), 1.0, 0.1, 1.0)
    with pytest.raises(NotImplementedError):
        SVSP(GaussianPrior(), kernel, fx["z"], num_latent_gps=4).test_acc_nll(0, fx["x"][:4], fx["y"][:4], 8)


def test_kzz_cache_follows_the_content_of_the_inducing_images(ctx, fx):
    model = _model(fx, "svgp")
    z0, k0 = model.inducing_state(ctx=ctx)
    assert model.inducing_state(ctx=ctx)[1] is k0                                       # unchanged: kept
    before = k0.numpy().copy()
    model.inducing_variable.value[3] *= 2.0                                             # edited in place: same array, same id
    k1 = model.inducing_state(ctx=ctx)[1]
    assert k1 is not k0 and not np.array_equal(k1.numpy()[3], before[3]) and np.array_equal(k1.numpy()[5, 6], before[5, 6])
    model.kernel.w_std.assign(model.kernel.w_std.constraint.inverse(0.9))               # another hyper-parameter: rebuilt
    assert model.inducing_state(ctx=ctx)[1] is not k1
