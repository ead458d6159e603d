"""GPU tests of the exact GP / Student-t models on the neural tangent kernel (spax.kernels.NTKKernel; SMN_NET_NTK in the `net`
argument of the model entries; the six-state tangent pass of csrc/grad.hip) against the fp64 NumPy rules of
tests/_ntk_rules.py: Theta from the oracle, log-pdfs from oracle.mvn_logpdf / mvt_logpdf, central differences with h = 1e-5,
predictions from oracle.predict on Theta blocks, leave-one-out from tests/_loo_rules.  Every figure is printed before it is
asserted; no wall-clock assertion anywhere."""
import ctypes as C
import functools
import os
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _multi_rules as M  # noqa: E402
import _ntk_rules as N  # noqa: E402
from _tol import relerr_norm  # noqa: E402

U = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}
LOO_MEASURED = {np.float64: 1.1, np.float32: 3.4}          # tests/test_gpu_loo.py MEASURED: asserted at 8x, in units of cond u


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


def factory(family, layers, act):
    from smnngp import nt_kernels
    base = nt_kernels.get_mlp_kernel if family == "mlp" else nt_kernels.get_dense_resnet_kernel
    return lambda w, b, l: base(layers, 1, act=act, w_std=w, b_std=b, last_w_std=l)


def make_model(family, layers, act, method, dtype, x, y, hyp=N.HYP, multi=False, cls=None):
    from smnngp.spax.kernels import NTKKernel
    from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood
    from smnngp.spax.models import SPR, MultiSPR
    kernel = (cls or NTKKernel)(factory(family, layers, act), hyp["w_std"], hyp["b_std"], hyp["last_w_std"])
    lik = GaussianLikelihood() if method == "gp" else StudentTLikelihood(hyp["alpha"], hyp["beta"])
    if multi:
        model = MultiSPR(kernel, lik, np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype), eps=hyp["eps"])
    else:
        model = SPR(kernel, lik, np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype).reshape(-1), 0.0, 1.0, eps=hyp["eps"])
    vmap = {"w_std": kernel.w_std, "b_std": kernel.b_std, "last_w_std": kernel.last_w_std, "eps": model.eps}
    if method == "tp":
        vmap.update(alpha=lik.a, beta=lik.b)
    return model, vmap


def constrained_grads(model, vmap, grads):
    """d loss / d constrained value: the softplus chain rule undone."""
    names = {id(v): k for k, v in model.vars().items()}
    assert set(grads) == set(model.vars())
    return {k: grads[names[id(var)]] / float(var.constraint.grad(var.value)) for k, var in vmap.items()}


def check_loss_and_grad(tag, model, vmap, ref_loss, ref, loss_tol, grad_tol):
    loss, grads = model.loss_and_grad()
    got = constrained_grads(model, vmap, grads)
    scale = max(abs(v) for v in ref.values())
    print("%s loss %.15g ref %.15g |diff| %.3g" % (tag, loss, ref_loss, abs(loss - ref_loss)))
    for k in ref:
        print("%s d/d%s %.12g ref %.12g  err/max(scale,|ref|) %.3g" % (tag, k, got[k], ref[k], abs(got[k] - ref[k]) / max(scale, abs(ref[k]))))
    assert abs(loss - ref_loss) < loss_tol * max(1.0, abs(ref_loss))
    assert set(got) == set(ref)
    for k in ref:
        assert np.isfinite(got[k]) and abs(got[k] - ref[k]) < grad_tol * max(scale, abs(ref[k])), (k, got[k], ref[k])
    return loss, grads


# ------------------------------------------------------------------------------------------------- loss and gradient
GRAD_CASES = [(f, a, l) for f in ("mlp", "resnet") for a in ("relu", "erf") for l in (2, 3)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("family,act,layers", GRAD_CASES)
def test_loss_and_gradient_match_the_oracle_theta_and_its_central_differences(family, act, layers, method, dtype):
    """n = 150, d = 6, the hyper-parameters of the NNGP gradient test: SPR.loss_and_grad under NTKKernel against the oracle-built
    loss (1e-9 / 1e-3) and its central differences (2e-6 / 1e-2 of max(scale, |ref|)) -- the project's own tolerances."""
    x, y = N.reg_data(150)
    ref_loss, fd = N.ref_loss_and_fd(family, act, layers, method, 150)
    model, vmap = make_model(family, layers, act, method, dtype, x, y)
    f64 = dtype == np.float64
    loss, _ = check_loss_and_grad("%s %s L=%d %s %s" % (family, act, layers, method, np.dtype(dtype).name), model, vmap, ref_loss, fd,
                                  1e-9 if f64 else 1e-3, 2e-6 if f64 else 1e-2)
    assert abs(loss - model.loss()) < (1e-10 if f64 else 1e-4) * max(1.0, abs(ref_loss))


@pytest.mark.parametrize("family,act,layers,method", [("mlp", "erf", 1, "tp"), ("resnet", "relu", 1, "gp"), ("mlp", "relu", 6, "tp"),
                                                      ("resnet", "erf", 6, "tp")])
def test_depths_one_and_six(family, act, layers, method):
    """The first and a late activation set: an off-by-one in the set index shows only here."""
    x, y = N.reg_data(150)
    ref_loss, fd = N.ref_loss_and_fd(family, act, layers, method, 150)
    model, vmap = make_model(family, layers, act, method, np.float64, x, y)
    check_loss_and_grad("%s %s L=%d %s" % (family, act, layers, method), model, vmap, ref_loss, fd, 1e-9, 2e-6)


@pytest.mark.parametrize("family,act", [("mlp", "relu"), ("resnet", "erf")])
@pytest.mark.parametrize("n", [65, 129])
def test_ragged_tiles_of_the_contraction(family, act, n):
    """One row past a 64-tile and one past two: ragged diagonal and off-diagonal tiles, both passes of the tile, fp64."""
    x, y = N.reg_data(n)
    ref_loss, fd = N.ref_loss_and_fd(family, act, 2, "tp", n)
    model, vmap = make_model(family, 2, act, "tp", np.float64, x, y)
    check_loss_and_grad("%s %s n=%d" % (family, act, n), model, vmap, ref_loss, fd, 1e-9, 2e-6)


def test_size_that_skips_identity_tiles():
    """n = 700 (several tile rows of the identity block, a ragged last tile), the tolerance of the NNGP test at this size."""
    x, y = N.reg_data(700, 5, 700)
    ref_loss, fd = N.ref_loss_and_fd("mlp", "relu", 2, "tp", 700, False, 700, 5)
    model, vmap = make_model("mlp", 2, "relu", "tp", np.float64, x, y)
    check_loss_and_grad("n=700", model, vmap, ref_loss, fd, 1e-9, 5e-6)


def test_duplicate_rows():
    """x[7] = x[3] exactly, ReLU, mlp depth 2, fp64: c = 1 off the diagonal, where D = 1/2 whatever the hyper-parameters.  Loss
    and all gradients finite and within 1e-3 of the scale of the central differences (their quotient of acos at c = 1 is the
    noisy side; the fp64 rules alone are within 3.1e-5)."""
    x, y = N.reg_data(150, dup=True)
    ref_loss, fd = N.ref_loss_and_fd("mlp", "relu", 2, "tp", 150, True)
    model, vmap = make_model("mlp", 2, "relu", "tp", np.float64, x, y)
    loss, grads = model.loss_and_grad()
    got = constrained_grads(model, vmap, grads)
    scale = max(abs(v) for v in fd.values())
    print("duplicate rows: loss %.15g ref %.15g" % (loss, ref_loss))
    assert np.isfinite(loss) and abs(loss - ref_loss) < 1e-9 * max(1.0, abs(ref_loss))
    for k, v in fd.items():
        print("duplicate rows: d/d%s %.12g fd %.12g  err/scale %.3g" % (k, got[k], v, abs(got[k] - v) / scale))
        assert np.isfinite(got[k]) and abs(got[k] - v) < 1e-3 * scale, (k, got[k], v)


def test_two_calls_give_the_same_bits():
    x, y = N.reg_data(150)
    for multi, yy in ((False, y), (True, np.stack([y, np.cos(y), y * y], axis=1))):
        model, _ = make_model("resnet", 2, "relu", "tp", np.float32, x, yy, multi=multi)
        first, second = model.loss_and_grad(), model.loss_and_grad()
        assert first[0] == second[0] and first[1] == second[1]


# -------------------------------------------------------------------------------------------------------- predictions
@functools.lru_cache(maxsize=None)
def pred_case():
    rng = np.random.default_rng(41)
    x, xt, y = rng.standard_normal((40, 6)), rng.standard_normal((7, 6)), rng.standard_normal((40, 2))
    yt = rng.standard_normal(7)
    return x, xt, y, yt


@pytest.mark.parametrize("family,act,layers", [("mlp", "relu", 2), ("resnet", "erf", 2)])
def test_predict_is_the_gp_on_theta(family, act, layers):
    """N = 40, T = 7, C = 2, fp64: NTKKernel.predict against oracle.predict on Theta blocks (relerr_norm < 1e-7, as the conv
    predict test asks); its mean equals predict_fn(get="ntk")'s, its covariance does not (that one is the ensemble's)."""
    from smnngp import predict
    from smnngp.spax.kernels import NNGPKernel, NTKKernel
    x, xt, y, _ = pred_case()
    hyp = {k: N.HYP[k] for k in ("w_std", "b_std", "last_w_std")}
    eps = 1e-2
    rm, rc = N.predict(family, x, y, xt, layers, act, eps=eps, **hyp)
    kernel = NTKKernel(factory(family, layers, act), *hyp.values())
    mean, cov = kernel.predict(kernel.get_kernel_fn(), x, y, xt, eps=eps)
    mean, cov = np.asarray(mean), np.asarray(cov)
    print("predict: mean %.3g cov %.3g" % (relerr_norm(mean, rm), relerr_norm(cov, rc)))
    assert mean.shape == (7, 2) and cov.shape == (7, 7)
    assert relerr_norm(mean, rm) < 1e-7 and relerr_norm(cov, rc) < 1e-7
    plain = factory(family, layers, act)(*hyp.values())
    em, ec = predict.gradient_descent_mse_ensemble(plain, x, y, diag_reg=eps)(x_test=xt, get="ntk")
    assert relerr_norm(mean, np.asarray(em)) < 1e-7
    assert relerr_norm(cov, np.asarray(ec)) > 1e-3
    # the NNGP posterior of the same kernel function is untouched by the covariance mode
    km, kc = NNGPKernel(factory(family, layers, act), *hyp.values()).predict(plain, x, y, xt, eps=eps)
    km2, kc2 = predict.gradient_descent_mse_ensemble(kernel.get_kernel_fn(), x, y, diag_reg=eps)(x_test=xt, get="nngp")
    nm, nc = M.predict(family, x, y, xt, layers, act, eps=eps, **hyp)
    print("nngp posterior through the ntk-mode kernel_fn: mean %.3g cov %.3g; against NNGPKernel.predict: %.3g %.3g" % (
        relerr_norm(np.asarray(km2), nm), relerr_norm(np.asarray(kc2), nc), relerr_norm(np.asarray(km2), np.asarray(km)),
        relerr_norm(np.asarray(kc2), np.asarray(kc))))
    for m_, c_ in ((km, kc), (km2, kc2)):
        assert relerr_norm(np.asarray(m_), nm) < 1e-7 and relerr_norm(np.asarray(c_), nc) < 1e-7
    assert relerr_norm(np.asarray(kc), cov) > 1e-3
    # any other callable: asked for get="ntk", the joint factorisation of what it returns
    gm, gcov = NTKKernel(lambda w, b, l: (lambda a, c=None, get="nngp": plain(a, c, get)), *hyp.values()).predict(
        lambda a, c=None, get="nngp": plain(a, c, get), x, y, xt, eps=eps)
    assert relerr_norm(np.asarray(gm), rm) < 1e-7 and relerr_norm(np.asarray(gcov), rc) < 1e-7


@pytest.mark.parametrize("method", ["gp", "tp"])
def test_test_nll(method):
    x, xt, y, yt = pred_case()
    hyp = dict(N.HYP, eps=1e-2)
    model, _ = make_model("mlp", 2, "relu", method, np.float64, x, y[:, 0], hyp)
    ref = N.predictive_nll("mlp", x, y[:, 0], xt, yt, 2, "relu", method, **hyp)
    got = model.test_nll(xt, yt)
    print("test_nll %s %.12g ref %.12g" % (method, got, ref))
    assert abs(got - ref) < 1e-7 * max(1.0, abs(ref))           # test_spr_loss_and_test_nll's fp64 tolerance (cond here ~1e5)


def test_sample_posterior_and_predictive_params():
    """Draws need predict and the fp64 quadratic form only: the shape of the Student-t law is the rules', the draws are finite
    and reproducible."""
    x, xt, y, _ = pred_case()
    hyp = dict(N.HYP, eps=1e-2)
    model, _ = make_model("mlp", 2, "relu", "tp", np.float64, x, y[:, 0], hyp)
    nu, s = 2.0 * hyp["alpha"], hyp["beta"] / hyp["alpha"]
    khat = s * N.theta("mlp", x, None, 2, "relu", hyp["w_std"], hyp["b_std"], hyp["last_w_std"]) + 1e-6 * np.eye(40)
    d = nu + float(y[:, 0] @ np.linalg.solve(khat, y[:, 0]))
    df_post, shape = model.predictive_params()
    assert df_post == nu + 40 and abs(shape - d / (nu + 40) * s) < 1e-7 * shape
    a, b = np.asarray(model.sample_posterior(3, xt, 5)), np.asarray(model.sample_posterior(3, xt, 5))
    assert a.shape == (5, 7) and np.isfinite(a).all() and np.array_equal(a, b)


# ----------------------------------------------------------------------------------------------------------- MultiSPR
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("family,act", [("mlp", "erf"), ("resnet", "relu")])
def test_three_outputs(family, act, method, dtype):
    """C = 3, n = 130 (n + C crosses a 128-tile of the appended rows): loss and gradients against the rules."""
    x, y = M.dense_data(130, 3, dtype == np.float32)[:2]
    hyp = dict(N.HYP)
    keys = N.KEYS if method == "tp" else N.KEYS[:4]
    ref_loss = N.loss(family, x, y, 2, act, method, **hyp)
    fd = N.loss_fd(family, x, y, 2, act, method, keys, **hyp)
    model, vmap = make_model(family, 2, act, method, dtype, x, y, hyp, multi=True)
    f64 = dtype == np.float64
    loss, _ = check_loss_and_grad("multi %s %s %s %s" % (family, act, method, np.dtype(dtype).name), model, vmap, ref_loss, fd,
                                  1e-9 if f64 else 1e-3, 2e-6 if f64 else 1e-2)
    assert abs(model.loss() - ref_loss) < (1e-9 if f64 else 1e-3) * max(1.0, abs(ref_loss))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("method", ["gp", "tp"])
def test_one_output_multispr_is_spr_bit_for_bit(method, dtype):
    x, y = N.reg_data(129)
    single, _ = make_model("mlp", 2, "relu", method, dtype, x, y)
    multi, _ = make_model("mlp", 2, "relu", method, dtype, x, y[:, None], multi=True)
    (l1, g1), (l2, g2) = single.loss_and_grad(), multi.loss_and_grad()
    assert l1 == l2 and [g1[k.replace("(MultiSPR)", "(SPR)")] for k in g2] == list(g2.values())
    assert single.loo_loss() == multi.loo_loss()


def test_classification():
    x, y, lab, xt, _, labt = M.dense_data(130, 3)
    hyp = dict(N.HYP, eps=1e-2)
    model, _ = make_model("mlp", 2, "relu", "gp", np.float64, x, y, hyp, multi=True)
    rm, _ = N.predict("mlp", x, y, xt, 2, "relu", hyp["w_std"], hyp["b_std"], hyp["last_w_std"], hyp["eps"])
    top = np.sort(rm, axis=1)
    assert np.min(top[:, -1] - top[:, -2]) > 1e-6            # no near tie: the arg-max is the rules' arg-max
    want = np.argmax(rm, axis=1)
    assert np.array_equal(model.classify(xt), want)
    assert model.accuracy(xt, labt) == float(np.mean(want == labt))
    r = N.loo("mlp", x, y, 2, "relu", "gp", **hyp)
    ltop = np.sort(r["mean"], axis=1)
    assert np.min(ltop[:, -1] - ltop[:, -2]) > 1e-6
    lwant = np.argmax(r["mean"], axis=1)
    assert np.array_equal(model.loo_classify(), lwant)
    assert model.loo_accuracy(lab) == float(np.mean(lwant == lab))


# ---------------------------------------------------------------------------------------------------------------- LOO
@functools.lru_cache(maxsize=None)
def loo_case(family, act, c, f32):
    """(x, Y [129,c], hyper-parameters with eps chosen for cond(Theta~) <= 1e4, cond): tests/test_gpu_loo.py e2e_case on Theta."""
    x, y = M.dense_data(129, c, f32)[:2]
    th = N.theta(family, x, None, 2, act, N.HYP["w_std"], N.HYP["b_std"], N.HYP["last_w_std"])
    eps = float(np.linalg.eigvalsh(th)[-1]) / 5000.0
    return x, y, dict(N.HYP, eps=eps), float(np.linalg.cond(th + eps * np.eye(129)))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("family,act,c", [("mlp", "relu", 1), ("resnet", "erf", 3)])
def test_leave_one_out(family, act, c, method, dtype):
    """loo_loss, loo_predict and loo_loss_and_grad against _loo_rules on Theta~, with the tolerances tests/test_gpu_loo.py uses
    for the NNGP: errors in units of cond(K~) u against the magnitudes the rules report, asserted at 8x the measured worst and
    never above 64; the gradient against the rules' analytic one with the same bound on sum |G| |dTheta~|."""
    x, y, hyp, cond = loo_case(family, act, c, dtype == np.float32)
    assert cond <= 1e4, cond
    n = y.shape[0]
    cu = cond * U[dtype]
    bound = 8.0 * LOO_MEASURED[dtype]
    assert bound <= 64.0
    ref = N.loo(family, x, y, 2, act, method, **hyp)
    ref_loss, ref_grads = N.loo_loss_grad(family, x, y, 2, act, method, **hyp)
    model, vmap = make_model(family, 2, act, method, dtype, x, y if c > 1 else y[:, 0], hyp, multi=c > 1)
    loss = model.loo_loss()
    mean, scale2, df = model.loo_predict()
    ratios = {"Lambda": abs(-loss * n - ref["lam"]) / ref["lam_abs"] / cu,
              "mean": relerr_norm(np.asarray(mean).reshape(n, c), ref["mean"]) / cu, "scale2": relerr_norm(scale2, ref["scale2"]) / cu}
    val, grads = model.loo_loss_and_grad()
    got = constrained_grads(model, vmap, grads)
    ratios["Lambda(grad call)"] = abs(-val * n - ref["lam"]) / ref["lam_abs"] / cu
    _, dw, db, dl = N.tangents(family, x, 2, act, hyp["w_std"], hyp["b_std"], hyp["last_w_std"])
    ag = np.abs(ref["g"])
    t_abs = {"w_std": np.sum(ag * np.abs(dw)) / n, "b_std": np.sum(ag * np.abs(db)) / n, "last_w_std": np.sum(ag * np.abs(dl)) / n,
             "eps": np.sum(np.abs(np.diag(ref["g"]))) / n}
    if method == "tp":
        a_, b_ = hyp["alpha"], hyp["beta"]
        t_abs.update(alpha=(2.0 * ref["dhead_abs"][0] + ref["dhead_abs"][1] * b_ / a_ ** 2) / n, beta=ref["dhead_abs"][1] / a_ / n)
    for k, v in ref_grads.items():
        ratios["d/d" + k] = abs(got[k] - v) / t_abs[k] / cu
    print("LOO %s %s c=%d %s %s cond %.3g  %s" % (family, act, c, method, np.dtype(dtype).name, cond,
                                                  " ".join("%s=%.3g" % kv for kv in sorted(ratios.items()))))
    assert df == ref["df"] and set(got) == set(ref_grads)
    assert max(ratios.values()) <= bound, ratios


# ------------------------------------------------------------------------------------------------ the flag is not ignored
def spr_loss(L, ctx, x, y, net, eps=1e-2):
    lp, quad, logdet, info = C.c_double(), C.c_double(), C.c_double(), C.c_int()
    n, d = x.shape
    ctx.call("smn_spr_loss", x.dcode, net, L.ACT["relu"], 2, 1.0, 0.3, 1.0, x.ptr, n, d, d, y.ptr, eps, 0.0, 1.0, C.byref(lp),
             C.byref(quad), C.byref(logdet), C.byref(info))
    return lp.value, quad.value, logdet.value, info.value


def cache_stats(ctx):
    h, m, b = C.c_int64(), C.c_int64(), C.c_size_t()
    ctx.call("smn_gram_cache_stats", C.byref(h), C.byref(m), C.byref(b))
    return h.value, m.value, b.value


def test_nngp_model_on_the_same_data_differs_and_is_untouched():
    from smnngp.spax.kernels import NNGPKernel
    x, y = N.reg_data(150)
    nngp, _ = make_model("mlp", 2, "relu", "tp", np.float64, x, y, cls=NNGPKernel)
    ntk, _ = make_model("mlp", 2, "relu", "tp", np.float64, x, y)
    first = (nngp.loss(), nngp.loss_and_grad(), nngp.loo_loss())
    other = (ntk.loss(), ntk.loss_and_grad(), ntk.loo_loss())
    third = (nngp.loss(), nngp.loss_and_grad(), nngp.loo_loss())
    assert first == third
    assert abs(first[0] - other[0]) > 1e-3 and abs(first[2] - other[2]) > 1e-3
    assert abs(first[0] - M.loss("mlp", x, y[:, None], 2, "relu", "tp", **N.HYP)) < 1e-9


def test_ntk_calls_leave_the_gram_cache_alone(L):
    """The f32 Gram-cache shape (2560 padded rows, small d): NNGP, NNGP, NNGP (a hit), NTK, NNGP.  The NTK call neither reads nor
    writes the cache (no hit, no miss, same bytes), the NNGP call behind it is a hit with the bits of the one in front, and the
    NTK result is that of a context that never had a cache."""
    rng = np.random.default_rng(31)
    xh, yh = rng.standard_normal((2500, 50)).astype(np.float32), rng.standard_normal((2500, 1)).astype(np.float32)
    ntk_net = L.NET_MLP | L.NET_NTK
    ctx = L.Context()
    try:
        x, y = ctx.to_device(xh), ctx.to_device(yh)
        for _ in range(3):
            before = spr_loss(L, ctx, x, y, L.NET_MLP)
        s0 = cache_stats(ctx)
        assert s0[0] == 1 and s0[2] > 0, s0
        theta = spr_loss(L, ctx, x, y, ntk_net)
        assert cache_stats(ctx) == s0
        after = spr_loss(L, ctx, x, y, L.NET_MLP)
        s1 = cache_stats(ctx)
        assert s1 == (s0[0] + 1, s0[1], s0[2]), (s0, s1)
        assert before == after and before[3] == 0
        assert theta[3] == 0 and abs(theta[0] - before[0]) > 1e-3 * abs(before[0])
    finally:
        ctx.close()
    cold = L.Context()
    try:
        assert spr_loss(L, cold, cold.to_device(xh), cold.to_device(yh), ntk_net) == theta
    finally:
        cold.close()


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_batched_entries_do_not_take_the_flag_and_stray_bits_are_invalid(L, ctx):
    from smnngp import sweeps, train
    x64, y64 = N.reg_data(65)
    x, y = ctx.to_device(np.ascontiguousarray(x64)), ctx.to_device(np.ascontiguousarray(y64[:, None]))
    n, d = x.shape
    ones = (C.c_double * 2)(1.0, 1.0)
    eps = (C.c_double * 2)(0.1, 0.1)
    quad, logdet, info, terms = (C.c_double * 2)(), (C.c_double * 2)(), (C.c_int * 2)(), (C.c_double * 8)()
    for net in (L.NET_MLP | L.NET_NTK, L.NET_DENSE_RESNET | L.NET_NTK):
        with pytest.raises(L.SmnError) as e:
            ctx.call("smn_spr_loss_grad_batch", L.F64, net, L.ACT["relu"], 2, 2, ones, ones, ones, x.ptr, n, d, d, y.ptr, eps, None, None,
                     quad, logdet, info, terms)
        assert e.value.code == L.ENOTSUP
        with pytest.raises(L.SmnError) as e:
            ctx.call("smn_spr_loss_batch", L.F64, net, L.ACT["relu"], 2, 2, ones, ones, ones, x.ptr, n, d, d, y.ptr, eps, None, None,
                     quad, quad, logdet, info)
        assert e.value.code == L.ENOTSUP
    with pytest.raises(NotImplementedError):
        sweeps.loss_and_grad_batch(ctx, x, y, network="mlp", num_hiddens=2, w_std=[1.0, 1.1], b_std=0.3, eps=0.1, covariance="ntk")
    lp, q1, ld, inf1, t4 = C.c_double(), C.c_double(), C.c_double(), C.c_int(), (C.c_double * 4)()
    for stray in (L.NET_MLP | L.NET_NTK | 0x200, L.NET_NTK | 2, 0x40, L.NET_NTK << 1, -1):
        with pytest.raises(L.SmnError) as e:
            ctx.call("smn_spr_loss", L.F64, stray, L.ACT["relu"], 2, 1.0, 0.3, 1.0, x.ptr, n, d, d, y.ptr, 0.1, 0.0, 1.0, C.byref(lp),
                     C.byref(q1), C.byref(ld), C.byref(inf1))
        assert e.value.code == L.EINVAL and str(stray) in str(e.value), (stray, str(e.value))
        with pytest.raises(L.SmnError) as e:
            ctx.call("smn_spr_loss_grad", L.F64, stray, L.ACT["relu"], 2, 1.0, 0.3, 1.0, x.ptr, n, d, d, y.ptr, 0.1, 0.0, 1.0,
                     C.byref(q1), C.byref(ld), C.byref(inf1), t4)
        assert e.value.code == L.EINVAL and str(stray) in str(e.value), (stray, str(e.value))
    model, _ = make_model("mlp", 2, "relu", "gp", np.float64, x64, y64)
    starts = {k: np.array([float(v.value), float(v.value) + 0.1]) for k, v in train.train_vars(model).items()}
    with pytest.raises(NotImplementedError):
        train.build_multistart_step(model, starts)(1e-2)


def test_fused_entries_equal_the_composed_ones(L, ctx):
    """smn_spr_loss with the flag == smn_lml of the Theta that smn_kernel_mlp builds + eps I (to rounding: two builds of the
    same matrix, one factorisation each), for both nets."""
    x64, y64 = N.reg_data(129)
    x, y = ctx.to_device(np.ascontiguousarray(x64)), ctx.to_device(np.ascontiguousarray(y64[:, None]))
    for family, net in (("mlp", L.NET_MLP), ("resnet", L.NET_DENSE_RESNET)):
        got = spr_loss(L, ctx, x, y, net | L.NET_NTK, eps=5e-2)
        th = N.theta(family, x64, None, 2, "relu", 1.0, 0.3, 1.0)
        ref = N.logpdf(th + 5e-2 * np.eye(129), y64, "gp", 1.0, 1.0)
        print(family, got[0], ref)
        assert got[3] == 0 and abs(got[0] - ref) < 1e-9 * abs(ref)


# ----------------------------------------------------------------------------------------------------------- training
@pytest.mark.parametrize("objective", ["lml", "loo"])
def test_five_adam_steps_lower_the_loss_on_syn_t(objective):
    from smnngp import train
    from smnngp.spax.kernels import NTKKernel
    from smnngp.spax.likelihoods import StudentTLikelihood
    from smnngp.spax.models import SPR
    num = 300
    rs = np.random.RandomState(761)
    xx = np.linspace(-num / 2, num / 2, num)[:, None]
    yy = rs.multivariate_normal(mean=np.zeros(num), cov=np.exp(-0.5 * (xx - xx.T) ** 2), size=1).flatten() + rs.standard_t(df=1, size=num) * 0.8
    idx = np.random.RandomState(10).permutation(num)
    xx, yy = xx[idx][:240], yy[idx][:240]
    xtr, ytr = (xx - xx.mean(0)) / xx.std(0), (yy - yy.mean()) / yy.std()
    kernel = NTKKernel(factory("mlp", 2, "relu"), 1.0, 1.0, 1.0)
    model = SPR(kernel, StudentTLikelihood(2.0, 2.0), xtr, ytr, 0.0, 1.0, eps=1e-2)
    value = model.loo_loss if objective == "loo" else model.loss
    start = value()
    step = train.build_train_step(model, method="analytic", objective=objective)
    seen = [step(0.03) for _ in range(5)]
    end = value()
    print("syn-t %s: %.6f -> %s -> %.6f" % (objective, start, ["%.6f" % v for v in seen], end))
    assert abs(seen[0] - start) < 1e-9 * max(1.0, abs(start))
    assert np.isfinite(end) and end < start
    auto = train.build_train_step(model, method="auto", objective=objective)
    assert np.isfinite(auto(0.03))


def test_checkpoint_of_an_ntk_model_restores():
    from smnngp import checkpoint as CK
    x, y = N.reg_data(65)
    model, _ = make_model("resnet", 2, "erf", "tp", np.float64, x, y)
    run = tempfile.mkdtemp(prefix="smnngp_ntk_")
    CK.Checkpointer(run).save(1, model.vars())
    args = dict(method="tp", network="resnet", num_hiddens=2, activation="erf", last_w_std=N.HYP["last_w_std"])
    CK.save_meta(run, dict(args, kernel="ntk"))
    restored, _ = CK.restore_spr(run, x, y, 0.0, 1.0, dtype=np.float64)
    assert type(restored.kernel).__name__ == "NTKKernel" and restored.loss() == model.loss()
    CK.save_meta(run, args)                                   # no `kernel` field: "nngp", as every earlier run directory
    plain, _ = CK.restore_spr(run, x, y, 0.0, 1.0, dtype=np.float64)
    assert type(plain.kernel).__name__ == "NNGPKernel" and plain.loss() != model.loss()
    for f in os.listdir(run):
        os.remove(os.path.join(run, f))
    os.rmdir(run)
