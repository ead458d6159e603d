"""GPU tests of the exact C-output GP / Student-t process (spax.models.MultiSPR and the *_multi entries of the C ABI)
against the fp64 NumPy rules of tests/_multi_rules.py.  Tolerances are the project's: loss 1e-9 (fp64) / 1e-3 (fp32) of
max(1, |ref|), gradients 2e-6 / 1e-2 of max(largest reference gradient, |ref|), contraction terms 1e-9 * sum |G| |dK|,
posterior outputs relerr_norm 1e-7 / 1e-2.  No wall-clock assertion anywhere."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _cnn_grad_rules as R  # noqa: E402
import _multi_rules as M  # noqa: E402
from _tol import relerr_norm  # noqa: E402

HYP = M.HYP
DTYPES = [np.float64, np.float32]
DENSE = [(fam, act, n, c) for n, c in M.DENSE_NC for fam, act in M.DENSE_NETS]
CONV = [(h, w, ch, n, c, act) for h, w, ch in M.CONV_IMAGES for n, c in M.CONV_NC for act in ("relu", "erf")]


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


def make_model(family, x, y, layers, act, method, dtype, hyp=HYP, single=False):
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood
    from smnngp.spax.models import SPR, MultiSPR
    factory = {"mlp": lambda w, b, l: nt_kernels.get_mlp_kernel(layers, act=act, w_std=w, b_std=b, last_w_std=l),
               "resnet": lambda w, b, l: nt_kernels.get_dense_resnet_kernel(layers, act=act, w_std=w, b_std=b, last_w_std=l),
               "cnn": lambda w, b, l: nt_kernels.get_cnn_kernel(layers, 1, act=act, w_std=w, b_std=b, last_w_std=l),
               "conv_resnet": lambda w, b, l: nt_kernels.get_conv_resnet_kernel(layers, 1, act=act, w_std=w, b_std=b,
                                                                               last_w_std=l)}[family]
    with np.errstate(divide="ignore"):      # a value of exactly 0 is stored as raw = -inf (softplus-inverse of 0)
        kernel = NNGPKernel(factory, hyp["w_std"], hyp["b_std"], hyp["last_w_std"])
        lik = GaussianLikelihood() if method == "gp" else StudentTLikelihood(hyp["alpha"], hyp["beta"])
        if single:
            model = SPR(kernel, lik, np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype), 0.0, 1.0, eps=hyp["eps"])
        else:
            model = MultiSPR(kernel, lik, np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype), eps=hyp["eps"])
    vmap = {"w_std": kernel.w_std, "b_std": kernel.b_std, "last_w_std": kernel.last_w_std, "eps": model.eps}
    if method == "tp":
        vmap.update(alpha=lik.a, beta=lik.b)
    return model, vmap


def keys_of(method):
    return M.KEYS if method == "tp" else M.KEYS[:4]


def constrained_grads(model, vmap, grads, method):
    """d loss / d constrained value: the softplus chain rule undone."""
    names = {id(v): k for k, v in model.vars().items()}
    return {k: grads[names[id(vmap[k])]] / float(vmap[k].constraint.grad(vmap[k].value)) for k in keys_of(method)}


def dense_key(n, c, dtype):
    return ("dense", n, c, dtype == np.float32)


def conv_key(n, c, h, w, ch, dtype):
    return ("conv", n, c, h, w, ch, dtype == np.float32)


# ------------------------------------------------------------------------------------- 1. C = 1 is the single-output model
@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("family,act,key", [("mlp", "relu", ("dense", 37, 3)), ("resnet", "erf", ("dense", 130, 10)),
                                            ("cnn", "relu", ("conv", 20, 3, 6, 6, 2))])
def test_one_column_equals_spr(family, act, key, method):
    """Loss, every gradient and test_nll of MultiSPR on one column within 1e-12 relative of SPR's, fp64."""
    x, y, _, xt, yt, _ = M.DATA[key[0]](*key[1:], False)
    layers = M.DENSE_LAYERS if key[0] == "dense" else M.CONV_LAYERS
    multi, _ = make_model(family, x, y[:, :1], layers, act, method, np.float64)
    single, _ = make_model(family, x, y[:, 0], layers, act, method, np.float64, single=True)

    def close(a, b):
        print("multi %.17g single %.17g" % (a, b))
        return abs(a - b) <= 1e-12 * abs(b)

    assert close(multi.loss(), single.loss())
    lm, gm = multi.loss_and_grad()
    ls, gs = single.loss_and_grad()
    assert close(lm, ls)
    assert sorted(k.split(".", 1)[1] for k in gm) == sorted(k.split(".", 1)[1] for k in gs)
    for k, v in gs.items():
        assert close(gm[k.replace("(SPR)", "(MultiSPR)")], v), k
    assert close(multi.test_nll(xt, yt[:, :1]), single.test_nll(xt, yt[:, 0]))


# ------------------------------------------------------------------------------------------------------- 2. loss parity
def check_loss(got, ref, dtype):
    print("loss %.15g reference %.15g" % (got, ref))
    assert abs(got - ref) < (1e-9 if dtype == np.float64 else 1e-3) * max(1.0, abs(ref))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("family,act,n,c", DENSE)
def test_dense_loss_matches_the_rules(family, act, n, c, method, dtype):
    key = dense_key(n, c, dtype)
    x, y = M.dense_data(*key[1:])[:2]
    model, _ = make_model(family, x, y, M.DENSE_LAYERS, act, method, dtype)
    check_loss(model.loss(), M.ref_loss(family, key, M.DENSE_LAYERS, act, method), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("h,w,ch,n,c,act", CONV)
def test_conv_loss_matches_the_rules(h, w, ch, n, c, act, method, dtype):
    key = conv_key(n, c, h, w, ch, dtype)
    x, y = M.conv_data(*key[1:])[:2]
    model, _ = make_model("cnn", x, y, M.CONV_LAYERS, act, method, dtype)
    check_loss(model.loss(), M.ref_loss("cnn", key, M.CONV_LAYERS, act, method), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", ["gp", "tp"])
def test_conv_resnet_loss_matches_the_rules(method, dtype):
    key = conv_key(12, 3, 8, 8, 1, dtype)
    x, y = M.conv_data(*key[1:])[:2]
    model, _ = make_model("conv_resnet", x, y, 1, "relu", method, dtype)
    check_loss(model.loss(), M.ref_loss("conv_resnet", key, 1, "relu", method), dtype)


# ---------------------------------------------------------------------------------------------- 3. the contraction alone
def padded(ctx, a, ld, dtype=np.float64):
    out = np.zeros((a.shape[0], ld), dtype=dtype)
    out[:, :a.shape[1]] = a
    return ctx.to_device(out)


@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("family,act,n,c", DENSE)
def test_dense_contraction_alone_against_the_numpy_rules(L, ctx, family, act, n, c, method):
    """smn_lml_grad_terms_multi fed -K~^-1 and A computed in NumPy, fp64: each term within 1e-9 * sum |G| |dK~/d theta|."""
    x, y = M.dense_data(n, c, False)[:2]
    k, kw, kb = M.dense_tangents(family, x, M.DENSE_LAYERS, act, HYP["w_std"], HYP["b_std"], HYP["last_w_std"])
    g, a, nkinv, coef = M.g_parts(k, y, HYP["eps"], method, HYP["alpha"], HYP["beta"])[:4]
    ref, bound = R.terms_from(g, k, kw, kb, HYP["w_std"], HYP["b_std"], HYP["last_w_std"])
    ld = (n + 1) // 2 * 2
    xd = ctx.to_device(np.ascontiguousarray(x))
    k0, q = ctx.empty((n, ld), np.float64), ctx.empty((n,), np.float64)
    ctx.call("smn_gram", L.F64, xd.ptr, n, M.DENSE_D, None, 0, 0, M.DENSE_D, k0.ptr, ld, q.ptr, None)
    kd, ad = padded(ctx, nkinv, ld), ctx.to_device(np.ascontiguousarray(a))
    terms = (C.c_double * 4)()
    net = L.NET_MLP if family == "mlp" else L.NET_DENSE_RESNET
    ctx.call("smn_lml_grad_terms_multi", L.F64, net, L.ACT[act], M.DENSE_LAYERS, HYP["w_std"], HYP["b_std"],
             HYP["last_w_std"], k0.ptr, n, ld, q.ptr, kd.ptr, ld, ad.ptr, c, coef, terms)
    for i in range(4):
        print("term %d got %.15g ref %.15g err %.3g bound %.3g" % (i, terms[i], ref[i], abs(terms[i] - ref[i]), 1e-9 * bound[i]))
        assert abs(terms[i] - ref[i]) <= 1e-9 * bound[i], (i, terms[i], ref[i])


def conv_terms(L, ctx, x, layers, act, nkinv, a, coef):
    n, h, w, ch = x.shape
    xd, kd, ad = (ctx.to_device(np.ascontiguousarray(v, dtype=np.float64)) for v in (x, nkinv, a))
    terms = (C.c_double * 4)()
    ctx.call("smn_kernel_cnn_grad_terms_multi", L.F64, L.ACT[act], layers, HYP["w_std"], HYP["b_std"], HYP["last_w_std"],
             xd.ptr, n, h, w, ch, kd.ptr, n, ad.ptr, a.shape[1], coef, terms)
    return np.array(list(terms))


@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("h,w,ch,n,c,act", CONV)
def test_conv_contraction_alone_against_the_numpy_rules(L, ctx, h, w, ch, n, c, act, method):
    x, y = M.conv_data(n, c, h, w, ch, False)[:2]
    k, kw, kb = R.tangent_matrices(x, M.CONV_LAYERS, act, HYP["w_std"], HYP["b_std"], HYP["last_w_std"])
    g, a, nkinv, coef = M.g_parts(k, y, HYP["eps"], method, HYP["alpha"], HYP["beta"])[:4]
    ref, bound = R.terms_from(g, k, kw, kb, HYP["w_std"], HYP["b_std"], HYP["last_w_std"])
    got = conv_terms(L, ctx, x, M.CONV_LAYERS, act, nkinv, a, coef)
    again = conv_terms(L, ctx, x, M.CONV_LAYERS, act, nkinv, a, coef)
    for i in range(4):
        print("term %d got %.15g ref %.15g err %.3g bound %.3g" % (i, got[i], ref[i], abs(got[i] - ref[i]), 1e-9 * bound[i]))
        assert abs(got[i] - ref[i]) <= 1e-9 * bound[i], (i, got[i], ref[i])
    assert got.tobytes() == again.tobytes()


# --------------------------------------------------------------------------------------------------- 4. loss_and_grad
def check_loss_and_grad(model, vmap, family, key, layers, act, dtype, hyp=HYP, skip=()):
    """Under the Student-t head, all six variables: against the rules' analytic gradient AND their central differences."""
    f64 = dtype == np.float64
    loss, grads = model.loss_and_grad()
    rl, ra = M.ref_grad(family, key, layers, act, "tp", hyp)
    fd = M.ref_fd(family, key, layers, act, "tp", hyp)
    check_loss(loss, rl, dtype)
    # loss() builds K by the fused kernel, loss_and_grad() by the recursion over the Gram matrix: each is held to the rules above
    assert abs(loss - model.loss()) < (2e-9 if f64 else 2e-3) * max(1.0, abs(rl))
    assert set(grads) == set(model.vars()) and all(np.isfinite(g) for g in grads.values()), grads
    got = constrained_grads(model, vmap, grads, "tp")
    tol = 2e-6 if f64 else 1e-2
    for name, ref in (("analytic", ra), ("differences", fd)):
        scale = max(abs(v) for k, v in ref.items() if k not in skip)
        for k in M.KEYS:
            if k in skip:
                continue
            err = abs(got[k] - ref[k]) / max(scale, abs(ref[k]))
            print("%s %s got %.12g ref %.12g err %.3g (tol %g)" % (name, k, got[k], ref[k], err, tol))
            assert err < tol, (name, k, got[k], ref[k])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,act,n,c", DENSE)
def test_dense_loss_and_grad_matches_the_rules(family, act, n, c, dtype):
    key = dense_key(n, c, dtype)
    x, y = M.dense_data(*key[1:])[:2]
    model, vmap = make_model(family, x, y, M.DENSE_LAYERS, act, "tp", dtype)
    check_loss_and_grad(model, vmap, family, key, M.DENSE_LAYERS, act, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h,w,ch,n,c,act", CONV)
def test_conv_loss_and_grad_matches_the_rules(h, w, ch, n, c, act, dtype):
    key = conv_key(n, c, h, w, ch, dtype)
    x, y = M.conv_data(*key[1:])[:2]
    model, vmap = make_model("cnn", x, y, M.CONV_LAYERS, act, "tp", dtype)
    check_loss_and_grad(model, vmap, "cnn", key, M.CONV_LAYERS, act, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,act,key", [("mlp", "relu", ("dense", 37, 3)), ("cnn", "erf", ("conv", 20, 3, 6, 6, 2))])
def test_loss_and_grad_with_the_default_b_std(family, act, key, dtype):
    """b_std = 1e-8 (the reference's default): every value finite, the other five gradients within tolerance; a relative
    step is useless for b_std there, so that one entry is not compared."""
    key = key + (dtype == np.float32,)
    x, y = M.DATA[key[0]](*key[1:])[:2]
    layers = M.DENSE_LAYERS if key[0] == "dense" else M.CONV_LAYERS
    hyp = dict(HYP, b_std=1e-8)
    model, vmap = make_model(family, x, y, layers, act, "tp", dtype, hyp)
    check_loss_and_grad(model, vmap, family, key, layers, act, dtype, hyp, skip=("b_std",))


# ------------------------------------------------------------------------------------------------------- 5. prediction
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,act,layers,key", M.PRED_CASES)
def test_prediction_nll_and_classification(family, act, layers, key, dtype):
    f32 = dtype == np.float32
    x, y, lab, xt, yt, labt = M.DATA[key[0]](*key[1:], f32)
    ref = M.ref_prediction(family, act, layers, key, f32)
    tol = 1e-2 if f32 else 1e-7
    for method in ("gp", "tp"):
        model, _ = make_model(family, x, y, layers, act, method, dtype)
        mean, cov = model.predict(np.asarray(xt, dtype=dtype))
        mean, var = np.asarray(mean, dtype=np.float64), np.asarray(cov.diagonal(), dtype=np.float64)
        assert mean.shape == ref["mean"].shape and var.shape == ref["var"].shape
        print("mean err %.3g var err %.3g" % (relerr_norm(mean, ref["mean"]), relerr_norm(var, ref["var"])))
        assert relerr_norm(mean, ref["mean"]) < tol and relerr_norm(var, ref["var"]) < tol
        nll = model.test_nll(np.asarray(xt, dtype=dtype), yt)
        print("%s test_nll %.15g reference %.15g" % (method, nll, ref["nll_" + method]))
        assert abs(nll - ref["nll_" + method]) < tol * max(1.0, abs(ref["nll_" + method]))
        got = model.classify(np.asarray(xt, dtype=dtype))
        assert np.array_equal(got, ref["labels"])
        assert model.accuracy(np.asarray(xt, dtype=dtype), labt) == float(np.mean(ref["labels"] == labt))


def test_from_labels_builds_the_classifier():
    from smnngp.spax.models import MultiSPR
    x, y, lab, xt, _, _ = M.dense_data(37, 3, False)
    model, _ = make_model("mlp", x, M.label_targets(lab, 3), M.DENSE_LAYERS, "relu", "gp", np.float64)
    other = MultiSPR.from_labels(model.kernel, model.likelihood, x, lab, 3, eps=HYP["eps"])
    assert other.num_outputs == 3 and other.loss() == model.loss()
    assert np.array_equal(other.classify(xt), model.classify(xt))


# ------------------------------------------------------------------------------------------------------ 6. determinism
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,act,key", [("mlp", "erf", ("dense", 100, 48)), ("resnet", "relu", ("dense", 130, 10)),
                                            ("cnn", "relu", ("conv", 36, 10, 8, 8, 3))])
def test_two_calls_give_identical_bits(family, act, key, dtype):
    x, y = M.DATA[key[0]](*key[1:], dtype == np.float32)[:2]
    layers = M.DENSE_LAYERS if key[0] == "dense" else M.CONV_LAYERS
    model, _ = make_model(family, x, y, layers, act, "tp", dtype)
    first, again = model.loss_and_grad(), model.loss_and_grad()
    assert np.float64(first[0]).tobytes() == np.float64(again[0]).tobytes()
    for k in first[1]:
        assert np.float64(first[1][k]).tobytes() == np.float64(again[1][k]).tobytes(), k
    assert np.float64(model.loss()).tobytes() == np.float64(model.loss()).tobytes()


# --------------------------------------------------------------------------------------------- 7. not positive definite
@pytest.mark.parametrize("family", ["mlp", "cnn"])
def test_non_pd_matrix_gives_nan_and_ok(L, ctx, family):
    """Duplicate rows with eps = 0: info > 0, NaN loss and NaN gradients, no exception."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((12, 7)) if family == "mlp" else rng.standard_normal((12, 6, 6, 2))
    x = np.concatenate([x, x, x], axis=0).astype(np.float32)
    y = rng.standard_normal((36, 3)).astype(np.float32)
    model, _ = make_model(family, x, y, 2, "relu", "gp", np.float32, dict(HYP, eps=0.0))
    assert model.eps.safe_value == 0.0
    assert np.isnan(model.loss())
    loss, grads = model.loss_and_grad()
    assert np.isnan(loss) and set(grads) == set(model.vars()) and all(np.isnan(g) for g in grads.values())
    xd, yd = ctx.to_device(x), ctx.to_device(y)
    quad, logdet, info = C.c_double(), C.c_double(), C.c_int()
    cols, terms = (C.c_double * 3)(), (C.c_double * 4)()
    if family == "mlp":
        ctx.call("smn_spr_loss_grad_multi", L.F32, L.NET_MLP, L.ACT["relu"], 2, 1.3, 0.4, 0.9, xd.ptr, 36, 7, 7, yd.ptr, 3, 0.0,
                 0.0, 1.0, C.byref(quad), cols, C.byref(logdet), C.byref(info), terms)
    else:
        ctx.call("smn_spr_cnn_loss_grad_multi", L.F32, L.ACT["relu"], 2, 1.3, 0.4, 0.9, xd.ptr, 36, 6, 6, 2, yd.ptr, 3, 0.0,
                 0.0, 1.0, C.byref(quad), cols, C.byref(logdet), C.byref(info), terms)
    assert info.value > 0 and all(np.isnan(t) for t in terms) and np.isnan(quad.value) and np.isnan(logdet.value)
    assert all(np.isnan(v) for v in cols)
    lp = C.c_double()
    if family == "mlp":
        ctx.call("smn_spr_loss_multi", L.F32, L.NET_MLP, L.ACT["relu"], 2, 1.3, 0.4, 0.9, xd.ptr, 36, 7, 7, yd.ptr, 3, 0.0, 0.0,
                 1.0, C.byref(lp), C.byref(quad), cols, C.byref(logdet), C.byref(info))
        assert info.value > 0 and np.isnan(lp.value) and np.isnan(quad.value) and all(np.isnan(v) for v in cols)


# ------------------------------------------------------------------------------------------------------------ 8. limits
def test_more_than_48_columns_is_not_supported(L, ctx):
    rng = np.random.default_rng(2)
    n, c = 20, 49
    x, xi = ctx.to_device(rng.standard_normal((n, 7))), ctx.to_device(rng.standard_normal((n, 6, 6, 1)))
    y, k = ctx.to_device(rng.standard_normal((n, c))), ctx.to_device(np.eye(n))
    out = [C.c_double() for _ in range(4)]
    info, terms = C.c_int(), (C.c_double * 4)()
    calls = [
        ("smn_lml_multi", L.F64, k.ptr, n, n, y.ptr, c, 1e-3, 0.0, 1.0, C.byref(out[0]), C.byref(out[1]), None,
         C.byref(out[2]), C.byref(info)),
        ("smn_spr_loss_multi", L.F64, L.NET_MLP, 0, 2, 1.3, 0.4, 0.9, x.ptr, n, 7, 7, y.ptr, c, 1e-3, 0.0, 1.0, C.byref(out[0]),
         C.byref(out[1]), None, C.byref(out[2]), C.byref(info)),
        ("smn_lml_grad_terms_multi", L.F64, L.NET_MLP, 0, 2, 1.3, 0.4, 0.9, k.ptr, n, n, y.ptr, k.ptr, n, y.ptr, c, 1.0, terms),
        ("smn_kernel_cnn_grad_terms_multi", L.F64, 0, 2, 1.3, 0.4, 0.9, xi.ptr, n, 6, 6, 1, k.ptr, n, y.ptr, c, 1.0, terms),
        ("smn_spr_loss_grad_multi", L.F64, L.NET_MLP, 0, 2, 1.3, 0.4, 0.9, x.ptr, n, 7, 7, y.ptr, c, 1e-3, 0.0, 1.0,
         C.byref(out[0]), None, C.byref(out[1]), C.byref(info), terms),
        ("smn_spr_cnn_loss_grad_multi", L.F64, 0, 2, 1.3, 0.4, 0.9, xi.ptr, n, 6, 6, 1, y.ptr, c, 1e-3, 0.0, 1.0,
         C.byref(out[0]), None, C.byref(out[1]), C.byref(info), terms),
    ]
    for call in calls:
        with pytest.raises(L.SmnError) as e:
            ctx.call(*call)
        assert e.value.code == L.ENOTSUP, call[0]
    # 48 columns are served
    y48 = ctx.to_device(rng.standard_normal((n, 48)))
    ctx.call("smn_spr_loss_multi", L.F64, L.NET_MLP, 0, 2, 1.3, 0.4, 0.9, x.ptr, n, 7, 7, y48.ptr, 48, 1e-3, 0.0, 1.0,
             C.byref(out[0]), C.byref(out[1]), None, C.byref(out[2]), C.byref(info))
    assert info.value == 0 and np.isfinite(out[0].value)


def test_conv_resnet_has_no_analytic_gradient():
    from smnngp import train
    x, y = M.conv_data(12, 3, 8, 8, 1, False)[:2]
    model, _ = make_model("conv_resnet", x, y, 1, "relu", "gp", np.float64)
    with pytest.raises(NotImplementedError):
        model.loss_and_grad()
    with pytest.raises(NotImplementedError):
        train.build_train_step(model, method="analytic")(1e-2)


def test_images_above_the_limit_are_refused_and_auto_falls_back(L, ctx):
    from smnngp import train
    rng = np.random.default_rng(9)
    n, h, w, ch, c = 6, 40, 40, 1, 3
    x, y = rng.standard_normal((n, h, w, ch)), rng.standard_normal((n, c))
    xd, yd = ctx.to_device(x), ctx.to_device(y)
    quad, logdet, info = C.c_double(), C.c_double(), C.c_int()
    terms = (C.c_double * 4)()
    with pytest.raises(L.SmnError) as e:
        ctx.call("smn_spr_cnn_loss_grad_multi", L.F64, L.ACT["relu"], 2, 1.3, 0.4, 0.9, xd.ptr, n, h, w, ch, yd.ptr, c, 5e-2,
                 0.0, 1.0, C.byref(quad), None, C.byref(logdet), C.byref(info), terms)
    assert e.value.code == L.ENOTSUP and "1024" in str(e.value)
    model, _ = make_model("cnn", x, y, 2, "relu", "gp", np.float64, dict(HYP, eps=5e-2))
    with pytest.raises(NotImplementedError):
        model.loss_and_grad()
    before = {k: float(v.value) for k, v in model.vars().items()}
    value = train.build_train_step(model, method="auto")(1e-2)
    assert np.isfinite(value) and any(float(v.value) != before[k] for k, v in model.vars().items())


# ---------------------------------------------------------------------------------------------------------- 9. training
@pytest.mark.parametrize("family,act,key", [("mlp", "relu", ("dense", 37, 3)), ("cnn", "relu", ("conv", 20, 3, 6, 6, 2))])
def test_three_adam_steps_follow_the_rules_gradients(family, act, key):
    """build_train_step on a MultiSPR against a shadow Adam fed the rules' analytic gradients at the shadow's own values."""
    from smnngp import train
    from smnngp.spax.base import TrainVar
    x, y = M.DATA[key[0]](*key[1:], False)[:2]
    layers = M.DENSE_LAYERS if key[0] == "dense" else M.CONV_LAYERS
    model, vmap = make_model(family, x, y, layers, act, "tp", np.float64)
    assert set(train.train_vars(model)) == set(model.vars())
    names = {id(v): k for k, v in model.vars().items()}
    shadow = {k: TrainVar(float(v.value)) for k, v in model.vars().items()}
    adam = train.Adam(shadow)
    step = train.build_train_step(model, method="analytic")
    for it in range(3):
        hyp = {k: float(vmap[k].constraint(shadow[names[id(vmap[k])]].value)) for k in M.KEYS}
        rl, rg = M.loss_grad(family, x, y, layers, act, "tp", **hyp)
        raw = {names[id(vmap[k])]: rg[k] * float(vmap[k].constraint.grad(shadow[names[id(vmap[k])]].value)) for k in M.KEYS}
        before = {k: float(v.value) for k, v in shadow.items()}
        adam(1e-2, raw)
        value = step(1e-2)
        assert abs(value - rl) < 1e-9 * max(1.0, abs(rl))
        for k, v in model.vars().items():
            got, want = float(v.value) - before[k], float(shadow[k].value) - before[k]
            print("step %d %s update %.12g reference %.12g" % (it, k, got, want))
            assert abs(got - want) < 2e-6 * max(abs(want), 1e-2), (it, k, got, want)
    # method="auto" takes the analytic route too: the fused entry is called, no forward build from Python
    model2, _ = make_model(family, x, y, layers, act, "tp", np.float64)
    c2 = model2.x_data.ctx
    calls, orig = [], c2.call

    def counting(name, *args):
        calls.append(name)
        return orig(name, *args)

    c2.call = counting
    try:
        train.build_train_step(model2, method="auto")(1e-2)
    finally:
        del c2.call
    entry = "smn_spr_loss_grad_multi" if key[0] == "dense" else "smn_spr_cnn_loss_grad_multi"
    assert calls == [entry], calls


# --------------------------------------------------------------- the rectangle route of the factorisation (n_pad >= 8192)
def test_rectangle_route_carries_the_columns(L, ctx):
    """n = 8190, C = 3, fp64: from n_pad = 8192 on the gradient entries factor the rectangle [[K~], [I], [Y^T]] and read A off its
    appended rows; n + C crosses a 128-tile that n + 1 does not.  A NumPy reference of this size is minutes of work, so the
    check is between device calls: under the Gaussian head G = sum_c (a_c a_c^T - K~^-1), hence the joint terms are the SUM of
    the single-output entry's terms over the columns and the per-column quadratic forms are its quad.  Both sides factor the
    same fp64 matrix with the same kernels; they differ in the rows carried and in summation order only, i.e. by a few
    units of cond(K~) * 2^-53 <= (1.5 n / eps) * 1.1e-16 = 1.4e-11: the bound is 1e-8 of sum_c |terms_c|.  One column
    through the multi entry returns the single-output entry's values (1e-12 relative)."""
    rng = np.random.default_rng(8190)
    n, c, d, eps = 8190, 3, 7, 1e-1
    x = ctx.to_device(rng.standard_normal((n, d)))
    yh = rng.standard_normal((n, c))
    y = ctx.to_device(yh)
    args = (L.F64, L.NET_MLP, L.ACT["relu"], 2, 1.3, 0.4, 0.9, x.ptr, n, d, d)

    def single(col):
        yc = ctx.to_device(np.ascontiguousarray(yh[:, col]))
        quad, logdet, info, terms = C.c_double(), C.c_double(), C.c_int(), (C.c_double * 4)()
        ctx.call("smn_spr_loss_grad", *args, yc.ptr, eps, 0.0, 1.0, C.byref(quad), C.byref(logdet), C.byref(info), terms)
        assert info.value == 0
        return quad.value, logdet.value, np.array(list(terms))

    def multi(yd, cols):
        quad, logdet, info, terms = C.c_double(), C.c_double(), C.c_int(), (C.c_double * 4)()
        qc = (C.c_double * cols)()
        ctx.call("smn_spr_loss_grad_multi", *args, yd.ptr, cols, eps, 0.0, 1.0, C.byref(quad), qc, C.byref(logdet),
                 C.byref(info), terms)
        assert info.value == 0
        return quad.value, np.array(list(qc)), logdet.value, np.array(list(terms))

    singles = [single(k) for k in range(c)]
    quad, qcols, logdet, terms = multi(y, c)
    want = sum(s[2] for s in singles)
    scale = sum(np.abs(s[2]) for s in singles)
    for i in range(4):
        print("term %d joint %.15g sum of columns %.15g scale %.3g" % (i, terms[i], want[i], scale[i]))
        assert abs(terms[i] - want[i]) <= 1e-8 * scale[i]
    for k in range(c):
        assert abs(qcols[k] - singles[k][0]) <= 1e-8 * singles[k][0]
    assert abs(quad - qcols.sum()) <= 1e-14 * quad and abs(logdet - singles[0][1]) <= 1e-10 * abs(logdet)
    q1, qc1, ld1, t1 = multi(ctx.to_device(np.ascontiguousarray(yh[:, :1])), 1)
    assert abs(q1 - singles[0][0]) <= 1e-12 * q1 and abs(ld1 - singles[0][1]) <= 1e-12 * abs(ld1)
    assert np.all(np.abs(t1 - singles[0][2]) <= 1e-12 * np.abs(singles[0][2]))


# ------------------------------------------------------ the fused entries start from one factored posterior (heads.hip)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_entries_share_one_factorisation(L, ctx, dtype):
    """n = 129, d = 5, MLP-ReLU with two layers, eps_abs = 0.1: smn_spr_loss_grad, smn_spr_loss_grad_multi (c = 1),
    smn_spr_kinv (c = 1) and smn_spr_loo_grad (c = 1) all build the same K~ and factor it with the same identity block, so
    what each of them reports of that factorisation -- quad, logdet, info -- is the same bits."""
    rng = np.random.default_rng(129)
    n, d, ld = 129, 5, 132
    x, y = ctx.to_device(rng.standard_normal((n, d)).astype(dtype)), ctx.to_device(rng.standard_normal(n).astype(dtype))
    args = (L.dtype_code(np.dtype(dtype)), L.NET_MLP, L.ACT["relu"], 2, 1.3, 0.4, 0.9, x.ptr, n, d, d, y.ptr)
    quad, logdet, info = [C.c_double() for _ in range(2)], [C.c_double() for _ in range(3)], [C.c_int(-1) for _ in range(4)]
    terms, dhead, lam = (C.c_double * 4)(), (C.c_double * 2)(), C.c_double()
    ctx.call("smn_spr_loss_grad", *args, 0.1, 0.0, 1.0, C.byref(quad[0]), C.byref(logdet[0]), C.byref(info[0]), terms)
    ctx.call("smn_spr_loss_grad_multi", *args, 1, 0.1, 0.0, 1.0, C.byref(quad[1]), None, C.byref(logdet[1]), C.byref(info[1]),
             terms)
    ninv, alpha = ctx.empty((n, ld), dtype), ctx.empty((n, 1), dtype)
    ctx.call("smn_spr_kinv", *args, 1, 0.1, ninv.ptr, ld, alpha.ptr, C.byref(logdet[2]), C.byref(info[2]))
    ctx.call("smn_spr_loo_grad", *args, 1, 0.1, 0.0, 1.0, C.byref(lam), dhead, C.byref(info[3]), terms, None, None)
    print("quad", [q.value for q in quad], "logdet", [v.value for v in logdet], "info", [i.value for i in info])
    assert info[0].value == 0 and np.isfinite(quad[0].value) and np.isfinite(logdet[0].value)
    assert quad[1].value == quad[0].value and logdet[1].value == logdet[0].value and info[1].value == info[0].value
    assert logdet[2].value == logdet[0].value and info[2].value == info[0].value
    assert info[3].value == info[0].value
