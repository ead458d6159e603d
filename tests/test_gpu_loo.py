"""GPU tests of leave-one-out cross-validation (csrc/loo.hip: smn_loo_head, smn_loo_multi, smn_spr_loo_grad,
smn_spr_cnn_loo_grad; spax.models.SPR / MultiSPR loo_*; train.build_train_step(objective="loo")) against the fp64 NumPy rules
of tests/_loo_rules.py.  No wall-clock assertion anywhere; every figure is printed before it is asserted."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _loo_rules as LR  # noqa: E402
import _multi_rules as M  # noqa: E402
from _tol import relerr_norm  # noqa: E402

HEAD = dict(alpha=1.7, beta=2.4)
U = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}
DTYPES = [np.float64, np.float32]
# G's element-wise rounding bound is K_G (n + 8) u g_abs_ij.  The product sums n_pad terms N_ik (N_jk d_k) in the MFMA
# accumulator, one after the other: (n - 1) additions and n products, each operand of which carries the one rounding of the
# column scaling, plus d_k itself rounded to the storage type -- (n + 2) u in all; the rank-2C terms are summed in fp64 and the
# entry is rounded once more: (n + 3) u to first order, inside (n + 8) u.  The factor 2 is for what the MFMA does inside one
# instruction (the order and rounding of its four products is not documented) and for the second-order terms.
K_G = 2.0
# End to end, the largest error / (cond(K~) u) measured over the cases below (profiles/r12_loo.txt); asserted at 8x that for
# shape-to-shape variation.  Nothing may need more than 64 cond u.
MEASURED = {np.float64: 1.1, np.float32: 3.4}


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


def head_params(method):
    return (0.0, 1.0) if method == "gp" else (2.0 * HEAD["alpha"], HEAD["beta"] / HEAD["alpha"])


def run_head(L, ctx, nk, a, y, dtype, method, want_g=True):
    """smn_loo_head on host arrays (already representable in `dtype`) -> (Lambda, mean, scale2, dhead, G or None)."""
    n, c = y.shape
    df, scale = head_params(method)
    nk_d, a_d, y_d = (ctx.to_device(np.ascontiguousarray(v, dtype=dtype)) for v in (nk, a, y))
    mean, scale2 = ctx.empty((n, c), dtype), ctx.empty((n,), dtype)
    g = ctx.to_device(np.full((n, n), 7.0, dtype=dtype)) if want_g else None
    lam, dhead = C.c_double(), (C.c_double * 2)()
    ctx.call("smn_loo_head", L.dtype_code(dtype), nk_d.ptr, n, a_d.ptr, y_d.ptr, n, c, df, scale, C.byref(lam), mean.ptr,
             scale2.ptr, dhead, g.ptr if want_g else None, n)
    return lam.value, mean.raw_numpy(), scale2.raw_numpy(), np.array(list(dhead)), g.raw_numpy() if want_g else None


def check_head(got, ref, nk, a, y, dtype, rows=None):
    """Lambda, mean, scale2, dhead and G (all rows, or `rows`) of one head call against the rules fed the same values."""
    lam, mean, scale2, dhead, g = got
    n, c = y.shape
    u, u64 = U[dtype], U[np.float64]
    # fp64 sums of n terms in a tree, each term a handful of libm calls (a few ulp each): (n + 64) u64 of the terms' magnitudes
    tol = (n + 64) * u64 * ref["lam_abs"]
    print("Lambda %.15g rules %.15g  |diff| %.3g  bound %.3g" % (lam, ref["lam"], abs(lam - ref["lam"]), tol))
    assert abs(lam - ref["lam"]) <= tol
    for k in range(2):
        tol = (n + 64) * u64 * ref["dhead_abs"][k]
        print("dhead[%d] %.15g rules %.15g  bound %.3g" % (k, dhead[k], ref["dhead"][k], tol))
        assert abs(dhead[k] - ref["dhead"][k]) <= tol
    p = ref["p"]
    # one rounding to the storage type on top of fp64 arithmetic on the same inputs
    m_tol = 2.0 * u * (np.abs(y) + np.abs(a) / p[:, None])
    assert np.all(np.abs(mean - ref["mean"]) <= m_tol), float(np.max(np.abs(mean - ref["mean"]) / m_tol))
    # scale2: a handful of fp64 operations on each side and one rounding to the storage type.  The Student-t shape also carries
    # t_i = nu + (Q - e_i) / s; both sides take that difference from sums kept beyond fp64 (two-part sums on the device,
    # extended precision in the rules), so what is left is the tree that adds the points' shares of Q: at most 16 roundings of
    # the magnitude of Q on each side
    s_tol = 8.0 * u * ref["scale2"]
    if ref["df"] is not None:
        nu, s = 2.0 * HEAD["alpha"], HEAD["beta"] / HEAD["alpha"]
        s_tol = s_tol + 2.0 * 16.0 * u64 * ref["q_abs"] / s / (ref["scale2"] * p * ref["df"] / s) * ref["scale2"] * (n > 1)
    print("scale2: max |err| / bound = %.3g" % float(np.max(np.abs(scale2 - ref["scale2"]) / s_tol)))
    assert np.all(np.abs(scale2 - ref["scale2"]) <= s_tol)
    if g is None:
        return
    idx = np.arange(n) if rows is None else np.asarray(rows)
    low = np.arange(n)[None, :] <= idx[:, None]                      # the lower triangle of those rows
    err = np.abs(g[idx] - ref["g"])
    bound = K_G * (n + 8) * u * ref["g_abs"]
    ratio = float(np.max(np.where(low, err / bound, 0.0)))
    print("G: max |err| / (K_G (n + 8) u g_abs) = %.3g" % ratio)
    assert ratio <= 1.0
    if rows is None and n > 1:       # above the diagonal: the 64 x 64 diagonal blocks are mirrored, nothing else is written
        ii, jj = np.arange(n)[:, None], np.arange(n)[None, :]
        upper, block = jj > ii, (ii // 64) == (jj // 64)
        assert np.all(g[upper & ~block] == 7.0)
        assert np.array_equal(g[upper & block], g.T[upper & block])


# ---------------------------------------------------------------------------------------------------- 1. the head alone
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("c", [1, 3, 48])
@pytest.mark.parametrize("n", [1, 2, 127, 128, 129, 300])
def test_head_against_the_rules(L, ctx, n, c, method, dtype):
    f32 = dtype == np.float32
    nk, a, y = LR.head_case(n, c, f32)
    ref = LR.head_ref(n, c, f32, method, **HEAD)
    check_head(run_head(L, ctx, nk, a, y, dtype, method), ref, nk, a, y, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", ["gp", "tp"])
def test_head_is_reproducible_and_the_seed_is_optional(L, ctx, method, dtype):
    n, c = 300, 3
    nk, a, y = LR.head_case(n, c, dtype == np.float32)
    first = run_head(L, ctx, nk, a, y, dtype, method)
    second = run_head(L, ctx, nk, a, y, dtype, method)
    bare = run_head(L, ctx, nk, a, y, dtype, method, want_g=False)
    for x1, x2 in zip(first, second):
        assert np.array_equal(np.asarray(x1), np.asarray(x2))
    for x1, x3 in zip(first[:4], bare[:4]):
        assert np.array_equal(np.asarray(x1), np.asarray(x3))
    # only the lower triangle of the input is read
    junk = np.array(nk)
    junk[np.triu_indices(n, 1)] = np.nan
    third = run_head(L, ctx, junk, a, y, dtype, method)
    for x1, x3 in zip(first, third):
        assert np.array_equal(np.asarray(x1), np.asarray(x3))


def test_limits_and_bad_sizes(L, ctx):
    n = 6
    k, y49, y = ctx.to_device(np.eye(n)), ctx.to_device(np.ones((n, 49))), ctx.to_device(np.ones((n, 2)))
    x, xi = ctx.to_device(np.ones((n, 7))), ctx.to_device(np.ones((n, 40, 40, 1)))
    lam, dh, info, terms = C.c_double(), (C.c_double * 2)(), C.c_int(), (C.c_double * 4)()
    notsup = [("smn_loo_head", L.F64, k.ptr, n, y49.ptr, y49.ptr, n, 49, 0.0, 1.0, C.byref(lam), None, None, dh, None, 0),
              ("smn_loo_multi", L.F64, k.ptr, n, n, y49.ptr, 49, 1e-3, 0.0, 1.0, C.byref(lam), None, None, dh, None,
               C.byref(info), None, 0),
              ("smn_spr_loo_grad", L.F64, L.NET_MLP, 0, 2, 1.3, 0.4, 0.9, x.ptr, n, 7, 7, y49.ptr, 49, 1e-3, 0.0, 1.0,
               C.byref(lam), dh, C.byref(info), terms, None, None),
              ("smn_spr_cnn_loo_grad", L.F64, 0, 2, 1.3, 0.4, 0.9, xi.ptr, n, 40, 40, 1, y.ptr, 2, 1e-3, 0.0, 1.0, C.byref(lam),
               dh, C.byref(info), terms, None, None)]
    for call in notsup:
        with pytest.raises(L.SmnError) as e:
            ctx.call(*call)
        assert e.value.code == L.ENOTSUP, call[0]
    inval = [("smn_loo_head", L.F64, k.ptr, n - 1, y.ptr, y.ptr, n, 2, 0.0, 1.0, C.byref(lam), None, None, dh, None, 0),
             ("smn_loo_head", L.F64, k.ptr, n, y.ptr, y.ptr, 0, 2, 0.0, 1.0, C.byref(lam), None, None, dh, None, 0),
             ("smn_loo_head", L.F64, k.ptr, n, y.ptr, y.ptr, n, 2, 3.0, 0.0, C.byref(lam), None, None, dh, None, 0),
             ("smn_loo_multi", L.F64, k.ptr, n, n, y.ptr, 0, 1e-3, 0.0, 1.0, C.byref(lam), None, None, dh, None, C.byref(info),
              None, 0)]
    for call in inval:
        with pytest.raises(L.SmnError) as e:
            ctx.call(*call)
        assert e.value.code == L.EINVAL, call[0]


# ------------------------------------------------------------------------------------------------------- 2. end to end
DENSE = [(fam, act, n) for fam, act in (("mlp", "relu"), ("mlp", "erf"), ("resnet", "relu")) for n in (5, 129, 260)]
CONV = [(h, w, ch, layers) for h, w, ch in ((8, 8, 1), (4, 16, 3)) for layers in (0, 2)]
BASE = dict(w_std=1.3, b_std=0.4, last_w_std=0.9, **HEAD)


@functools.lru_cache(maxsize=None)
def e2e_case(family, act, layers, data_key):
    """(x, Y, hyper-parameters with eps chosen for cond(K~) <= 1e4, cond(K~)) of one end-to-end case."""
    x, y = M.DATA[data_key[0]](*data_key[1:])[:2]
    k = M.kernel(family, x, None, layers, act, BASE["w_std"], BASE["b_std"], BASE["last_w_std"])
    ev = np.linalg.eigvalsh(k)
    eps = float(ev[-1]) / 5000.0
    cond = float(np.linalg.cond(k + eps * np.eye(k.shape[0])))
    return x, y, dict(BASE, eps=eps), cond


@functools.lru_cache(maxsize=None)
def e2e_ref(family, act, layers, data_key, method):
    x, y, hyp, _ = e2e_case(family, act, layers, data_key)
    k = M.kernel(family, x, None, layers, act, hyp["w_std"], hyp["b_std"], hyp["last_w_std"])
    r = LR.from_matrix(k + hyp["eps"] * np.eye(k.shape[0]), y, method, hyp["alpha"], hyp["beta"])
    if family == "conv_resnet":
        return r, None, None, None
    _, grads, terms, terms_abs = LR.loss_grad(family, x, y, layers, act, method, **hyp)
    keys = LR.KEYS if method == "tp" else LR.KEYS[:4]
    fds = [LR.loss_fd(family, x, y, layers, act, method, keys, h=h, **hyp) for h in (1e-4, 2e-4, 5e-5)]
    return r, grads, (terms, terms_abs), fds


def device_e2e(L, ctx, family, act, layers, x, y, hyp, method, dtype):
    """(Lambda, dhead, terms or None, mean, scale2) from the fused entry of the family (smn_loo_multi for the conv ResNet)."""
    n, c = y.shape
    df, scale = head_params(method)
    xd, yd = ctx.to_device(np.ascontiguousarray(x, dtype=dtype)), ctx.to_device(np.ascontiguousarray(y, dtype=dtype))
    mean, scale2 = ctx.empty((n, c), dtype), ctx.empty((n,), dtype)
    lam, dh, info, terms = C.c_double(), (C.c_double * 2)(), C.c_int(), (C.c_double * 4)()
    code = L.dtype_code(dtype)
    w, b, lw, eps = hyp["w_std"], hyp["b_std"], hyp["last_w_std"], hyp["eps"]
    if family in ("mlp", "resnet"):
        net = L.NET_MLP if family == "mlp" else L.NET_DENSE_RESNET
        ctx.call("smn_spr_loo_grad", code, net, L.ACT[act], layers, w, b, lw, xd.ptr, n, x.shape[1], x.shape[1], yd.ptr, c, eps, df,
                 scale, C.byref(lam), dh, C.byref(info), terms, mean.ptr, scale2.ptr)
    elif family == "cnn":
        ctx.call("smn_spr_cnn_loo_grad", code, L.ACT[act], layers, w, b, lw, xd.ptr, n, x.shape[1], x.shape[2], x.shape[3], yd.ptr, c,
                 eps, df, scale, C.byref(lam), dh, C.byref(info), terms, mean.ptr, scale2.ptr)
    else:
        from smnngp import nt_kernels
        k = nt_kernels.get_conv_resnet_kernel(layers, 1, act=act, w_std=w, b_std=b, last_w_std=lw)(xd, None, fill="lower")
        ctx.call("smn_loo_multi", code, k.ptr, n, n, yd.ptr, c, eps, df, scale, C.byref(lam), mean.ptr, scale2.ptr, dh, None,
                 C.byref(info), None, 0)
        terms = None
    assert info.value == 0
    return lam.value, np.array(list(dh)), None if terms is None else np.array(list(terms)), mean.raw_numpy(), scale2.raw_numpy()


def check_e2e(L, ctx, family, act, layers, data_key, c, method, dtype):
    f32 = dtype == np.float32
    key = tuple(data_key) + (f32,)
    x, y, hyp, cond = e2e_case(family, act, layers, key)
    assert cond <= 1e4, cond
    ref, grads, terms_ref, fds = e2e_ref(family, act, layers, key, method)
    lam, dh, terms, mean, scale2 = device_e2e(L, ctx, family, act, layers, x, y, hyp, method, dtype)
    cu = cond * U[dtype]
    n = y.shape[0]
    ratios = {"Lambda": abs(lam - ref["lam"]) / ref["lam_abs"] / cu,
              "mean": relerr_norm(mean, ref["mean"]) / cu, "scale2": relerr_norm(scale2, ref["scale2"]) / cu}
    if method == "tp":
        for k in range(2):
            ratios["dhead%d" % k] = abs(dh[k] - ref["dhead"][k]) / ref["dhead_abs"][k] / cu
    if terms is not None:
        for k in range(4):
            ratios["term%d" % k] = abs(terms[k] - terms_ref[0][k]) / terms_ref[1][k] / cu
    worst = max(ratios.values())
    print("RATIO %s %s L=%d %s c=%d %s %s cond %.3g worst %.4g  %s" % (
        family, act, layers, data_key, c, method, np.dtype(dtype).name, cond, worst,
        " ".join("%s=%.3g" % kv for kv in sorted(ratios.items()))))
    assert worst <= 64.0, "needs more than 64 cond u: a finding, not a tolerance"
    assert worst <= 8.0 * MEASURED[dtype]
    if terms is None:
        return
    # the loss gradients against central differences of the rules' own loss; floor: the differences' own error (see
    # test_loo_host.py), on top of the bound just asserted on the terms
    got = {k: -t / n for k, t in zip(("w_std", "b_std", "last_w_std", "eps"), terms)}
    t_abs = dict(zip(("w_std", "b_std", "last_w_std", "eps"), terms_ref[1] / n))
    if method == "tp":
        got.update(LR.head_grads(dh, n, hyp["alpha"], hyp["beta"]))
        hs = LR.head_grads(ref["dhead_abs"], n, hyp["alpha"], hyp["beta"])
        t_abs.update(alpha=2.0 * ref["dhead_abs"][0] / n + ref["dhead_abs"][1] * hyp["beta"] / hyp["alpha"] ** 2 / n,
                     beta=abs(hs["beta"]))
    fd, fd_2h, fd_h2 = fds
    for k, v in got.items():
        floor = 4.0 * abs(fd[k] - fd_2h[k]) + 4.0 * abs(fd[k] - fd_h2[k]) + 1e-12 * abs(fd[k])
        assert abs(v - fd[k]) <= floor + 8.0 * MEASURED[dtype] * cu * t_abs[k], (k, v, fd[k], floor)
        assert abs(v - grads[k]) <= 8.0 * MEASURED[dtype] * cu * t_abs[k], (k, v, grads[k])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("family,act,n", DENSE)
def test_dense_end_to_end(L, ctx, family, act, n, c, method, dtype):
    check_e2e(L, ctx, family, act, 2, ("dense", n, c), c, method, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("h,w,ch,layers", CONV)
def test_cnn_end_to_end(L, ctx, h, w, ch, layers, c, method, dtype):
    check_e2e(L, ctx, "cnn", "relu", layers, ("conv", 12, c, h, w, ch), c, method, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("c", [1, 3])
def test_conv_resnet_value_end_to_end(L, ctx, c, method, dtype):
    check_e2e(L, ctx, "conv_resnet", "relu", 1, ("conv", 12, c, 8, 8, 1), c, method, dtype)


# ----------------------------------------------------------------------------- 3. the rectangle route (n_pad >= 8192)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rectangle_route(L, ctx, dtype):
    """n = 8190, MLP, C = 3.  No N^3 work on the host: the device's own -K~^-1 and A (smn_spr_kinv: the rectangle route) are
    downloaded and the rules are fed those -- Lambda, mean, scale2 and dhead in O(N^2), G on 256 random rows (a 256 x N x N
    product).  The fused entry goes through the same launches, so its Lambda, mean and scale2 are the head's bits."""
    rng = np.random.default_rng(8190)
    n, c, d, eps = 8190, 3, 7, 1e-1
    x, y = rng.standard_normal((n, d)).astype(dtype), rng.standard_normal((n, c)).astype(dtype)
    xd, yd = ctx.to_device(x), ctx.to_device(y)
    code = L.dtype_code(dtype)
    ld = n + (-n) % (16 // np.dtype(dtype).itemsize)
    nk_d, a_d = ctx.empty((n, ld), dtype), ctx.empty((n, c), dtype)
    info = C.c_int()
    net = (L.NET_MLP, L.ACT["relu"], 2, 1.3, 0.4, 0.9)
    ctx.call("smn_spr_kinv", code, *net, xd.ptr, n, d, d, yd.ptr, c, eps, nk_d.ptr, ld, a_d.ptr, None, C.byref(info))
    assert info.value == 0
    nk = np.tril(nk_d.raw_numpy()[:, :n].astype(np.float64))
    nk = nk + np.tril(nk, -1).T
    a, y64 = a_d.raw_numpy().astype(np.float64), y.astype(np.float64)
    rows = np.sort(rng.choice(n, size=256, replace=False))
    df, scale = head_params("tp")
    ref = LR.parts(-nk, a, y64, "tp", rows=rows, **HEAD)
    mean, scale2, g = ctx.empty((n, c), dtype), ctx.empty((n,), dtype), ctx.empty((n, n), dtype)
    lam, dh = C.c_double(), (C.c_double * 2)()
    ctx.call("smn_loo_head", code, nk_d.ptr, ld, a_d.ptr, yd.ptr, n, c, df, scale, C.byref(lam), mean.ptr, scale2.ptr, dh, g.ptr, n)
    got = (lam.value, mean.raw_numpy(), scale2.raw_numpy(), np.array(list(dh)), g.raw_numpy())
    check_head(got, ref, nk, a, y64, dtype, rows=rows)
    lam2, dh2, info2, terms = C.c_double(), (C.c_double * 2)(), C.c_int(), (C.c_double * 4)()
    mean2, scale22 = ctx.empty((n, c), dtype), ctx.empty((n,), dtype)
    ctx.call("smn_spr_loo_grad", code, *net, xd.ptr, n, d, d, yd.ptr, c, eps, df, scale, C.byref(lam2), dh2, C.byref(info2), terms,
             mean2.ptr, scale22.ptr)
    assert info2.value == 0 and lam2.value == lam.value and list(dh2) == list(dh)
    assert np.array_equal(mean2.raw_numpy(), got[1]) and np.array_equal(scale22.raw_numpy(), got[2])
    # tr G = d Lambda / d eps from the seed the head returned (fp64 sum of n entries of the storage type)
    tr = float(np.sum(np.diag(got[4]).astype(np.float64)))
    print("terms", list(terms), "tr G", tr)
    assert all(np.isfinite(t) for t in terms) and abs(terms[3] - tr) <= 1e-12 * np.sum(np.abs(np.diag(got[4])))


# ------------------------------------------------------------------------------------------------------ 4. model level
def make_model(family, x, y, layers, act, method, dtype, hyp, single=False):
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood
    from smnngp.spax.models import SPR, MultiSPR
    factory = {"mlp": lambda w, b, l: nt_kernels.get_mlp_kernel(layers, act=act, w_std=w, b_std=b, last_w_std=l),
               "cnn": lambda w, b, l: nt_kernels.get_cnn_kernel(layers, 1, act=act, w_std=w, b_std=b, last_w_std=l),
               "conv_resnet": lambda w, b, l: nt_kernels.get_conv_resnet_kernel(layers, 1, act=act, w_std=w, b_std=b,
                                                                               last_w_std=l)}[family]
    kernel = NNGPKernel(factory, hyp["w_std"], hyp["b_std"], hyp["last_w_std"])
    lik = GaussianLikelihood() if method == "gp" else StudentTLikelihood(hyp["alpha"], hyp["beta"])
    if single:
        model = SPR(kernel, lik, np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype).reshape(-1), 0.0, 1.0, eps=hyp["eps"])
    else:
        model = MultiSPR(kernel, lik, np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype), eps=hyp["eps"])
    vmap = {"w_std": kernel.w_std, "b_std": kernel.b_std, "last_w_std": kernel.last_w_std, "eps": model.eps}
    if method == "tp":
        vmap.update(alpha=lik.a, beta=lik.b)
    return model, vmap


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("family,act,layers,data_key", [("mlp", "relu", 2, ("dense", 129, 1)), ("cnn", "relu", 2, ("conv", 12, 1, 8, 8, 1))])
def test_one_column_multispr_is_spr_bit_for_bit(family, act, layers, data_key, method, dtype):
    x, y, hyp, _ = e2e_case(family, act, layers, tuple(data_key) + (dtype == np.float32,))
    single, _ = make_model(family, x, y, layers, act, method, dtype, hyp, single=True)
    multi, _ = make_model(family, x, y, layers, act, method, dtype, hyp)
    assert single.loo_loss() == multi.loo_loss()
    (l1, g1), (l2, g2) = single.loo_loss_and_grad(), multi.loo_loss_and_grad()
    assert l1 == l2 and [g1[k.replace("(MultiSPR)", "(SPR)")] for k in g2] == list(g2.values())
    (m1, s1, d1), (m2, s2, d2) = single.loo_predict(), multi.loo_predict()
    assert m1.shape == (y.shape[0],) and m2.shape == (y.shape[0], 1)
    assert np.array_equal(m1, m2[:, 0]) and np.array_equal(s1, s2) and d1 == d2
    assert d1 == (None if method == "gp" else 2.0 * hyp["alpha"] + (y.shape[0] - 1))


def test_loo_accuracy_and_predictions_on_a_three_class_set():
    key = ("dense", 129, 3, False)
    x, y, hyp, cond = e2e_case("mlp", "relu", 2, key)
    labels = M.dense_data(129, 3)[2]
    ref = e2e_ref("mlp", "relu", 2, key, "tp")[0]
    model, _ = make_model("mlp", x, y, 2, "relu", "tp", np.float64, hyp)
    mean, scale2, df = model.loo_predict()
    assert relerr_norm(mean, ref["mean"]) <= 64 * cond * U[np.float64] and df == ref["df"]
    assert relerr_norm(scale2, ref["scale2"]) <= 64 * cond * U[np.float64]
    top = np.sort(ref["mean"], axis=1)
    assert np.min(top[:, -1] - top[:, -2]) > 1e-6        # no near tie: the arg-max is the rules' arg-max
    want = np.argmax(ref["mean"], axis=1)
    assert np.array_equal(model.loo_classify(), want)
    assert model.loo_accuracy(labels) == float(np.mean(want == labels))
    assert model.loo_accuracy() == float(np.mean(want == np.argmax(y, axis=1)))
    assert abs(model.loo_loss() + ref["lam"] / 129) <= 64 * cond * U[np.float64] * ref["lam_abs"] / 129


@pytest.mark.parametrize("family,act,layers,data_key", [("mlp", "relu", 2, ("dense", 129, 3)), ("cnn", "relu", 2, ("conv", 12, 3, 8, 8, 1))])
def test_first_adam_step_of_the_loo_objective(family, act, layers, data_key):
    from smnngp import train
    key = tuple(data_key) + (False,)
    x, y, hyp, _ = e2e_case(family, act, layers, key)
    _, rg, _, _ = e2e_ref(family, act, layers, key, "tp")
    model, vmap = make_model(family, x, y, layers, act, "tp", np.float64, hyp)
    names = {id(v): k for k, v in model.vars().items()}
    before = {k: float(v.value) for k, v in model.vars().items()}
    lml_before = model.loss_and_grad()
    value = train.build_train_step(model, objective="loo")(1e-2)
    ref_loss = LR.loss(family, x, y, layers, act, "tp", **hyp)
    assert abs(value - ref_loss) <= 1e-9 * max(1.0, abs(ref_loss))
    for k in LR.KEYS:
        var = vmap[k]
        raw_g = rg[k] * float(var.constraint.grad(before[names[id(var)]]))
        m, v = 0.1 * raw_g, 0.001 * raw_g * raw_g                     # Adam's first step, bias-corrected
        want = -1e-2 * np.sqrt(1 - 0.999) / (1 - 0.9) * m / (np.sqrt(v) + 1e-8)
        got = float(var.value) - before[names[id(var)]]
        print("%s update %.12g rules %.12g" % (k, got, want))
        assert got != 0.0 and abs(got - want) <= 2e-6 * abs(want)
    # the default objective is untouched by any loo_* call: same bits before and after
    for k, v in model.vars().items():
        v.assign(before[k])
    model.loo_loss(); model.loo_predict(); model.loo_loss_and_grad()
    lml_after = model.loss_and_grad()
    assert lml_before[0] == lml_after[0] and lml_before[1] == lml_after[1]
    step = train.build_train_step(model)                              # objective="lml": loss_and_grad, call for call
    calls, orig = [], model.x_data.ctx.call

    def counting(name, *args):
        calls.append(name)
        return orig(name, *args)

    model.x_data.ctx.call = counting
    try:
        step(1e-2)
    finally:
        del model.x_data.ctx.call
    assert calls == ["smn_spr_loss_grad_multi" if family == "mlp" else "smn_spr_cnn_loss_grad_multi"]


@pytest.mark.parametrize("single", [False, True])
def test_not_positive_definite_is_nan_everywhere(single):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((12, 7))
    x = np.concatenate([x, x, x], axis=0)                             # equal rows: K is singular
    y = rng.standard_normal((36, 1 if single else 3))
    hyp = dict(BASE, eps=1e-300)
    model, _ = make_model("mlp", x, y, 2, "relu", "tp", np.float32, hyp, single=single)
    assert model.eps.safe_value < 1e-290
    loss, grads = model.loo_loss_and_grad()
    assert np.isnan(loss) and set(grads) == set(model.vars()) and all(np.isnan(g) for g in grads.values())
    assert np.isnan(model.loo_loss())
    mean, scale2, _ = model.loo_predict()
    assert np.isnan(mean).all() and np.isnan(scale2).all()


def test_images_above_the_limit_raise_and_auto_falls_back():
    from smnngp import train
    rng = np.random.default_rng(9)
    x, y = rng.standard_normal((6, 40, 40, 1)), rng.standard_normal((6, 3))
    model, _ = make_model("cnn", x, y, 2, "relu", "gp", np.float64, dict(BASE, eps=5e-2))
    with pytest.raises(NotImplementedError):
        model.loo_loss_and_grad()
    with pytest.raises(NotImplementedError):
        train.build_train_step(model, method="analytic", objective="loo")(1e-2)
    before = {k: float(v.value) for k, v in model.vars().items()}
    value = train.build_train_step(model, method="auto", objective="loo")(1e-2)
    assert np.isfinite(value)
    assert any(float(v.value) != before[k] for k, v in model.vars().items())
    resnet, _ = make_model("conv_resnet", M.conv_data(12, 3, 8, 8, 1)[0], M.conv_data(12, 3, 8, 8, 1)[1], 1, "relu", "gp",
                           np.float64, dict(BASE, eps=5e-2))
    with pytest.raises(NotImplementedError):
        resnet.loo_loss_and_grad()
    assert np.isfinite(resnet.loo_loss())
