"""Regression on the pivoted-Cholesky factor on the device (csrc/lowrank.hip, smnngp/lowrank.py, spax.models.LowRankSPR).

1. smn_lowrank_gram through the C ABI on random L, in windows with guards (tests/_windows.py): every entry of G, B and s within
       |err_ab| <= (k + 3) u sum_i |w_i l_ia l_ib| + (splits + 1) u64 sum_i |w_i l_ia l_ib|
   of an extended-precision reference -- k - 1 additions, the product, the weight's product and the weight's rounding, each
   within one unit roundoff of the accumulating precision, then one fp64 addition per split and the final rounding; k = the
   split length and u = 2^-24 in f32, k = n and u = 2^-53 in f64 (B and s take l_ib -> y_ik and l_ia l_ib -> y_ik^2).  Derived,
   not measured.  G symmetric to the bit, two calls and both layouts the same bits, output guards untouched, NaN input guards.
2. smn_lowrank_fit / smn_lowrank_readout on the device's OWN factor and pivots (pivot ties cannot matter) against the dense
   form of tests/_lowrank_rules.py, for mlp / resnet / cnn / pool kernels x relu / erf x both corrections x the gp / tp heads at
   N in {65, 300}, M in {1, 17, 40}, eps in {1e-1, 1e-2}:
       f64   1e-8 relative (norm-wise: the largest error over the largest reference entry), quantity by quantity;
       f32   16 x the rules' float32-split run against their fp64 run (the largest over four summation orders), quantity by
             quantity: the project's margin for a same-precision yardstick.
   Each case prints "lowrank-multiple" lines: the error as a multiple of the bound (f64) or of the yardstick (f32).
3. a matrix I + G that does not factor, chunked predictions, rank = N against SPR, the rank limit, the model on top."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _cnn_pool_rules as PR  # noqa: E402
import _lowrank_rules as LR  # noqa: E402
import _windows as W  # noqa: E402
from oracle import nngp_oracle as O  # noqa: E402

HP = dict(w_std=1.3, b_std=0.2, last_w_std=0.9)
DTYPES = [np.float64, np.float32]
T_TEST = 11
_PD = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


# ------------------------------------------------------------------------------------------------ 1. the Gram entry
def gram_shapes(split):
    return [(1, 1, 1), (65, 33, 1), (257, 96, 3), (split + 1, 17, 2), (3 * split + 5, 130, 1)]


def gram_call(ctx, L, Lh, w, Y, layout):
    n, m = Lh.shape
    c = Y.shape[1]
    Lw, Yw = W.in_window(ctx, Lh, layout), W.in_window(ctx, Y, layout)
    ww = None if w is None else W.in_window(ctx, np.asarray(w, dtype=np.float64), layout)
    Gw = W.out_window(ctx, m, m, np.float64, layout)
    Bw, sw = W.out_window(ctx, m, c, np.float64, "block", seed=1), W.out_window(ctx, 1, c, np.float64, "block", seed=2)
    ctx.call("smn_lowrank_gram", L.dtype_code(Lh.dtype), Lw.ptr, n, m, Lw.ld, None if ww is None else ww.ptr, Yw.ptr, c, Yw.ld,
             Gw.ptr, Gw.ld, Bw.ptr, sw.ptr)
    return Gw.result("G"), Bw.result("B"), sw.result("s")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
@pytest.mark.parametrize("case", range(5))
def test_gram_componentwise(ctx, L, case, weighted, dtype):
    split = L.LOWRANK_SPLIT
    n, m, c = gram_shapes(split)[case]
    rng = np.random.default_rng(100 + case)
    Lh = rng.standard_normal((n, m)).astype(dtype)
    Y = rng.standard_normal((n, c)).astype(dtype)
    w = 10.0 ** rng.uniform(-3.0, 3.0, n) if weighted else None
    G, B, s = gram_call(ctx, L, Lh, w, Y, "aligned")
    G2, B2, s2 = gram_call(ctx, L, Lh, w, Y, "aligned")
    G3, B3, s3 = gram_call(ctx, L, Lh, w, Y, "unaligned")
    for a, b, d in ((G, G2, G3), (B, B2, B3), (s, s2, s3)):
        assert np.array_equal(a, b), "two calls differ"
        assert np.array_equal(a, d), "the bits depend on the layout"
    assert np.array_equal(G, G.T)
    ld = np.longdouble
    wl = np.ones(n, dtype=ld) if w is None else w.astype(ld)
    Ll, Yl = Lh.astype(ld), Y.astype(ld)
    splits = (n + split - 1) // split
    k, u = (split, 2.0 ** -24) if np.dtype(dtype) == np.float32 else (n, 2.0 ** -53)
    what = "gram-n%d-m%d-c%d-%s-%s" % (n, m, c, "w" if weighted else "1", np.dtype(dtype).name)
    for name, got, ref, mag in (("G", G, (Ll * wl[:, None]).T @ Ll, (np.abs(Ll) * wl[:, None]).T @ np.abs(Ll)),
                                ("B", B, (Ll * wl[:, None]).T @ Yl, (np.abs(Ll) * wl[:, None]).T @ np.abs(Yl)),
                                ("s", s.reshape(-1), (wl[:, None] * Yl * Yl).sum(axis=0), (wl[:, None] * Yl * Yl).sum(axis=0))):
        bound = ((k + 3) * u + (splits + 1) * 2.0 ** -53) * mag.astype(np.float64)
        err = np.abs(got.astype(ld) - ref).astype(np.float64)
        print("lowrank-multiple %s %s %.3g" % (what, name, float((err / bound).max())))
        assert np.all(err <= bound), (what, name, float((err / bound).max()))


# ------------------------------------------------------------------------------------------------ 2. fit and read-out
def data(n, d, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)) * np.exp(0.5 * rng.standard_normal((n, 1)))


def images(n, seed=1):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, 4, 4, 1)) * np.exp(0.5 * rng.standard_normal((n, 1, 1, 1)))


def kernel_fn(kind, act, hp=HP):
    from smnngp import nt_kernels as nt
    make = {"mlp": nt.get_mlp_kernel, "resnet": nt.get_dense_resnet_kernel, "cnn": nt.get_cnn_kernel, "pool": nt.get_cnn_pool_kernel}
    return make[kind](2, act=act, **hp)


_ORACLE = {}


def problem(kind, act, n, dtype):
    """(x [n + T_TEST, ...] as `dtype` holds it, the fp64 reference kernel of all of it, targets [n, 2]); shared, never modified."""
    key = (kind, act, n, np.dtype(dtype).name)
    if key not in _ORACLE:
        xa = (images(n + T_TEST) if kind in ("cnn", "pool") else data(n + T_TEST, 5)).astype(dtype).astype(np.float64)
        f = {"mlp": O.mlp_kernel, "resnet": O.dense_resnet_kernel, "cnn": O.cnn_kernel, "pool": PR.pool_kernel}[kind]
        K = np.asarray(f(xa, None, num_hiddens=2, act=act, **HP), dtype=np.float64)
        rng = np.random.default_rng(7)
        flat = xa[:n].reshape(n, -1)
        y = np.stack([np.sin(flat[:, 0]) + 0.1 * rng.standard_normal(n), rng.standard_normal(n)], axis=1)
        for a in (xa, K, y):
            a.setflags(write=False)
        _ORACLE[key] = (xa, K, y)
    return _ORACLE[key]


QUANT = {"quad": lambda r: r.quad, "logdet": lambda r: r.logdet, "mean": lambda r: r.mean, "var": lambda r: r.var}


def heads(n):
    """The gp and tp log-marginal likelihoods of the first target column, as functions of a result (df = 4, scale = 1.7)."""
    return {"gp": lambda r: LR.gp_logpdf(r.quad[0], r.logdet, n), "tp": lambda r: LR.tp_logpdf(r.quad[0], r.logdet, n, 4.0, 1.7)}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("act", ["relu", "erf"])
@pytest.mark.parametrize("kind", ["mlp", "resnet", "cnn", "pool"])
@pytest.mark.parametrize("n", [65, 300])
def test_fit_and_readout_against_the_dense_form(ctx, L, n, kind, act, dtype):
    from types import SimpleNamespace
    from smnngp import lowrank
    xa, K, y = problem(kind, act, n, dtype)
    fn = kernel_fn(kind, act)
    f32 = np.dtype(dtype) == np.float32
    quant = dict(QUANT, **heads(n))
    for m in (1, 17, 40):
        res = lowrank.pivoted_cholesky(fn, xa[:n].astype(dtype), m)
        assert res.rank == m, "the kernel ran out of rank"
        Lh = res.factor.raw_numpy().astype(np.float64)
        P = res.pivots
        R = Lh[P]
        assert np.all(np.triu(R, 1) == 0.0) and np.all(np.diag(R) > 0.0)
        kzt = K[P][:, n:].astype(dtype).astype(np.float64)
        ktt = np.diag(K)[n:].astype(dtype).astype(np.float64)
        ys = y.astype(dtype).astype(np.float64)
        for fitc in (True, False):
            for eps in (1e-1, 1e-2):
                what = "%s-%s-n%d-m%d-%s-eps%g-%s" % (kind, act, n, m, "fitc" if fitc else "none", eps, np.dtype(dtype).name)
                fit = lowrank.woodbury_fit(res, ys, eps, fitc)
                assert fit.info == 0, what
                mean, var = fit.readout(kzt.astype(dtype), ktt.astype(dtype))
                got = SimpleNamespace(quad=fit.quad, logdet=fit.logdet, mean=mean.raw_numpy().astype(np.float64),
                                      var=var.raw_numpy().astype(np.float64))
                ref = LR.dense(Lh, res.resid, eps, fitc, ys, R, kzt, ktt)
                yard = LR.yardstick(Lh, res.resid, eps, fitc, ys, R, kzt, ktt, L.LOWRANK_SPLIT, quant) if f32 else None
                for name, f in quant.items():
                    r = np.asarray(f(ref), dtype=np.float64)
                    err = float(np.abs(np.asarray(f(got), dtype=np.float64) - r).max())
                    unit = yard[name] if f32 else 1e-8 * float(np.abs(r).max())
                    print("lowrank-multiple %s %s %.3g" % (what, name, err / unit if unit > 0.0 else (0.0 if err == 0.0 else np.inf)))
                    assert err <= (16.0 * unit if f32 else unit), (what, name, err, unit)
                assert np.all(got.var > 0.0), what


# ------------------------------------------------------------------------------------------------ 3. further cases
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_a_matrix_that_does_not_factor_gives_nan_and_info(ctx, L, dtype):
    """I + L^T W L with a NaN in it has no Cholesky factor: SMN_OK, info = the failing pivot, NaN everywhere."""
    n, m, c = 65, 17, 2
    rng = np.random.default_rng(0)
    Lh = rng.standard_normal((n, m)).astype(dtype)
    Lh[5, 3] = np.nan
    Ld, yd = ctx.to_device(Lh), ctx.to_device(rng.standard_normal((n, c)).astype(dtype))
    Cf, beta = ctx.to_device(np.zeros((m, m))), ctx.to_device(np.zeros((m, c)))
    quad, logdet, info = np.zeros(c), C.c_double(0.0), C.c_int(0)
    ctx.call("smn_lowrank_fit", L.dtype_code(dtype), Ld.ptr, n, m, m, None, 1e-2, 0, yd.ptr, c, c, Cf.ptr, beta.ptr,
             quad.ctypes.data_as(_PD), C.byref(logdet), C.byref(info))
    assert 1 <= info.value <= m
    assert np.all(np.isnan(quad)) and np.isnan(logdet.value)
    assert np.all(np.isnan(Cf.raw_numpy())) and np.all(np.isnan(beta.raw_numpy()))


def test_rank_above_the_limit_is_not_supported(ctx, L):
    m = L.LOWRANK_MAX_RANK + 1
    buf = ctx.to_device(np.zeros(16))
    quad, logdet, info = np.zeros(1), C.c_double(0.0), C.c_int(0)
    calls = [("smn_lowrank_gram", (L.F64, buf.ptr, 1, m, m, None, None, 0, 1, buf.ptr, m, None, None)),
             ("smn_lowrank_fit", (L.F64, buf.ptr, 1, m, m, None, 1e-2, 0, buf.ptr, 1, 1, buf.ptr, buf.ptr, quad.ctypes.data_as(_PD),
                                  C.byref(logdet), C.byref(info))),
             ("smn_lowrank_readout", (L.F64, buf.ptr, 1, buf.ptr, 1, m, buf.ptr, m, buf.ptr, buf.ptr, 1, buf.ptr, buf.ptr))]
    for name, args in calls:
        with pytest.raises(L.SmnError) as e:
            ctx.call(name, *args)
        assert e.value.code == L.ENOTSUP and "4096" in str(e.value), name


def _model(kind, act, lik, x, y, dtype, **kw):
    from smnngp import nt_kernels as nt
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.models import LowRankSPR
    make = {"mlp": nt.get_mlp_kernel, "cnn": nt.get_cnn_kernel}[kind]
    kernel = NNGPKernel(lambda w, b, l: make(2, act=act, w_std=w, b_std=b, last_w_std=l), HP["w_std"], HP["b_std"], HP["last_w_std"])
    return LowRankSPR(kernel, lik, np.asarray(x, dtype=dtype), y, 0.3, 1.7, **kw)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_chunked_predictions_carry_the_bits_of_single_rows(ctx, L, dtype):
    from smnngp import lowrank
    from smnngp.spax.likelihoods import GaussianLikelihood
    n = 65
    xa, K, y = problem("mlp", "relu", n, dtype)
    res = lowrank.pivoted_cholesky(kernel_fn("mlp", "relu"), xa[:n].astype(dtype), 17)
    fit = lowrank.woodbury_fit(res, y, 1e-2, True)
    kzt, ktt = K[res.pivots][:, n:].astype(dtype), np.diag(K)[n:].astype(dtype)
    mean, var = (a.raw_numpy() for a in fit.readout(kzt, ktt))
    for j in range(T_TEST):
        m1, v1 = (a.raw_numpy() for a in fit.readout(np.ascontiguousarray(kzt[:, j:j + 1]), ktt[j:j + 1]))
        assert np.array_equal(m1[0], mean[j]) and v1[0] == var[j], j
    model = _model("mlp", "relu", GaussianLikelihood(), xa[:n], y[:, 0], dtype, rank=17, eps=1e-2)
    whole = model.predict(xa[n:])
    for chunk in (1, 4):
        part = model.predict(xa[n:], chunk=chunk)
        assert np.array_equal(whole[0], part[0]) and np.array_equal(whole[1], part[1]), chunk
    assert whole[0].shape == (T_TEST, 1) and whole[1].shape == (T_TEST,) and whole[0].dtype == np.dtype(dtype)


@pytest.mark.parametrize("method", ["gp", "tp"])
def test_full_rank_reproduces_the_exact_model(ctx, L, method):
    """rank = N = 65 in f64: L L^T is K itself and both corrections coincide, so loss, mean and the diagonal covariance are
    SPR's, to 1e-8 relative; so is the Gaussian test_nll (the Student-t one differs by design: LowRankSPR's docstring)."""
    from smnngp import nt_kernels as nt
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood
    from smnngp.spax.models import SPR
    n = 65
    xa, _, y = problem("mlp", "relu", n, np.float64)
    lik = (lambda: GaussianLikelihood()) if method == "gp" else (lambda: StudentTLikelihood(2.0, 3.4))
    kernel = NNGPKernel(lambda w, b, l: nt.get_mlp_kernel(2, act="relu", w_std=w, b_std=b, last_w_std=l), HP["w_std"], HP["b_std"],
                        HP["last_w_std"])
    exact = SPR(kernel, lik(), xa[:n], y[:, 0], 0.3, 1.7, eps=1e-3)
    loss = exact.loss()
    mean, cov = exact.predict(xa[n:])
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(cov.diagonal(), dtype=np.float64)
    yt = np.cos(xa[n:, 0])
    for correction in ("fitc", "none"):
        model = _model("mlp", "relu", lik(), xa[:n], y[:, 0], np.float64, rank=n, correction=correction, eps=1e-3)
        assert model._factor()[1].rank == n
        got = model.loss()
        print("lowrank-multiple fullrank-%s-%s loss %.3g" % (method, correction, abs(got - loss) / (1e-8 * abs(loss))))
        assert abs(got - loss) <= 1e-8 * abs(loss)
        m, v = model.predict(xa[n:])
        for name, a, b in (("mean", m, mean), ("var", v, var)):
            e = float(np.abs(a - b).max() / np.abs(b).max())
            print("lowrank-multiple fullrank-%s-%s %s %.3g" % (method, correction, name, e / 1e-8))
            assert e <= 1e-8, (name, e)
        if method == "gp":
            a, b = model.test_nll(xa[n:], yt), exact.test_nll(xa[n:], yt)
            assert abs(a - b) <= 1e-8 * abs(b)
        else:
            assert np.isfinite(model.test_nll(xa[n:], yt))


@pytest.mark.parametrize("kind,dtype", [("mlp", np.float64), ("cnn", np.float64), ("mlp", np.float32)], ids=["mlp-f64", "cnn-f64", "mlp-f32"])
def test_model_on_its_own_factor(ctx, L, kind, dtype):
    """LowRankSPR end to end (fused and matrix route): loss() and test_nll() against the rules' dense form on the model's own
    factor, for both heads; the factor is kept while the hyper-parameters stand and remade when they move; a train step by
    central differences lowers nothing it should not.  f64: 1e-8 relative (the test inputs' kernel comes from the device here,
    the reference's from the reference kernels: their difference is rounding-level in fp64); f32: finite values only, the
    numbers are section 2's."""
    from smnngp import train
    from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood
    n, m, eps = 65, 17, 1e-2
    xa, K, y = problem(kind, "relu", n, dtype)
    yt = np.cos(xa[n:].reshape(T_TEST, -1)[:, 0])
    for lik, correction in ((GaussianLikelihood(), "fitc"), (StudentTLikelihood(2.0, 3.4), "none")):
        model = _model(kind, "relu", lik, xa[:n], y[:, 0], dtype, rank=m, correction=correction, eps=eps)
        loss, nll = model.loss(), model.test_nll(xa[n:], yt)
        res = model._factor()[1]
        assert model._factor()[1] is res and res.rank == m
        if np.dtype(dtype) == np.float32:
            assert np.isfinite(loss) and np.isfinite(nll)
        else:
            Lh, P = res.factor.raw_numpy().astype(np.float64), res.pivots
            fitc = correction == "fitc"
            df, scale = lik.lml_params()
            a = LR.dense(Lh, res.resid, eps, fitc, y[:, 0])
            lp = LR.tp_logpdf(a.quad[0], a.logdet, n, df, scale) if df > 0 else LR.gp_logpdf(a.quad[0], a.logdet, n)
            assert abs(loss + lp / n) <= 1e-8 * abs(lp / n), (kind, correction)
            lam = eps * res.trace[0] / n
            b = LR.dense(Lh, res.resid, lam, fitc, y[:, 0], Lh[P], K[P][:, n:], np.diag(K)[n:])
            mu, v, ys = b.mean[:, 0] * 1.7 + 0.3, b.var * 1.7 ** 2, yt * 1.7 + 0.3
            if df > 0:
                sig = np.sqrt((df + b.quad[0] / scale) / (df + n) * scale * v)
                ref = -np.mean(O.student_t_logpdf(ys, df + n, mu, sig))
            else:
                ref = -np.mean(O.normal_logpdf(ys, mu, np.sqrt(v)))
            assert abs(nll - ref) <= 1e-8 * abs(ref), (kind, correction, nll, ref)
        step = train.build_train_step(model, method="auto")
        before = step(1e-2)
        assert before == pytest.approx(loss, rel=1e-12) and model._factor()[1] is not res
        assert np.isfinite(model.loss())
