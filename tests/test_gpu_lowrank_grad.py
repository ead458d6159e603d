"""Frozen inducing points and the analytic gradient of the low-rank model on the device (csrc/pchol.hip: smn_pchol_mlp_at;
csrc/lowrank_grad.hip: smn_lowrank_grad; smnngp/lowrank.py; spax.models.LowRankSPR).

1. A factor built at the pivots the greedy call returned carries the greedy call's bits: factor, resid and trace, fused and matrix
   route, f32 and f64, contiguous and in windows with ldl > m and a misaligned base (tests/_windows.py).  A duplicated input row
   listed as a later pivot ends the factor there.
2. smn_lowrank_grad through the C ABI, in windows with ldl > m and ldx > d, on the device's OWN factor, residual and pivots,
   against the closed form of tests/_lowrank_grad_rules.py (itself held to central differences of the dense model on the CPU):
       f64   every term within 1e-8 S, S = that term's sum of absolute contracted products (the level test_gpu_lowrank_gp holds
             its f64 results to);
       f32   every term within 16 x the same-precision yardstick: the rules' float32 run (L, U, K0 and the tangents as float32
             holds them, the m x m side in fp64) against their fp64 run on the same stored inputs, the largest over the four
             summation orders of tests/_lowrank_rules.py, floored at u32 S.  16 x is the project's standing allowance.
   Each case prints "lowrank-grad-multiple" lines: the error as a multiple of its bound (f64) or of the yardstick (f32).
3. Two calls give the same four doubles; the aligned and the misaligned window give the same bits.
4. The model: freeze_pivots() changes no bit of loss() and predict(); loss_and_grad()[0] is loss(); the gradient against central
   differences of the frozen loss(); rank = N against SPR.loss_and_grad; a training step; refresh_pivots().
5. SMN_NET_NTK and the conv kernels are refused before any launch."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _lowrank_grad_rules as G  # noqa: E402
import _pchol_rules as PR  # noqa: E402
import _windows as W  # noqa: E402

HP = dict(w_std=1.3, b_std=0.2, last_w_std=0.9)
_PD, _PI64 = C.POINTER(C.c_double), C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


def data(n, d, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)) * np.exp(0.5 * rng.standard_normal((n, 1)))


def kernel_fn(net, act, layers, hp=HP):
    from smnngp import nt_kernels as nt
    return {"mlp": nt.get_mlp_kernel, "resnet": nt.get_dense_resnet_kernel}[net](layers, act=act, **hp)


# ------------------------------------------------------------------------------------------------ 1. prescribed pivots
def fused_at(ctx, L, fn, x, pivots, layout):
    """smn_pchol_mlp_at with x, the factor and nothing else in windows: (factor [n, m], resid, trace, rank)."""
    n, d = x.shape
    m = len(pivots)
    xw = W.in_window(ctx, x, layout)
    fw = W.out_window(ctx, n, m, x.dtype, layout)
    resid = ctx.to_device(np.zeros(n))
    piv = np.ascontiguousarray(pivots, dtype=np.int64)
    trace, rank = np.zeros(m + 1), C.c_int64(0)
    ctx.call("smn_pchol_mlp_at", L.dtype_code(x.dtype), fn.net, fn.act, fn.num_hiddens, fn.w_std, fn.b_std, fn.last_w_std, xw.ptr, n,
             xw.ld, d, piv.ctypes.data_as(_PI64), m, 0.0, fw.ptr, fw.ld, resid.ptr, trace.ctypes.data_as(_PD), C.byref(rank))
    return fw.result("factor"), resid.raw_numpy(), trace, int(rank.value)


def matrix_at(ctx, L, fn, x, pivots, layout):
    """The matrix route's loop (smn_pchol_begin / smn_pchol_step) at prescribed pivots with the factor in a window."""
    from smnngp import lowrank
    n, m = x.shape[0], len(pivots)
    xd = ctx.to_device(x)
    diag = lowrank.kernel_diag(fn, xd)
    init = np.zeros((n, m), dtype=x.dtype)
    fw = W.Window(n, m, x.dtype, layout, "out", data=init).upload(ctx)
    resid = ctx.to_device(np.zeros(n))
    piv, rmax, tr = C.c_int64(0), C.c_double(0.0), C.c_double(0.0)
    ctx.call("smn_pchol_begin", L.dtype_code(x.dtype), n, diag.ptr, resid.ptr, C.byref(piv), C.byref(rmax), C.byref(tr))
    trace = [tr.value]
    for j, p in enumerate(pivots):
        k = fn(lowrank._row_view(xd, int(p)), xd, get="nngp")
        ctx.call("smn_pchol_step", L.dtype_code(x.dtype), n, j, int(p), k.ptr, fw.ptr, fw.ld, resid.ptr, C.byref(piv), C.byref(rmax),
                 C.byref(tr))
        trace.append(tr.value)
    return fw.result("factor"), resid.raw_numpy(), np.asarray(trace), m


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("route", ["fused", "matrix"])
@pytest.mark.parametrize("n", [65, 300])
def test_factor_at_the_greedy_pivots_carries_the_greedy_bits(ctx, L, n, route, dtype):
    from smnngp import lowrank
    x = data(n, 5, seed=n).astype(dtype)
    fn = kernel_fn("mlp", "relu", 2)
    for m in (1, 17, 48):
        greedy = lowrank.pivoted_cholesky(fn, x, m, route=route)
        assert greedy.rank == m
        want = greedy.factor.raw_numpy()
        again = lowrank.pivoted_cholesky(fn, x, pivots=greedy.pivots, route=route)
        assert again.rank == m and np.array_equal(again.pivots, greedy.pivots)
        assert np.array_equal(again.factor.raw_numpy(), want), (route, m, "factor")
        assert np.array_equal(again.resid, greedy.resid) and np.array_equal(again.trace, greedy.trace), (route, m)
        assert lowrank.pivoted_cholesky(fn, x, m, pivots=greedy.pivots, route=route).rank == m      # max_rank = len(pivots)
        for layout in ("aligned", "unaligned"):
            f, r, t, rank = (fused_at if route == "fused" else matrix_at)(ctx, L, fn, x, greedy.pivots, layout)
            assert rank == m
            assert np.array_equal(f, want), (route, m, layout, "factor")
            assert np.array_equal(r, greedy.resid), (route, m, layout, "resid")
            assert np.array_equal(t, greedy.trace), (route, m, layout, "trace")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("route", ["fused", "matrix"])
def test_a_duplicated_row_listed_as_a_later_pivot_ends_the_factor(ctx, L, route, dtype):
    from smnngp import lowrank
    x = data(65, 5, seed=3).astype(dtype)
    x[9] = x[5]
    fn = kernel_fn("mlp", "erf", 2)
    res = lowrank.pivoted_cholesky(fn, x, pivots=[5, 2, 9, 7], route=route)
    assert res.rank == 2 and res.pivots.tolist() == [5, 2]
    assert tuple(res.factor.shape) == (65, 2) and res.trace.shape == (3,)
    full = lowrank.pivoted_cholesky(fn, x, pivots=[5, 2], route=route)
    assert np.array_equal(full.factor.raw_numpy(), res.factor.raw_numpy()) and np.array_equal(full.resid, res.resid)
    with pytest.raises(L.SmnError) as e:                                    # the C entry checks the range itself
        bad = np.asarray([5, 65], dtype=np.int64)
        xd, f, r = ctx.to_device(x), ctx.to_device(np.zeros((65, 2), dtype=dtype)), ctx.to_device(np.zeros(65))
        t, k = np.zeros(3), C.c_int64(0)
        ctx.call("smn_pchol_mlp_at", L.dtype_code(dtype), fn.net, fn.act, 2, 1.3, 0.2, 0.9, xd.ptr, 65, 5, 5, bad.ctypes.data_as(_PI64), 2,
                 0.0, f.ptr, 2, r.ptr, t.ctypes.data_as(_PD), C.byref(k))
    assert e.value.code == L.EINVAL


# ------------------------------------------------------------------------------------------------ 2. smn_lowrank_grad
COEF = 1.37

#        n     m    d   net       act     depth fitc c
CASES = [(65, 1, 7, "mlp", "relu", 1, 1, 1),
         (65, 7, 24, "resnet", "erf", 2, 0, 3),
         (65, 65, 7, "mlp", "erf", 3, 1, 3),
         (130, 7, 7, "resnet", "relu", 1, 1, 3),
         (130, 65, 24, "mlp", "relu", 2, 0, 1),
         (130, 130, 7, "resnet", "erf", 3, 1, 1),
         (1300, 1, 24, "resnet", "relu", 2, 1, 1),
         (1300, 7, 7, "mlp", "erf", 1, 0, 3),
         (1300, 65, 7, "resnet", "erf", 1, 1, 3),
         (1300, 130, 24, "mlp", "relu", 3, 1, 3),
         (1300, 130, 7, "resnet", "relu", 2, 0, 1),
         (1300, 130, 7, "mlp", "erf", 2, 1, 1)]


def grad_call(ctx, L, fn, x, res, fit, y, fitc, layout, coef=COEF):
    """smn_lowrank_grad with x, the factor and the targets in NaN-guarded windows (ldx > d, ldl > m, ldy > c)."""
    n, d = x.shape
    m, c = res.rank, y.shape[1]
    xw = W.in_window(ctx, x, layout)
    lw = W.in_window(ctx, res.factor.raw_numpy().reshape(n, m), layout)
    yw = W.in_window(ctx, y, layout)
    resid = ctx.to_device(np.ascontiguousarray(res.resid, dtype=np.float64)) if fitc else None
    piv = np.ascontiguousarray(res.pivots, dtype=np.int64)
    terms = np.zeros(4)
    ctx.call("smn_lowrank_grad", L.dtype_code(x.dtype), fn.net, fn.act, fn.num_hiddens, fn.w_std, fn.b_std, fn.last_w_std, xw.ptr, n,
             xw.ld, d, piv.ctypes.data_as(_PI64), lw.ptr, m, lw.ld, None if resid is None else resid.ptr, fit.lam, 1 if fitc else 0,
             yw.ptr, c, yw.ld, fit.c_fac.ptr, fit.beta.ptr, fit.r_fac.ptr, m, coef, terms.ctypes.data_as(_PD))
    return terms


def check_against_rules(ctx, L, what, net, act, layers, hp, x, y, m, fitc, dtype, eps_list=(1e-1, 1e-2)):
    from smnngp import lowrank
    fn = kernel_fn(net, act, layers, hp)
    f32 = np.dtype(dtype) == np.float32
    xs = x.astype(dtype)
    ys = y.astype(dtype)
    res = lowrank.pivoted_cholesky(fn, xs, m)
    assert res.rank >= 1
    Lh = res.factor.raw_numpy().astype(np.float64).reshape(xs.shape[0], res.rank)
    kern = (net, act, layers, hp["w_std"], hp["b_std"], hp["last_w_std"], xs.astype(np.float64))
    worst = 0.0
    for eps in eps_list:
        fit = lowrank.woodbury_fit(res, ys, eps, bool(fitc))
        assert fit.info == 0, what
        got = grad_call(ctx, L, fn, xs, res, fit, ys, fitc, "aligned")
        assert np.all(np.isfinite(got)), (what, got)
        if f32:
            ref, S, yard = G.yardstick32(Lh, res.resid, res.pivots, eps, fitc, ys, COEF, kern, split=L.LOWRANK_SPLIT)
            bound = 16.0 * yard
        else:
            ref, S = G.formula(Lh, res.resid, res.pivots, eps, fitc, ys, COEF, kern)
            bound = 1e-8 * S
        assert np.all(np.isfinite(ref)) and np.all(np.isfinite(S))
        err = np.abs(got - ref)
        for t, name in enumerate(G.NAMES):
            mult = err[t] / bound[t] if bound[t] > 0.0 else (0.0 if err[t] == 0.0 else np.inf)
            worst = max(worst, mult)
            print("lowrank-grad-multiple %s-rank%d-eps%g-%s %s %.3g (|err| / S = %.3g)" % (
                what, res.rank, eps, np.dtype(dtype).name, name, mult, err[t] / S[t] if S[t] > 0.0 else 0.0))
        assert np.all(err <= bound), (what, eps, got, ref, bound)
    return worst


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_grad_terms_against_the_rules(ctx, L, case, dtype):
    n, m, d, net, act, layers, fitc, c = CASES[case]
    rng = np.random.default_rng(1000 + case)
    x = data(n, d, seed=case)
    y = np.sin(x[:, :1] * np.arange(1, c + 1)[None, :]) + 0.3 * rng.standard_normal((n, c))
    what = "n%d-m%d-d%d-%s-%s-L%d-%s-c%d" % (n, m, d, net, act, layers, "fitc" if fitc else "none", c)
    check_against_rules(ctx, L, what, net, act, layers, HP, x, y, m, fitc, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("net,act", [("mlp", "relu"), ("resnet", "relu"), ("mlp", "erf")])
def test_grad_terms_with_zero_duplicate_and_near_duplicate_rows_at_b_std_zero(ctx, L, net, act, dtype):
    """b_std = 0 with an all-zero row (zero variance at every layer: the dead-row rule of the tables), an exact duplicate of
    another row and a near duplicate (1 - c0 = 1e-4): every term finite and within the bound, the b_std term exactly 0."""
    n, d = 130, 7
    x = data(n, d, seed=11)
    x[17] = 0.0
    x[40] = x[3]
    u = x[8] / np.linalg.norm(x[8])
    v = x[9] - (x[9] @ u) * u
    v /= np.linalg.norm(v)
    th = np.arccos(1.0 - 1e-4)
    x[60] = np.linalg.norm(x[8]) * (np.cos(th) * u + np.sin(th) * v)
    rng = np.random.default_rng(5)
    y = np.sin(x[:, :1]) + 0.3 * rng.standard_normal((n, 1))
    hp = dict(w_std=1.3, b_std=0.0, last_w_std=0.9)
    for m, fitc in ((65, 1), (7, 0)):
        what = "bzero-%s-%s-m%d-%s" % (net, act, m, "fitc" if fitc else "none")
        check_against_rules(ctx, L, what, net, act, 2, hp, x, y, m, fitc, dtype)


# ------------------------------------------------------------------------------------------------ 3. determinism
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,m,d,c", [(130, 65, 7, 3), (1300, 130, 24, 1)])
def test_two_calls_and_both_layouts_give_the_same_bits(ctx, L, n, m, d, c, dtype):
    from smnngp import lowrank
    fn = kernel_fn("mlp", "relu", 2)
    x = data(n, d, seed=2).astype(dtype)
    y = np.random.default_rng(3).standard_normal((n, c)).astype(dtype)
    res = lowrank.pivoted_cholesky(fn, x, m)
    fit = lowrank.woodbury_fit(res, y, 1e-2, True)
    a = grad_call(ctx, L, fn, x, res, fit, y, 1, "aligned")
    b = grad_call(ctx, L, fn, x, res, fit, y, 1, "aligned")
    u = grad_call(ctx, L, fn, x, res, fit, y, 1, "unaligned")
    assert np.all(np.isfinite(a))
    assert a.tobytes() == b.tobytes(), "two calls differ"
    assert a.tobytes() == u.tobytes(), "the bits depend on the layout"
    w = lowrank.woodbury_grad(fit, fn, x, COEF)                            # the host wrapper: contiguous, ld = extent
    assert a.tobytes() == w.tobytes()


# ------------------------------------------------------------------------------------------------ 4. the model
def _model(lik, x, y, dtype=np.float64, make=None, kernel_cls=None, **kw):
    from smnngp import nt_kernels as nt
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.models import LowRankSPR
    make = make or (lambda w, b, l: nt.get_mlp_kernel(2, act="relu", w_std=w, b_std=b, last_w_std=l))
    kernel = (kernel_cls or NNGPKernel)(make, HP["w_std"], HP["b_std"], HP["last_w_std"])
    return LowRankSPR(kernel, lik, np.asarray(x, dtype=dtype), y, 0.3, 1.7, **kw)


def _lik(method):
    from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood
    return GaussianLikelihood() if method == "gp" else StudentTLikelihood(2.0, 3.4)


def _problem(n, d=8):
    x = data(n + 9, d, seed=n)
    rng = np.random.default_rng(n)
    y = np.sin(x[:n, 0]) + 0.1 * rng.standard_normal(n)
    return x[:n], y, x[n:]


@pytest.mark.parametrize("correction", ["fitc", "none"])
@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("n", [200, 300])
def test_frozen_model_loss_and_gradient(ctx, L, n, method, correction):
    from smnngp import train
    x, y, xt = _problem(n)
    model = _model(_lik(method), x, y, rank=24, correction=correction, eps=1e-2)
    with pytest.raises(NotImplementedError):
        model.loss_and_grad()
    loss, (mean, var) = model.loss(), model.predict(xt)
    nll = model.test_nll(xt, np.cos(xt[:, 0]))
    greedy = model._factor()[1]
    assert model.freeze_pivots() is model and np.array_equal(model.pivots, greedy.pivots)
    for clear in (False, True):                                            # the kept factor, then one rebuilt at the pivots
        if clear:
            model._factor_cache = None
        assert model.loss() == loss
        m2, v2 = model.predict(xt)
        assert np.array_equal(m2, mean) and np.array_equal(v2, var)
        assert model.test_nll(xt, np.cos(xt[:, 0])) == nll
    assert model._factor()[1] is not greedy and np.array_equal(model._factor()[1].pivots, greedy.pivots)
    value, grads = model.loss_and_grad()
    assert value == model.loss()
    variables = train.train_vars(model)
    assert set(grads) == set(variables) and len(grads) == (6 if method == "tp" else 4)
    _, fd = train.value_and_grad_fd(model.loss, variables, h=1e-5)
    for name in sorted(grads):
        rel = abs(grads[name] - fd[name]) / abs(fd[name])
        print("lowrank-grad-model n%d-%s-%s %s analytic %.12g fd %.12g rel %.3g" % (n, method, correction, name, grads[name], fd[name], rel))
        assert rel <= 1e-6, (name, grads[name], fd[name])
    assert model.unfreeze_pivots() is model and model.pivots is None
    with pytest.raises(NotImplementedError):
        model.loss_and_grad()


# the two routes' disagreement on the loss value itself, measured on an MI355X: 6.0e-14 relative, the largest over the eight cases
# below (profiles/r34_lowrank_grad.txt), x 16
FULL_RANK_ALLOWANCE = 16.0 * 6.0e-14


@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("n", [200, 300])
def test_full_rank_frozen_gradient_is_the_exact_models(ctx, L, n, method):
    """rank = N with every point frozen, f64: K^ is K + eps I, and SPR.loss_and_grad -- which shares no code with the low-rank
    route -- must give the same gradient."""
    from smnngp import nt_kernels as nt
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.models import SPR
    x, y, _ = _problem(n)
    kernel = NNGPKernel(lambda w, b, l: nt.get_mlp_kernel(2, act="relu", w_std=w, b_std=b, last_w_std=l), HP["w_std"], HP["b_std"],
                        HP["last_w_std"])
    exact = SPR(kernel, _lik(method), x, y, 0.3, 1.7, eps=1e-2)
    ev, eg = exact.loss_and_grad()
    for correction in ("fitc", "none"):
        model = _model(_lik(method), x, y, rank=n, correction=correction, eps=1e-2).freeze_pivots()
        assert len(model.pivots) == n
        value, grads = model.loss_and_grad()
        dl = abs(value - ev) / abs(ev)
        print("lowrank-grad-fullrank n%d-%s-%s loss disagreement %.3g" % (n, method, correction, dl))
        tail = lambda k: k.split(").", 1)[1]                               # names agree up to the class name in front
        mine = {tail(k): v for k, v in grads.items()}
        assert set(mine) == {tail(k) for k in eg}
        scale = max(abs(v) for v in eg.values())
        worst = 0.0
        for k in sorted(eg):
            e = abs(mine[tail(k)] - eg[k]) / scale
            worst = max(worst, e)
            print("lowrank-grad-fullrank n%d-%s-%s %s |diff| / max |grad| %.3g = %.3g of the allowance"
                  % (n, method, correction, tail(k), e, e / FULL_RANK_ALLOWANCE))
        assert worst <= FULL_RANK_ALLOWANCE, (method, correction, worst)


def test_analytic_training_step_and_refresh(ctx, L):
    from smnngp import train
    n = 200
    x, y, _ = _problem(n)
    model = _model(_lik("gp"), x, y, rank=24, eps=1e-2).freeze_pivots()
    old = model.pivots
    step = train.build_train_step(model, method="analytic")
    before = step(5e-2)
    after = model.loss()
    assert np.array_equal(model.pivots, old), "a training step must not move the frozen pivots"
    assert after < before, (before, after)
    auto = train.build_train_step(model, method="auto")
    assert auto(5e-2) == after and model.loss() < after                    # auto takes the analytic route on a frozen model
    # hyper-parameters far from where the pivots were chosen: the rules' greedy selection moves, so must the device's
    model.kernel.b_std.assign(model.kernel.b_std.constraint.inverse(np.float64(3.0)))
    w, b, lw = model.kernel.get_params()
    new_rule = PR.pivoted_cholesky(G.oracle_kernel("mlp", "relu", 2, w, b, lw, x), 24).pivots
    old_rule = PR.pivoted_cholesky(G.oracle_kernel("mlp", "relu", 2, HP["w_std"], HP["b_std"], HP["last_w_std"], x), 24).pivots
    stale = model._factor()[1]
    assert np.array_equal(stale.pivots, old)
    assert model.refresh_pivots() is model
    assert model._factor()[1] is not stale and len(model.pivots) == 24
    if not np.array_equal(np.sort(new_rule), np.sort(old_rule)):
        assert not np.array_equal(model.pivots, old)
    assert np.isfinite(model.loss_and_grad()[0])


# ------------------------------------------------------------------------------------------------ 5. what is refused
def test_ntk_and_conv_kernels_are_refused_before_any_launch(ctx, L, monkeypatch):
    from smnngp import lowrank
    from smnngp import nt_kernels as nt
    from smnngp.spax.kernels import NTKKernel
    n = 65
    x, y, _ = _problem(n)
    fn = kernel_fn("mlp", "relu", 2)
    res = lowrank.pivoted_cholesky(fn, x, 7)
    fit = lowrank.woodbury_fit(res, y, 1e-2, True)
    images = np.random.default_rng(1).standard_normal((24, 4, 4, 1))
    ntk_model = _model(_lik("gp"), x, y, kernel_cls=NTKKernel, rank=7, eps=1e-2).freeze_pivots(np.arange(7))
    cnn_model = _model(_lik("gp"), images, np.zeros(24), rank=5, eps=1e-2,
                       make=lambda w, b, l: nt.get_cnn_kernel(2, act="relu", w_std=w, b_std=b, last_w_std=l)).freeze_pivots(np.arange(5))
    xd = ctx.to_device(x)
    resid = ctx.to_device(res.resid)
    piv, terms = np.ascontiguousarray(res.pivots), np.zeros(4)
    args = (xd.ptr, n, 8, 8, piv.ctypes.data_as(_PI64), res.factor.ptr, 7, 7, resid.ptr, 1e-2, 1, fit.y_dev.ptr, 1, 1, fit.c_fac.ptr,
            fit.beta.ptr, fit.r_fac.ptr, 7, 1.0, terms.ctypes.data_as(_PD))
    with pytest.raises(L.SmnError) as e:
        ctx.call("smn_lowrank_grad", L.F64, fn.net | L.NET_NTK, fn.act, 2, 1.3, 0.2, 0.9, *args)
    assert e.value.code == L.ENOTSUP
    with pytest.raises(L.SmnError) as e:                                    # a pivot listed twice: SMN_EINVAL, nothing launched
        twice = np.asarray([res.pivots[0]] * 2 + list(res.pivots[2:]), dtype=np.int64)
        ctx.call("smn_lowrank_grad", L.F64, fn.net, fn.act, 2, 1.3, 0.2, 0.9, *(args[:4] + (twice.ctypes.data_as(_PI64),) + args[5:]))
    assert e.value.code == L.EINVAL

    def no_call(self, name, *a, **k):
        raise AssertionError("%s was called" % name)
    monkeypatch.setattr(type(ctx), "call", no_call)
    for model in (ntk_model, cnn_model):
        with pytest.raises(NotImplementedError):
            model.loss_and_grad()
    with pytest.raises(NotImplementedError):
        lowrank.woodbury_grad(fit, fn.with_cov("ntk"), x, 1.0)
