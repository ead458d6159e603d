"""GPU tests of the batched analytic gradient: smn_spr_loss_grad_batch (csrc/grad.hip) against the serial
smn_spr_loss_grad bit for bit, against central differences of the fp64 oracle, and train.build_multistart_step against
independent build_train_step runs."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import nngp_oracle as O  # noqa: E402  (test infrastructure only)


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


# the seven problems of test_batched_loss_and_predict_are_bit_identical_to_the_serial_calls (test_gpu_parity.py)
WS = np.array([1.0, 1.4, 2.0, 0.7, 1.0, 1.2, 1.0])
BS = np.array([0.0, 0.3, 1.0, 0.1, 1e-8, 0.5, 0.2])
LWS = np.array([1.0, 1.0, 0.5, 2.0, 1.0, 1.0, 1.0])
EPS = np.array([1e-2, 1e-1, 1e-3, 1e-2, 1e-2, 3e-2, -50.0])      # the last one: a negative shift -> not positive definite
DFS = np.array([0.0, 4.0, 0.0, 2.0, 6.0, 0.0, 0.0])
SCS = np.array([1.0, 1.5, 1.0, 0.5, 2.0, 1.0, 1.0])


def _serial(L, ctx, x, y, net, act, layers, b, ws=WS, bs=BS, lws=LWS, eps=EPS, dfs=DFS, scs=SCS):
    n, d = x.shape
    quad, logdet, info = C.c_double(), C.c_double(), C.c_int()
    terms = (C.c_double * 4)()
    netc = L.NET_MLP if net == "mlp" else L.NET_DENSE_RESNET
    ctx.call("smn_spr_loss_grad", x.dcode, netc, L.ACT[act], layers, ws[b], bs[b], lws[b], x.ptr, n, d, d, y.ptr, eps[b], dfs[b],
             scs[b], C.byref(quad), C.byref(logdet), C.byref(info), terms)
    return quad.value, logdet.value, info.value, tuple(terms)


def _check(got, want, b, gb, tag):
    lp, quad, logdet, info, terms = got
    if want[2]:
        assert info[gb] == want[2] and np.isnan(quad[gb]) and np.isnan(logdet[gb]) and np.isnan(terms[gb]).all(), (b, tag)
        assert np.isnan(lp[gb])
    else:
        assert (quad[gb], logdet[gb], info[gb], tuple(terms[gb])) == want, (b, tag)
        assert np.isfinite(lp[gb])


def _per_problem_bytes(n, dtype):
    n_total = (n + 127) // 128 * 128 + (n + 1 + 127) // 128 * 128    # the joint matrix [[K~, .], [I, 0], [y^T, 0, 0]]
    return n_total * n_total * np.dtype(dtype).itemsize


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,d,net,act,layers", [(245, 6, "mlp", "relu", 2), (700, 12, "mlp", "erf", 3), (1300, 20, "resnet", "relu", 2),
                                                 (2048, 8, "mlp", "relu", 4)])
def test_batched_gradient_is_bit_identical_to_the_serial_calls(L, ctx, dtype, n, d, net, act, layers):
    """Every positive-definite problem returns (quad, logdet, info, terms[0..3]) equal to smn_spr_loss_grad's with ==,
    Student-t problems included (their coef comes from the problem's own quad); the one that is not reports its own info
    and NaNs; in one pass, in chunks of at most three problems, and as a batch of one."""
    from smnngp import sweeps
    rng = np.random.default_rng(500 + n)
    xh = rng.standard_normal((n, d)).astype(dtype)
    xh[7] = xh[3]                                              # two equal rows: singular without a shift
    yh = rng.standard_normal((n, 1)).astype(dtype)
    x, y = ctx.to_device(xh), ctx.to_device(yh)
    g = len(WS)
    want = [_serial(L, ctx, x, y, net, act, layers, b) for b in range(g)]
    assert want[-1][2] > 0 and all(w[2] == 0 for w in want[:-1])
    assert all(np.isfinite(w[3]).all() for w in want[:-1]) and np.isnan(want[-1][3]).all()
    kw = dict(network=net, num_hiddens=layers, activation=act)
    try:
        for budget in (1 << 40, 3 * _per_problem_bytes(n, dtype)):        # one pass; chunks of at most three problems
            ctx.call("smn_debug_batch_bytes", int(budget))
            got = sweeps.loss_and_grad_batch(ctx, x, y, w_std=WS, b_std=BS, last_w_std=LWS, eps=EPS, df=DFS, scale=SCS, **kw)
            for b in range(g):
                _check(got, want[b], b, b, budget)
        ctx.call("smn_debug_batch_bytes", 48 << 30)
        for b in (1, 3, 6):                                                # G = 1: Student-t twice, the one that is not PD
            got = sweeps.loss_and_grad_batch(ctx, x, y, w_std=WS[b], b_std=BS[b], last_w_std=LWS[b], eps=EPS[b], df=DFS[b],
                                             scale=SCS[b], **kw)
            assert len(got[0]) == 1
            _check(got, want[b], b, 0, "G=1")
    finally:
        ctx.call("smn_debug_batch_bytes", 48 << 30)


def test_argument_errors_follow_the_batched_loss(L, ctx):
    x = ctx.to_device(np.ones((8, 2))); y = ctx.to_device(np.ones((8, 1)))
    one = (C.c_double * 1)(1.0)
    bad = (C.c_double * 1)(0.0)
    terms = (C.c_double * 4)()
    args = lambda nprob, w, eps, df, sc: ("smn_spr_loss_grad_batch", L.F64, L.NET_MLP, L.ACT["relu"], 1, nprob, w, one, one, x.ptr, 8, 2, 2,   # noqa: E731
                                           y.ptr, eps, df, sc, None, None, None, terms)
    for a in (args(0, one, one, None, None), args(1, None, one, None, None), args(1, one, None, None, None),
              args(1, one, one, one, bad), args(1, one, one, one, None)):
        with pytest.raises(L.SmnError):
            ctx.call(*a)
    ctx.call(*args(1, one, one, None, None))                               # quad / logdet / info may be NULL
    assert np.isfinite(np.array(terms)).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("method", ["gp", "tp"])
def test_multistart_gradients_match_finite_differences_of_the_oracle(dtype, method):
    """The gradient build_multistart_step forms for three starts against central differences of the fp64 oracle loss:
    the shapes and tolerances of test_analytic_loss_gradient_matches_finite_differences_of_the_oracle (2e-6 of the
    largest reference gradient in float64, 1e-2 in float32; the loss to 1e-9 / 1e-3)."""
    from smnngp import nt_kernels, train
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood
    from smnngp.spax.models import SPR
    rng = np.random.default_rng(17)
    n, d, nh, act = 150, 6, 2, "relu"
    x = rng.standard_normal((n, d))
    y = np.sin(x[:, 0]) + 0.3 * rng.standard_normal(n)
    hyps = [dict(w_std=1.3, b_std=0.4, last_w_std=0.9, eps=5e-2, alpha=1.7, beta=2.4),
            dict(w_std=0.8, b_std=0.9, last_w_std=1.4, eps=2e-1, alpha=2.5, beta=1.1),
            dict(w_std=1.9, b_std=0.1, last_w_std=0.6, eps=1e-2, alpha=1.2, beta=3.0)]
    kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_mlp_kernel(nh, 1, act=act, w_std=w, b_std=b, last_w_std=l), 1.0, 1.0, 1.0)
    lik = GaussianLikelihood() if method == "gp" else StudentTLikelihood(2.0, 2.0)
    model = SPR(kernel, lik, x.astype(dtype), y.astype(dtype), 0.0, 1.0, eps=1e-2)
    vmap = {"w_std": kernel.w_std, "b_std": kernel.b_std, "last_w_std": kernel.last_w_std, "eps": model.eps}
    if method == "tp":
        vmap.update(alpha=lik.a, beta=lik.b)
    names = {id(v): k for k, v in model.vars().items()}
    starts = {names[id(var)]: np.array([float(var.constraint.inverse(h[key])) for h in hyps]) for key, var in vmap.items()}
    multi = train.build_multistart_step(model, starts)
    losses, grads = multi.value_and_grad()
    assert set(grads) == set(model.vars())
    tol = 2e-6 if dtype == np.float64 else 1e-2
    for s, hyp in enumerate(hyps):
        okw = dict(kernel="mlp", num_hiddens=nh, act=act, method=method, **hyp)
        ref = O.spr_loss_grad_fd(x, y, keys=tuple(vmap), **okw)
        rl = O.spr_loss(x, y, **okw)
        print("start %d: loss %.12g oracle %.12g" % (s, losses[s], rl))
        assert abs(losses[s] - rl) < (1e-9 if dtype == np.float64 else 1e-3) * max(1.0, abs(rl))
        scale = max(abs(v) for v in ref.values())
        for key, var in vmap.items():
            name = names[id(var)]
            got = grads[name][s] / float(var.constraint.grad(starts[name][s]))     # undo the softplus chain rule
            print("  %s: got %.10g ref %.10g" % (key, got, ref[key]))
            assert abs(got - ref[key]) < tol * max(scale, abs(ref[key])), (s, key, got, ref[key])


def test_other_entry_points_are_undisturbed(L, ctx):
    """K0 is shared by the problems of ONE call, not kept: another x of the same shape gives that x's serial results; a
    smn_spr_loss between two batched calls changes nothing; the Gram cache's counters do not move."""
    from smnngp import sweeps
    n, d, net, act, layers, dtype = 700, 12, "mlp", "relu", 2, np.float32
    rng = np.random.default_rng(9)
    x1 = ctx.to_device(rng.standard_normal((n, d)).astype(dtype))
    x2 = ctx.to_device(rng.standard_normal((n, d)).astype(dtype))
    y = ctx.to_device(rng.standard_normal((n, 1)).astype(dtype))
    idx = [0, 1, 3]
    sel = dict(w_std=WS[idx], b_std=BS[idx], last_w_std=LWS[idx], eps=EPS[idx], df=DFS[idx], scale=SCS[idx])
    kw = dict(network=net, num_hiddens=layers, activation=act, **sel)

    def stats():
        h, m, by = C.c_int64(), C.c_int64(), C.c_size_t()
        ctx.call("smn_gram_cache_stats", C.byref(h), C.byref(m), C.byref(by))
        return h.value, m.value, by.value

    before = stats()
    want1 = [_serial(L, ctx, x1, y, net, act, layers, b) for b in idx]
    want2 = [_serial(L, ctx, x2, y, net, act, layers, b) for b in idx]
    got1 = sweeps.loss_and_grad_batch(ctx, x1, y, **kw)
    got2 = sweeps.loss_and_grad_batch(ctx, x2, y, **kw)
    assert stats() == before
    lp, quad, logdet, info = C.c_double(), C.c_double(), C.c_double(), C.c_int()
    ctx.call("smn_spr_loss", x1.dcode, L.NET_MLP, L.ACT[act], layers, 1.1, 0.2, 1.0, x1.ptr, n, d, d, y.ptr, 1e-2, 0.0, 1.0,
             C.byref(lp), C.byref(quad), C.byref(logdet), C.byref(info))
    loss_between = (lp.value, quad.value, logdet.value, info.value)
    got1b = sweeps.loss_and_grad_batch(ctx, x1, y, **kw)
    ctx.call("smn_spr_loss", x1.dcode, L.NET_MLP, L.ACT[act], layers, 1.1, 0.2, 1.0, x1.ptr, n, d, d, y.ptr, 1e-2, 0.0, 1.0,
             C.byref(lp), C.byref(quad), C.byref(logdet), C.byref(info))
    assert (lp.value, quad.value, logdet.value, info.value) == loss_between and info.value == 0
    for gb, b in enumerate(idx):
        _check(got1, want1[gb], b, gb, "x1")
        _check(got2, want2[gb], b, gb, "x2")
        _check(got1b, want1[gb], b, gb, "x1 again")
    assert want1[0][3] != want2[0][3]


def test_large_n_runs_the_problems_through_the_serial_route(L, ctx):
    """From n_pad = 8192 on the serial call takes the rectangle route and one problem fills the chip: the batched entry runs
    the problems one after another and fills the same outputs."""
    from smnngp import sweeps
    n, d, dtype = 8192, 16, np.float32
    rng = np.random.default_rng(4)
    x = ctx.to_device(rng.standard_normal((n, d)).astype(dtype))
    y = ctx.to_device(rng.standard_normal((n, 1)).astype(dtype))
    idx = [1, 5]
    want = [_serial(L, ctx, x, y, "mlp", "relu", 2, b) for b in idx]
    got = sweeps.loss_and_grad_batch(ctx, x, y, network="mlp", num_hiddens=2, activation="relu", w_std=WS[idx], b_std=BS[idx],
                                     last_w_std=LWS[idx], eps=EPS[idx], df=DFS[idx], scale=SCS[idx])
    for gb, b in enumerate(idx):
        assert want[gb][2] == 0
        _check(got, want[gb], b, gb, "n=8192")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("method", ["gp", "tp"])
def test_multistart_training_equals_independent_single_start_runs(dtype, method):
    """G = 8 starts over 10 steps equal 8 runs of build_train_step(method="analytic") from the same raw values: the
    device outputs agree bit for bit and the host arithmetic is the same float64 arithmetic, so losses and raw values
    agree to 1e-12 relative.  assign_best() leaves a model that test_nll evaluates."""
    from smnngp import nt_kernels, train
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood
    from smnngp.spax.models import SPR
    rng = np.random.default_rng(23)
    n, d, g, steps, lr = 245, 6, 8, 10, 0.05
    x = rng.standard_normal((n, d)).astype(dtype)
    y = (np.sin(x[:, 0]) + 0.3 * rng.standard_normal(n)).astype(dtype)
    xt = rng.standard_normal((32, d)).astype(dtype)
    yt = np.sin(xt[:, 0]).astype(dtype)

    def make():
        kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_mlp_kernel(2, 1, act="relu", w_std=w, b_std=b, last_w_std=l), 1.0, 0.5, 1.0)
        lik = GaussianLikelihood() if method == "gp" else StudentTLikelihood(2.0, 2.0)
        return SPR(kernel, lik, x, y, 0.0, 1.0, eps=1e-2)

    model = make()
    starts = {k: float(v.value) + 0.4 * rng.standard_normal(g) for k, v in model.vars().items()}
    multi = train.build_multistart_step(model, starts)
    hist = np.array([multi(lr) for _ in range(steps)])
    assert np.isfinite(hist).all()
    for s in range(g):
        single = make()
        for k, v in single.vars().items():
            v.assign(starts[k][s])
        step = train.build_train_step(single, method="analytic")
        one = np.array([step(lr) for _ in range(steps)])
        assert np.allclose(one, hist[:, s], rtol=1e-12, atol=0.0), (s, np.abs(one - hist[:, s]).max())
        for k, v in single.vars().items():
            assert abs(float(v.value) - multi.raw[k][s]) <= 1e-12 * abs(float(v.value)), (s, k)
    best = multi.assign_best()
    assert best == int(np.argmin(hist[-1]))
    for k, v in model.vars().items():
        assert float(v.value) == multi.raw[k][best]
    assert np.isfinite(model.test_nll(xt, yt))
