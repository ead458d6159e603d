"""CPU-side checks of the batched analytic gradient (smn_spr_loss_grad_batch, sweeps.loss_and_grad_batch,
train.build_multistart_step): the C-ABI entry exists and rejects a NULL context, and the host logic of the multi-start
step -- per-start chain rule, element-wise Adam, NaN starts, best / assign_best -- reproduces independent single-start
runs when the device call is replaced by the fp64 oracle.  No GPU needed."""
import ctypes as C
import types

import numpy as np
import pytest

from oracle import nngp_oracle as O  # noqa: E402  (test infrastructure only)

LAYERS, ACT = 2, "relu"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from smnngp import _lib
    return _lib


def test_library_exports_the_batched_gradient_entry_and_it_rejects_a_null_context(lib):
    raw = C.CDLL(lib.LIB_PATH)
    assert hasattr(raw, "smn_spr_loss_grad_batch"), "libsmnngp.so does not export smn_spr_loss_grad_batch"
    assert "smn_spr_loss_grad_batch" in lib.PROTOTYPES
    one = (C.c_double * 1)(1.0)
    terms = (C.c_double * 4)()
    rc = lib._lib.smn_spr_loss_grad_batch(None, lib.F64, lib.NET_MLP, lib.ACT["relu"], 1, 1, one, one, one, None, 4, 4, 4, None,
                                          one, None, None, None, None, None, terms)
    assert rc == lib.EINVAL


def _oracle_batch(calls):
    """Stand-in for sweeps.loss_and_grad_batch: quad, logdet and terms of every problem in NumPy fp64 (oracle kernel,
    dK/dw_std and dK/db_std by central differences of it, numpy.linalg for the rest)."""
    from smnngp.spax.models import lml_value_and_grads

    def fake(ctx, x, y, *, network, num_hiddens, activation, w_std, b_std, last_w_std=1.0, eps, df=0.0, scale=1.0):
        assert network == "mlp" and activation == ACT and num_hiddens == LAYERS
        g = max(np.size(v) for v in (w_std, b_std, last_w_std, eps, df, scale))
        calls.append(g)
        w, b, lw, e, dfs, scs = (np.broadcast_to(np.asarray(v, dtype=np.float64), (g,)) for v in (w_std, b_std, last_w_std, eps, df, scale))
        xh, yh = x.host, y.host
        n = xh.shape[0]
        lp, quad, logdet = np.full(g, np.nan), np.full(g, np.nan), np.full(g, np.nan)
        info, terms = np.zeros(g, dtype=np.int32), np.full((g, 4), np.nan)
        for i in range(g):
            kfn = lambda ww, bb: O.mlp_kernel(xh, None, LAYERS, ACT, ww, bb, lw[i])      # noqa: E731
            k = kfn(w[i], b[i])
            kt = k + e[i] * np.eye(n)
            ev = np.linalg.eigvalsh(kt)
            if ev[0] <= 1e-13 * ev[-1]:                              # not (numerically) positive definite
                info[i] = 1
                continue
            kinv = np.linalg.inv(kt)
            al = kinv @ yh
            quad[i] = float(yh @ al)
            logdet[i] = float(np.linalg.slogdet(kt)[1])
            coef = 1.0 if dfs[i] <= 0 else (dfs[i] + n) / ((dfs[i] + quad[i] / scs[i]) * scs[i])
            gm = coef * np.outer(al, al) - kinv
            h = 1e-6
            dkw = (kfn(w[i] + h, b[i]) - kfn(w[i] - h, b[i])) / (2 * h)
            dkb = (kfn(w[i], b[i] + h) - kfn(w[i], b[i] - h)) / (2 * h)
            terms[i] = [np.sum(gm * dkw), np.sum(gm * dkb), np.sum(gm * k) * 2.0 / lw[i], np.trace(gm)]
            lp[i] = lml_value_and_grads(terms[i], quad[i], logdet[i], n, dfs[i], scs[i], 1.0, 1.0)[0]
        return lp, quad, logdet, info, terms

    return fake


def _model(method, kernel_factory=None):
    """An SPR whose data live on the host only (the stand-in reads .host): nothing here touches a device."""
    from smnngp import nt_kernels
    from smnngp.spax.base import ConstraintTrainVar
    from smnngp.spax.bijectors import positive
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood
    from smnngp.spax.models import SPR
    rng = np.random.default_rng(3)
    n, d = 40, 4
    x = rng.standard_normal((n, d))
    x[7] = x[3]                                                   # two equal rows: singular without a shift
    y = np.sin(x[:, 0]) + 0.3 * rng.standard_normal(n)
    factory = kernel_factory or (lambda w, b, l: nt_kernels.get_mlp_kernel(LAYERS, 1, act=ACT, w_std=w, b_std=b, last_w_std=l))
    model = SPR.__new__(SPR)
    model.kernel = NNGPKernel(factory, 1.0, 0.5, 1.0)
    model.likelihood = GaussianLikelihood() if method == "gp" else StudentTLikelihood(2.0, 2.0)
    model.x_data = types.SimpleNamespace(host=x, shape=x.shape, dtype=np.float64, ctx=None)
    model.y_data = types.SimpleNamespace(host=y)
    model.y_host = y
    model.num_data = n
    model.eps = ConstraintTrainVar(1e-2, constraint=positive())
    return model


def _starts(model, g, seed, bad=None):
    """g raw starting points around the model's own values; start `bad` gets a raw eps so negative that eps underflows
    and the matrix with its two equal rows is no longer positive definite."""
    rng = np.random.default_rng(seed)
    starts = {k: float(v.value) + 0.3 * rng.standard_normal(g) for k, v in model.vars().items()}
    if bad is not None:
        starts[[k for k in starts if k.endswith(".eps")][0]][bad] = -800.0
    return starts


@pytest.mark.parametrize("method", ["gp", "tp"])
def test_multistart_step_reproduces_independent_single_start_runs(lib, monkeypatch, method):
    from smnngp import sweeps, train
    calls = []
    monkeypatch.setattr(sweeps, "loss_and_grad_batch", _oracle_batch(calls))
    g, steps, lr = 5, 20, 0.05
    model = _model(method)
    assert len(model.vars()) == (4 if method == "gp" else 6)
    starts = _starts(model, g, 11)
    multi = train.build_multistart_step(model, starts)
    hist = np.array([multi(lr) for _ in range(steps)])            # [steps, g]
    assert calls == [g] * steps                                    # one batched call per step
    assert np.isfinite(hist).all() and (hist[-1] < hist[0]).all()
    for s in range(g):
        single = train.build_multistart_step(_model(method), {k: v[s:s + 1] for k, v in starts.items()})
        one = np.array([single(lr)[0] for _ in range(steps)])
        assert np.allclose(one, hist[:, s], rtol=1e-12, atol=0.0), (s, np.abs(one - hist[:, s]).max())
        for k in starts:
            assert abs(single.raw[k][0] - multi.raw[k][s]) <= 1e-12 * abs(single.raw[k][0]), (s, k)
    assert np.array_equal(multi.losses, hist[-1])
    assert multi.best() == int(np.argmin(hist[-1]))


@pytest.mark.parametrize("method", ["gp", "tp"])
def test_a_start_that_is_not_positive_definite_stays_nan_and_leaves_the_others_alone(lib, monkeypatch, method):
    from smnngp import sweeps, train
    monkeypatch.setattr(sweeps, "loss_and_grad_batch", _oracle_batch([]))
    g, steps, lr, bad = 5, 20, 0.05, 2
    model = _model(method)
    clean, broken = _starts(model, g, 11), _starts(model, g, 11, bad=bad)
    ref = train.build_multistart_step(_model(method), clean)
    multi = train.build_multistart_step(model, broken)
    frozen = {k: v[bad] for k, v in multi.raw.items()}
    for _ in range(steps):
        want, got = ref(lr), multi(lr)
        assert np.isnan(got[bad])
        keep = np.arange(g) != bad
        assert np.array_equal(got[keep], want[keep])
    for k in clean:
        assert multi.raw[k][bad] == frozen[k]                      # left where it was
        assert np.array_equal(multi.raw[k][keep], ref.raw[k][keep])
    best = multi.best()
    assert best != bad and multi.losses[best] == np.nanmin(multi.losses)
    assert multi.assign_best() == best
    for k, v in model.vars().items():
        assert float(v.value) == multi.raw[k][best]
    # every start NaN: nothing to choose from
    allbad = train.build_multistart_step(_model(method), {k: v[bad:bad + 1] for k, v in broken.items()})
    assert np.isnan(allbad(lr)).all()
    with pytest.raises(ValueError):
        allbad.best()


def test_multistart_refuses_conv_kernels_and_malformed_starts(lib):
    from smnngp import nt_kernels, train
    cnn = _model("gp", lambda w, b, l: nt_kernels.get_cnn_kernel(2, 1, act="relu", w_std=w, b_std=b, last_w_std=l))
    with pytest.raises(NotImplementedError):
        train.build_multistart_step(cnn, _starts(cnn, 3, 0))
    model = _model("gp")
    starts = _starts(model, 3, 0)
    with pytest.raises(ValueError):
        train.build_multistart_step(model, {k: v for k, v in list(starts.items())[:-1]})      # a trainable is missing
    ragged = dict(starts)
    ragged[next(iter(ragged))] = np.zeros(2)
    with pytest.raises(ValueError):
        train.build_multistart_step(model, ragged)
