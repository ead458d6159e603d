"""Host logic of the fitted posterior (posterior.py): the chunk planner and FittedPosterior on a stand-in context that records
the C-ABI calls instead of making them.  No GPU needed."""
import ctypes as C
import types

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from smnngp import _lib
    return _lib


@pytest.mark.parametrize("T,cap", [(1, 1), (5, 128), (127, 128), (128, 128), (129, 128), (256, 128), (257, 128), (1000, 7),
                                   (100000, 2048), (3, 1)])
def test_chunks_cover_every_row_once_in_order(lib, T, cap):
    from smnngp.posterior import chunks
    plan = chunks(T, cap)
    assert len(plan) == -(-T // cap)
    assert [s for s, _ in plan] == list(range(0, T, cap))
    assert all(1 <= r <= cap for _, r in plan) and all(r == cap for _, r in plan[:-1])
    covered = np.concatenate([np.arange(s, s + r) for s, r in plan])
    assert np.array_equal(covered, np.arange(T))
    assert plan[-1][1] == (T - 1) % cap + 1                       # T a multiple of the capacity: a full last chunk, no empty one


def test_chunks_edge_cases(lib):
    from smnngp.posterior import chunks
    assert chunks(0, 4) == []
    assert chunks(4, 4) == [(0, 4)] and chunks(5, 4) == [(0, 4), (4, 1)] and chunks(3, 4) == [(0, 3)]
    for bad in ((5, 0), (-1, 4)):
        with pytest.raises(ValueError):
            chunks(*bad)


class StubArray:
    _next = 4096

    def __init__(self, ctx, shape, dtype):
        self.ctx, self.shape, self.dtype = ctx, tuple(shape), np.dtype(dtype)
        StubArray._next += 4096
        self.ptr = C.c_void_p(StubArray._next)                     # a distinct fake address, never dereferenced


class StubContext:
    """Context look-alike: records (entry, arguments), fills the outputs of the create entries."""
    handle = object()

    def __init__(self):
        self.calls = []

    def empty(self, shape, dtype):
        return StubArray(self, shape, dtype)

    def to_device(self, host, dtype=None):
        host = np.asarray(host, dtype=dtype)
        return StubArray(self, host.shape, host.dtype)

    def call(self, name, *args):
        self.calls.append((name, args))
        if name == "smn_fit_create":
            args[16]._obj.value = 0xF17                             # smn_fit** out
            args[18]._obj.value = 1.5                               # logdet_h
            args[19]._obj.value = 0                                 # info_h

    def call_on(self, name, handle, *args):
        self.calls.append((name, (handle,) + args))
        if name == "smn_fit_info":
            args[3]._obj.value = 12345


def _stub_model(ctx, n=40, d=4):
    from smnngp import nt_kernels
    from smnngp.spax.base import ConstraintTrainVar
    from smnngp.spax.bijectors import positive
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.likelihoods import GaussianLikelihood
    from smnngp.spax.models import SPR
    model = SPR.__new__(SPR)
    model.kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_mlp_kernel(2, 1, act="relu", w_std=w, b_std=b, last_w_std=l), 1.1, 0.4, 1.0)
    model.likelihood = GaussianLikelihood()
    model.x_data = StubArray(ctx, (n, d), np.float32)
    model.y_data = StubArray(ctx, (n,), np.float32)
    model.y_host = np.zeros(n)
    model.y_mean, model.y_std, model.num_data = 0.0, 1.0, n
    model.eps = ConstraintTrainVar(1e-2, constraint=positive())
    return model


def test_posterior_on_a_stub_context(lib):
    ctx = StubContext()
    model = _stub_model(ctx)
    post = model.posterior(capacity=8)
    name, args = ctx.calls[0]
    assert name == "smn_fit_create"
    # (dtype, net, act, depth, w, b, lw, x, n, ldx, d, y, c, ridge_rel, ridge_abs, capacity, ...): eps is the RELATIVE ridge
    assert args[0] == lib.F32 and args[1] == lib.NET_MLP and args[3] == 2
    assert args[4:7] == pytest.approx((1.1, 0.4, 1.0), rel=1e-12)
    assert args[8:11] == (40, 4, 4) and args[12] == 1
    assert args[13] == pytest.approx(1e-2, rel=1e-12) and args[14] == 0.0 and args[15] == 8
    assert (post.capacity, post.num_data, post.nbytes, post.logdet, post.info) == (8, 40, 12345, 1.5, 0)
    # an unknown cov= value, and a full covariance above the capacity: refused by name before any device call
    made = len(ctx.calls)
    with pytest.raises(ValueError, match="cov must be"):
        post.predict(np.zeros((3, 4), np.float32), cov="banana")
    with pytest.raises(ValueError, match="capacity = 8"):
        post.predict(np.zeros((9, 4), np.float32), cov="full")
    assert [c[0] for c in ctx.calls[made:]] == []
    with pytest.raises(ValueError, match="features"):
        post.predict(np.zeros((3, 5), np.float32))
    # the diagonal has no such limit: one call, any T; var and no cov
    mean, var = post.predict(np.zeros((100, 4), np.float32))
    name, args = ctx.calls[-1]
    assert name == "smn_fit_predict" and args[0].value == 0xF17 and args[2:4] == (100, 4)
    assert mean.shape == (100, 1) and var.shape == (100,) and args[5] is var.ptr and args[6] is None
    # the snapshot does not move with the model's variables
    snap = dict(post.hyper)
    model.kernel.w_std.assign(model.kernel.w_std.constraint.inverse(np.asarray(2.5)))
    model.eps.assign(model.eps.constraint.inverse(np.asarray(0.3)))
    assert post.hyper == snap and snap["w_std"] == pytest.approx(1.1, rel=1e-12) and snap["eps"] == pytest.approx(1e-2, rel=1e-12)
    assert post.kernel_fn.w_std == pytest.approx(1.1, rel=1e-12)
    later = model.posterior(capacity=8)
    assert later.hyper["w_std"] == pytest.approx(2.5, rel=1e-12)
    # close is idempotent and destroys the state once
    post.close()
    post.close()
    assert [c[0] for c in ctx.calls].count("smn_fit_destroy") == 1
    with later:
        pass
    assert [c[0] for c in ctx.calls].count("smn_fit_destroy") == 2
    with pytest.raises(ValueError, match="closed"):
        post.predict(np.zeros((3, 4), np.float32))


def test_predict_fn_keeps_its_signature_and_its_positional_learning_rate(lib):
    """`cache` is a keyword and nothing else about the factory's calling convention moves: the five leading parameters,
    `learning_rate` with its default as the signature's last entry (tests/test_gd_host.py pins that), and a sixth POSITIONAL
    argument still being learning_rate, as on every earlier version of the factory."""
    import inspect
    from smnngp import nt_kernels, predict
    sig = inspect.signature(predict.gradient_descent_mse_ensemble)
    P = inspect.Parameter
    assert list(sig.parameters)[:5] == ["kernel_fn", "x_train", "y_train", "diag_reg", "diag_reg_absolute_scale"]
    assert all(sig.parameters[k].kind is P.POSITIONAL_OR_KEYWORD for k in list(sig.parameters)[:5])
    assert sig.parameters["cache"].default is False and sig.parameters["cache"].kind is P.KEYWORD_ONLY
    assert sig.parameters["cache_capacity"].default == 2048 and sig.parameters["cache_capacity"].kind is P.KEYWORD_ONLY
    assert list(sig.parameters)[-1] == "learning_rate" and sig.parameters["learning_rate"].default == 1.0
    assert sig.parameters["diag_reg"].default == 0.0 and sig.parameters["diag_reg_absolute_scale"].default is False
    # the calls themselves, on the stand-in context: the factory only uploads x and y
    kfn = nt_kernels.get_mlp_kernel(1)
    kfn.ctx = StubContext()
    x, y = np.zeros((4, 3)), np.zeros(4)

    def rate(fn):                                                  # the learning_rate the returned predict_fn's t=... branch closes over
        cells = dict(zip(fn.__code__.co_freevars, (c.cell_contents for c in fn.__closure__)))
        return cells["learning_rate"] if "learning_rate" in cells else rate(cells["_predict_gd"])
    make = predict.gradient_descent_mse_ensemble
    assert rate(make(kfn, x, y)) == 1.0
    assert rate(make(kfn, x, y, 0.0, False, 2.0)) == 2.0           # sixth positional argument
    assert rate(make(kfn, x, y, 0.0, False, learning_rate=2.5)) == 2.5
    assert rate(make(kfn, x, y, 1e-3, cache=True, learning_rate=0.5)) == 0.5
    with pytest.raises(TypeError):
        make(kfn, x, y, 0.0, False, 2.0, True)                     # a seventh positional argument: cache is keyword-only
    with pytest.raises(TypeError):
        make(kfn, x, y, 0.0, False, 2.0, learning_rate=3.0)        # both
