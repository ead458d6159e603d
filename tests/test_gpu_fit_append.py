"""GPU tests of appending training points to a fitted posterior: FittedPosterior.append / reserve and the smn_fit_reserve,
smn_fit_append, smn_fit_append_from_kernel, smn_fit_stats entries (csrc/fit.hip) against the fp64 rules of
_fit_append_rules.py.

The reference of an appended state is the oracle's one-shot posterior of ALL the points at the ABSOLUTE ridge the state froze
at creation (post.ridge); the tolerance is the one test_gpu_fit.py allows a fresh state against the oracle (relerr_norm < 1e-7
in fp64 at the relative ridge 1e-3, < 1e-2 in fp32 at 1e-2; var against diag(cov) normalised by max|cov|).  Shapes: the
smallest at which the layout can go wrong (the table of APPEND_SHAPES), d = 6 and 40 (below and above the 16 / 32-element
padding of the feature dimension).  Each case prints the worst error of the appended state and of the fresh one
(profiles/r22_fit_append.txt)."""
import ctypes as C
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import nngp_oracle as O  # noqa: E402  (test infrastructure only)
from _tol import relerr_norm  # noqa: E402

import _fit_append_rules as R  # noqa: E402
import _input_grad_rules as IR  # noqa: E402

TOL, RIDGE, W, B, LW, T = R.TOL, R.RIDGE, R.W, R.B, R.LW, R.T
# (n0, appends, capacity): same tile | crosses 128 and forces growth | exact tile boundary, k = 1 | three chunks, crosses 256 |
# three calls
APPEND_SHAPES = [(70, (5,), 16), (120, (20,), 64), (128, (1,), 16), (250, (140,), 64), (70, (5, 60, 1), 64)]


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


def kernel_fn(net):
    from smnngp import nt_kernels
    fac = nt_kernels.get_mlp_kernel if net == "mlp" else nt_kernels.get_dense_resnet_kernel
    return fac(R.DEPTH[net], 1, act="relu", w_std=W, b_std=B, last_w_std=LW)


def make(ctx, net, kind, dtype, x, y, cap, **ridge):
    from smnngp.posterior import FittedPosterior
    dev = lambda a: ctx.to_device(np.ascontiguousarray(a, dtype=dtype))   # noqa: E731
    return FittedPosterior(kernel_fn(net), dev(x), dev(y), capacity=cap, mode=kind, ctx=ctx, **ridge)


def worst_error(post, ref, xt, tol, what):
    """The largest of the test_gpu_fit.py error readings of `post` against the one-shot rules `ref`; asserts each."""
    scale = np.abs(ref["cov"]).max()
    mean, var = (a.raw_numpy() for a in post.predict(xt))
    tf = min(xt.shape[0], post.capacity)
    mean_f, cov = (a.raw_numpy() for a in post.predict(xt[:tf], cov="full"))
    errs = dict(mean=relerr_norm(mean, ref["mean"]), var=np.abs(var.astype(np.float64) - np.diag(ref["cov"])).max() / scale,
                cov=relerr_norm(cov, ref["cov"][:tf, :tf]), mean_full=relerr_norm(mean_f, ref["mean"][:tf]),
                quad=float(np.max(np.abs(post.quad - ref["quad"]) / np.abs(ref["quad"]))),
                logdet=abs(post.logdet - ref["logdet"]) / abs(ref["logdet"]))
    print("%s: %s" % (what, "  ".join("%s %.3e" % kv for kv in errs.items())))
    assert post.info == 0
    for name, err in errs.items():
        assert err < tol if name != "logdet" and name != "quad" else err <= tol, (what, name, err)
    assert np.array_equal(cov, cov.T)
    return max(errs.values())


# ----------------------------------------------------------------------------- 1. append == the fresh fit at the frozen ridge
@pytest.mark.parametrize("d", [6, 40])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("shape", APPEND_SHAPES, ids=lambda s: "n%d+%s_cap%d" % (s[0], "+".join(map(str, s[1])), s[2]))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["nngp", "ntk"])
@pytest.mark.parametrize("net", ["mlp", "resnet"])
def test_append_equals_the_fresh_fit_with_the_frozen_ridge(ctx, net, kind, dtype, shape, c, d):
    n0, steps, cap = shape
    n, f32, tol = n0 + sum(steps), dtype == np.float32, TOL[dtype]
    x, xt, y = R.data(n, c, d, f32)
    kdd, ktd, ktt = (R.reference(net, kind, n0, n, c, d, f32)[k] for k in ("kdd", "ktd", "ktt"))
    with make(ctx, net, kind, dtype, x[:n0], y[:n0], cap, ridge_rel=RIDGE[dtype]) as post:
        lam = post.ridge
        assert abs(lam - R.frozen_ridge(kdd[:n0, :n0], RIDGE[dtype])) <= tol * lam
        assert post.max_points == -(-n0 // 128) * 128 and post.num_data == n0
        ref = R.one_shot(kdd, ktd, ktt, y, lam)
        at = n0
        for k in steps:
            assert post.append(x[at:at + k].astype(dtype), y[at:at + k]) is post
            at += k
            assert post.num_data == at and post.max_points >= at and post.max_points % 128 == 0
        assert post.ridge == lam
        what = "%s %s %s n0=%d +%s cap=%d c=%d d=%d" % (net, kind, np.dtype(dtype).name, n0, steps, cap, c, d)
        e_app = worst_error(post, ref, xt, tol, what + " appended")
    with make(ctx, net, kind, dtype, x, y, cap, ridge_rel=0.0, ridge_abs=lam) as fresh:
        assert fresh.ridge == lam
        e_fresh = worst_error(fresh, ref, xt, tol, what + " fresh   ")
    print("%s: worst error appended %.3e fresh %.3e" % (what, e_app, e_fresh))


@pytest.mark.parametrize("family,img,layers", [("cnn", (5, 4, 3), 2), ("conv_resnet", (8, 8, 1), 1)])
def test_matrix_form_appends_conv_kernels(ctx, family, img, layers):
    from smnngp import nt_kernels
    from smnngp.posterior import FittedPosterior
    rng = np.random.default_rng(11)
    n0, k, t, c = 10, 4, 5, 2
    x, xt, y = rng.standard_normal((n0 + k,) + img), rng.standard_normal((t,) + img), rng.standard_normal((n0 + k, c))
    fac = nt_kernels.get_cnn_kernel if family == "cnn" else nt_kernels.get_conv_resnet_kernel
    ofn = O.cnn_kernel if family == "cnn" else O.conv_resnet_kernel
    args = (layers, "relu", W, B, LW)
    kdd, ktd, ktt = ofn(x, None, *args), ofn(xt, x, *args), ofn(xt, None, *args)
    fn = fac(layers, 1, act="relu", w_std=W, b_std=B, last_w_std=LW)
    with FittedPosterior(fn, ctx.to_device(x[:n0]), ctx.to_device(y[:n0]), ridge_rel=1e-3, capacity=3, ctx=ctx) as post:
        lam = post.ridge
        assert abs(lam - R.frozen_ridge(kdd[:n0, :n0], 1e-3)) <= 1e-7 * lam
        post.append(x[n0:], y[n0:])                            # two chunks of the host loop: 3 + 1
        assert post.num_data == n0 + k and tuple(post.x_train.shape) == (n0 + k,) + img
        ref = R.one_shot(kdd, ktd, ktt, y, lam)
        mean, var = (a.raw_numpy() for a in post.predict(xt))
        assert relerr_norm(mean, ref["mean"]) < 1e-7
        assert np.abs(var - np.diag(ref["cov"])).max() / np.abs(ref["cov"]).max() < 1e-7
        mean3, cov3 = (a.raw_numpy() for a in post.predict(xt[:3], cov="full"))
        assert relerr_norm(cov3, ref["cov"][:3, :3]) < 1e-7
        assert np.allclose(post.quad, ref["quad"], rtol=1e-7, atol=0.0) and abs(post.logdet - ref["logdet"]) <= 1e-7 * abs(ref["logdet"])
    with FittedPosterior(fn, ctx.to_device(x), ctx.to_device(y), ridge_rel=0.0, ridge_abs=lam, capacity=3, ctx=ctx) as fresh:
        fmean, fvar = (a.raw_numpy() for a in fresh.predict(xt))
        assert relerr_norm(fmean, ref["mean"]) < 1e-7 and relerr_norm(mean, fmean) < 1e-7
        assert np.abs(fvar - var).max() / np.abs(ref["cov"]).max() < 1e-7


# ----------------------------------------------------------------------------- 2. reserve
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reserve(ctx, dtype):
    n0, steps, c, d, f32, tol = 70, (5, 60), 3, 6, dtype == np.float32, TOL[dtype]
    n = n0 + sum(steps)
    x, xt, y = R.data(n, c, d, f32)
    kdd, ktd, ktt = (R.reference("mlp", "nngp", n0, n, c, d, f32)[k] for k in ("kdd", "ktd", "ktt"))
    bits = lambda outs: [a.raw_numpy().view(np.uint8) for a in outs]   # noqa: E731
    with make(ctx, "mlp", "nngp", dtype, x[:n0], y[:n0], 64, ridge_rel=RIDGE[dtype]) as post, \
            make(ctx, "mlp", "nngp", dtype, x[:n0], y[:n0], 64, ridge_rel=RIDGE[dtype]) as grown:
        lam = post.ridge
        before, before_full, nbytes = bits(post.predict(xt)), bits(post.predict(xt, cov="full")), post.nbytes
        assert post.reserve(100) is post                       # within the room of 128: nothing moves
        assert post.max_points == 128 and post.nbytes == nbytes
        assert all(np.array_equal(a, b) for a, b in zip(before, bits(post.predict(xt))))
        assert all(np.array_equal(a, b) for a, b in zip(before_full, bits(post.predict(xt, cov="full"))))
        post.reserve(300)
        assert post.max_points == 384 and post.nbytes > nbytes and post.num_data == n0
        worst_error(post, R.one_shot(kdd[:n0, :n0], ktd[:, :n0], ktt, y[:n0], lam), xt, tol, "reserved 300, n = 70")
        reserved_bytes, at = post.nbytes, n0
        for k in steps:
            post.append(x[at:at + k], y[at:at + k])
            grown.append(x[at:at + k], y[at:at + k])
            at += k
            assert post.nbytes == reserved_bytes and post.max_points == 384
        assert grown.max_points == 256 and grown.nbytes < reserved_bytes      # 135 > 128: grew to round_up(max(135, 112), 128)
        ref = R.one_shot(kdd, ktd, ktt, y, lam)
        worst_error(post, ref, xt, tol, "reserved, appended")
        worst_error(grown, ref, xt, tol, "auto-grown, appended")
        (m1, v1), (m2, v2) = ([a.raw_numpy() for a in p.predict(xt)] for p in (post, grown))
        assert relerr_norm(m1, m2) < tol and np.abs(v1 - v2).max() / np.abs(ref["cov"]).max() < tol
        with pytest.raises(ValueError, match="below the 135 training points"):
            post.reserve(134)


# ----------------------------------------------------------------------------- 3. constant-diagonal data: the models agree
def _models(method, multi, dtype, n0, n):
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood
    from smnngp.spax.models import SPR, MultiSPR
    rng = np.random.default_rng(77)
    d, c = 6, 3
    x = R.constant_norm_rows(rng.standard_normal((n, d))).astype(dtype)
    xt = R.constant_norm_rows(rng.standard_normal((T, d))).astype(dtype)
    kernel = lambda: NNGPKernel(lambda w, b, l: nt_kernels.get_mlp_kernel(R.LAYERS, 1, act="relu", w_std=w, b_std=b, last_w_std=l),   # noqa: E731
                                W, B, LW)
    lik = lambda: GaussianLikelihood() if method == "gp" else StudentTLikelihood(1.7, 2.4)   # noqa: E731
    eps = RIDGE[dtype]
    if multi:
        labels, yt = rng.integers(0, c, n), MultiSPR.label_targets(rng.integers(0, c, T), c)
        first = MultiSPR.from_labels(kernel(), lik(), x[:n0], labels[:n0], c, 0.3, 1.7, eps=eps)
        whole = MultiSPR.from_labels(kernel(), lik(), x, labels, c, 0.3, 1.7, eps=eps)
        return first, whole, x, labels, xt, yt
    y, yt = rng.standard_normal(n), rng.standard_normal(T)
    return (SPR(kernel(), lik(), x[:n0], y[:n0], 0.3, 1.7, eps=eps), SPR(kernel(), lik(), x, y, 0.3, 1.7, eps=eps), x, y, xt, yt)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("method", ["gp", "tp"])
def test_constant_diagonal_append_equals_the_model_on_all_the_data(ctx, method, multi, dtype):
    n0, n, tol = 40, 150, TOL[dtype]
    first, whole, x, y, xt, yt = _models(method, multi, dtype, n0, n)
    with first.posterior(capacity=32) as post, whole.posterior(capacity=32) as all_at_once:
        stale_before = post.student_quad
        post.append(x[n0:100], y[n0:100]).append(x[100:], y[100:])       # labels for the MultiSPR.from_labels posterior
        assert post.num_data == n and abs(post.ridge - all_at_once.ridge) <= tol * post.ridge
        got, own, fitted = post.test_nll(xt, yt), whole.test_nll(xt, yt), all_at_once.test_nll(xt, yt)
        print("%s multi=%s %s: appended %.9g  model %.9g  model.posterior %.9g" % (method, multi, np.dtype(dtype).name, got, own, fitted))
        assert abs(got - own) <= tol * abs(own) and abs(got - fitted) <= tol * abs(fitted)
        if method == "tp":
            df_post, shape = post.predictive_params()
            assert df_post == 2 * 1.7 + n * (3 if multi else 1)                      # the degrees of freedom of the new N
            assert post.student_quad != stale_before
            assert abs(post.student_quad - all_at_once.student_quad) <= 1e-9 * abs(all_at_once.student_quad)
            assert abs(shape - whole.predictive_params()[1]) <= 1e-9 * abs(shape)
        if multi:
            assert np.array_equal(post.classify(xt), whole.classify(xt))


# ----------------------------------------------------------------------------- 4. predict_grad across an append
GRAD_TOL64, GRAD_FP32_TOL, GRAD_FP32_RATIO = 1e-8, 2e-3, 16.0     # the bound of test_gpu_input_grad.py


def _grad_check(what, got, ref64, ref32, dtype):
    err = relerr_norm(got, ref64)
    if np.dtype(dtype) == np.float64:
        print("%s: fp64 relerr_norm %.3g" % (what, err))
        assert err <= GRAD_TOL64, what
        return
    yard = relerr_norm(ref32, ref64)
    print("%s: fp32 relerr_norm %.3g, yardstick %.3g, ratio %.3g" % (what, err, yard, err / yard))
    assert GRAD_FP32_RATIO * yard <= GRAD_FP32_TOL, "%s: the bound exceeds the fp32 kernel tolerance" % what
    assert err <= GRAD_FP32_RATIO * yard, what


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("net,kind", [("mlp", "nngp"), ("resnet", "ntk")])
@pytest.mark.parametrize("n0,k", [(70, 5), (120, 20)], ids=["same_room", "grows"])
def test_predict_grad_across_an_append(ctx, n0, k, net, kind, dtype):
    c, d, f32, n = 3, 6, dtype == np.float32, n0 + k
    x, xt, y = R.data(n, c, d, f32)
    hyp = dict(num_hiddens=R.DEPTH[net], act="relu", w_std=W, b_std=B, last_w_std=LW)
    with make(ctx, net, kind, dtype, x[:n0], y[:n0], 16, ridge_rel=RIDGE[dtype]) as post:
        lam, room = post.ridge, post.max_points
        first = post.predict_grad(xt)                          # builds L', alpha, X^T at n0
        assert np.isfinite(first[0].raw_numpy()).all()
        post.append(x[n0:], y[n0:])
        assert (post.max_points > room) == (n0 + k > room)
        dmean, dvar = (a.raw_numpy() for a in post.predict_grad(xt))
    with make(ctx, net, kind, dtype, x, y, 16, ridge_rel=0.0, ridge_abs=lam) as fresh:
        fmean, fvar = (a.raw_numpy() for a in fresh.predict_grad(xt))
    m64, v64 = IR.predict_grad(net, x, y, xt, kind, diag_reg=lam, absolute=True, **hyp)
    m32, v32 = IR.predict_grad(net, x, y, xt, kind, diag_reg=lam, absolute=True, dtype=np.float32, **hyp) if f32 else (None, None)
    what = "predict_grad %s %s n0=%d+%d" % (net, kind, n0, k)
    for name, got, r64, r32 in (("appended dmean", dmean, m64, m32), ("appended dvar", dvar, v64, v32),
                                ("fresh dmean", fmean, m64, m32), ("fresh dvar", fvar, v64, v32)):
        _grad_check("%s %s" % (what, name), got, r64, r32, dtype)


# ----------------------------------------------------------------------------- 5. determinism, rows alone
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_same_sequence_same_bits_and_rows_alone_equal_rows_inside(ctx, dtype):
    n0, steps, c, d = 120, (20, 1, 70), 3, 6
    x, xt, y = R.data(n0 + sum(steps), c, d, dtype == np.float32)
    outs = []
    for _ in range(2):
        with make(ctx, "mlp", "nngp", dtype, x[:n0], y[:n0], 32, ridge_rel=RIDGE[dtype]) as post:
            at = n0
            for k in steps:
                post.append(x[at:at + k], y[at:at + k])
                at += k
            mean, var = (a.raw_numpy() for a in post.predict(xt))
            cov = post.predict(xt[:32], cov="full")[1].raw_numpy()
            m, v = (a.raw_numpy() for a in post.predict(xt[3:30]))
            assert np.array_equal(m.view(np.uint8), mean[3:30].view(np.uint8)) and np.array_equal(v.view(np.uint8), var[3:30].view(np.uint8))
            m, v = (a.raw_numpy() for a in post.predict(xt[33:36]))          # rows of the second chunk, alone
            assert np.array_equal(m.view(np.uint8), mean[33:36].view(np.uint8)) and np.array_equal(v.view(np.uint8), var[33:36].view(np.uint8))
            outs.append((mean, var, cov, post.quad.copy(), post.logdet))
    for a, b in zip(*outs):
        assert np.array_equal(np.atleast_1d(a).view(np.uint8), np.atleast_1d(b).view(np.uint8))


# ----------------------------------------------------------------------------- 6. failure leaves the state alone
class HandMadeKernel:
    """A foreign callable (matrix-form posterior): the oracle's MLP kernel, except that K(x+, x+) of the rows in `bad` is
    0.5 V V^T -- the Schur complement of those rows is then -0.5 V V^T, not positive definite."""

    def __init__(self, x_train):
        self.x_train, self.bad = np.asarray(x_train), None

    def __call__(self, x1, x2, mode):
        if x2 is None and self.bad is not None and x1.shape == self.bad.shape and np.array_equal(x1, self.bad):
            k_dd = R.kernel("mlp", "nngp", self.x_train)
            v = np.linalg.solve(np.linalg.cholesky(k_dd), R.kernel("mlp", "nngp", x1, self.x_train).T).T
            return 0.5 * v @ v.T
        return R.kernel("mlp", "nngp", x1, x2)


def _pivot(err):
    m = re.search(r"pivot (\d+)", str(err.value))
    assert m, str(err.value)
    return int(m.group(1))


def test_a_failing_append_leaves_the_state_alone(ctx):
    from smnngp.posterior import FittedPosterior
    n, k, c, d = 25, 3, 2, 6
    x, xt, y = R.data(n + 2 * k, c, d, False)
    bits = lambda outs: [a.raw_numpy().view(np.uint8) for a in outs]   # noqa: E731
    fn = HandMadeKernel(x[:n])
    with FittedPosterior(fn, x[:n], ctx.to_device(y[:n]), capacity=k, ctx=ctx) as post:     # ridge 0
        assert post.ridge == 0.0 and post.info == 0
        before, before_full = bits(post.predict(xt)), bits(post.predict(xt[:k], cov="full"))
        stats = (post.quad.copy(), post.logdet, post.nbytes, post.max_points)
        fn.bad = x[n:n + k]
        with pytest.raises(np.linalg.LinAlgError, match="0 of the 3 new points") as err:
            post.append(x[n:n + k], y[n:n + k])
        assert n < _pivot(err) <= n + k
        assert post.num_data == n and post.x_train.shape[0] == n
        assert np.array_equal(post.quad, stats[0]) and (post.logdet, post.nbytes, post.max_points) == stats[1:]
        assert all(np.array_equal(a, b) for a, b in zip(before, bits(post.predict(xt))))
        assert all(np.array_equal(a, b) for a, b in zip(before_full, bits(post.predict(xt[:k], cov="full"))))
        # two chunks, the second one bad: the first stays in
        fn.x_train, fn.bad = x[:n + k], x[n + k:]
        with pytest.raises(np.linalg.LinAlgError, match="3 of the 6 new points") as err:
            post.append(x[n:], y[n:])
        assert n + k < _pivot(err) <= n + 2 * k
        assert post.num_data == n + k and post.x_train.shape[0] == n + k
        fn.bad = None
        with FittedPosterior(fn, x[:n], ctx.to_device(y[:n]), capacity=k, ctx=ctx) as twin:
            twin.append(x[n:n + k], y[n:n + k])
            assert all(np.array_equal(a, b) for a, b in zip(bits(twin.predict(xt)), bits(post.predict(xt))))
            assert np.array_equal(twin.quad, post.quad) and twin.logdet == post.logdet
        post.append(x[n + k:], y[n + k:])                       # and the state is usable at that size
        kdd, ktd, ktt = R.kernel("mlp", "nngp", x), R.kernel("mlp", "nngp", xt, x), R.kernel("mlp", "nngp", xt)
        ref = R.one_shot(kdd, ktd, ktt, y, 0.0)
        assert post.num_data == n + 2 * k and relerr_norm(post.predict(xt)[0].raw_numpy(), ref["mean"]) < 1e-6


# ----------------------------------------------------------------------------- 7. C ABI edges
def _last_error(L, ctx):
    buf = C.create_string_buffer(512)
    L._lib.smn_last_error(ctx.handle, buf, 512)
    return buf.value.decode()


def test_refusals_name_the_value(L, ctx):
    n, k, c, d = 20, 3, 2, 6
    x, _, y = R.data(n + k, c, d, False)
    xd, yd = ctx.to_device(x), ctx.to_device(y)
    quad, logdet, info = (C.c_double * c)(), C.c_double(), C.c_int()
    outs = (quad, C.byref(logdet), C.byref(info))
    fused, matrix, bad = C.c_void_p(), C.c_void_p(), C.c_void_p()
    kd = ctx.to_device(R.kernel("mlp", "nngp", x))
    ctx.call("smn_fit_create", L.F64, 0, L.ACT["relu"], 1, W, B, LW, xd.ptr, n, d, d, yd.ptr, c, 1e-3, 0.0, 4, C.byref(fused), None, None, None)
    ctx.call("smn_fit_create_from_kernel", L.F64, kd.ptr, n, n + k, yd.ptr, c, 1e-3, 0.0, 4, C.byref(matrix), None, None, None)
    ctx.call("smn_fit_create", L.F64, 0, L.ACT["relu"], 1, W, B, LW, xd.ptr, n, d, d, yd.ptr, c, 0.0, -50.0, 4, C.byref(bad), None, None, C.byref(info))
    assert info.value > 0
    xn, yn = C.c_void_p(xd.ptr.value + 8 * n * d), C.c_void_p(yd.ptr.value + 8 * n * c)
    knd, knn = C.c_void_p(kd.ptr.value + 8 * n * (n + k)), C.c_void_p(kd.ptr.value + 8 * (n * (n + k) + n))
    ld = n + k
    app, appk, res, stats = L._lib.smn_fit_append, L._lib.smn_fit_append_from_kernel, L._lib.smn_fit_reserve, L._lib.smn_fit_stats
    try:
        for rc, code, word in (
                (lambda: app(fused, xn, 0, d, yn, *outs), L.EINVAL, "k = 0"),
                (lambda: app(fused, None, k, d, yn, *outs), L.EINVAL, "x_new_d"),
                (lambda: app(fused, xn, k, d, None, *outs), L.EINVAL, "y_new_d"),
                (lambda: app(fused, xn, k, d - 1, yn, *outs), L.EINVAL, "ldx = 5"),
                (lambda: app(matrix, xn, k, d, yn, *outs), L.EINVAL, "kernel matrix"),
                (lambda: app(bad, xn, k, d, yn, *outs), L.EINVAL, "info = "),
                (lambda: appk(fused, knd, k, n, ld, knn, ld, yn, *outs), L.ENOTSUP, "keeps its own copy of x"),
                (lambda: appk(matrix, knd, 0, n, ld, knn, ld, yn, *outs), L.EINVAL, "k = 0"),
                (lambda: appk(matrix, None, k, n, ld, knn, ld, yn, *outs), L.EINVAL, "k_nd_d"),
                (lambda: appk(matrix, knd, k, n, ld, None, ld, yn, *outs), L.EINVAL, "k_nn_d"),
                (lambda: appk(matrix, knd, k, n, ld, knn, ld, None, *outs), L.EINVAL, "y_new_d"),
                (lambda: appk(matrix, knd, k, n - 1, ld, knn, ld, yn, *outs), L.EINVAL, "n = 19, the state holds 20"),
                (lambda: appk(matrix, knd, k, n, n - 1, knn, ld, yn, *outs), L.EINVAL, "ldk = 19"),
                (lambda: appk(matrix, knd, k, n, ld, knn, k - 1, yn, *outs), L.EINVAL, "ldnn = 2"),
                (lambda: res(fused, n - 1), L.EINVAL, "max_points = 19"),
        ):
            assert rc() == code and word in _last_error(L, ctx), (word, _last_error(L, ctx))
        assert app(None, xn, k, d, yn, *outs) == L.EINVAL and res(None, 10) == L.EINVAL and stats(None, None, None, None, None) == L.EINVAL
        # nothing above changed a state; NULL outputs are allowed; the strided matrix form goes in
        room, lam, nn = C.c_int64(), C.c_double(), C.c_int64()
        for h in (fused, matrix):
            assert stats(h, C.byref(room), C.byref(lam), None, None) == L.OK and room.value == 128 and lam.value > 0.0
            ctx.call_on("smn_fit_info", h, C.byref(nn), None, None, None)
            assert nn.value == n
        assert app(fused, xn, k, d, yn, None, None, None) == L.OK
        assert appk(matrix, knd, k, n, ld, knn, ld, yn, *outs) == L.OK and info.value == 0
        q2 = (C.c_double * c)()
        assert stats(matrix, None, None, q2, None) == L.OK and list(q2) == list(quad)
        for h in (fused, matrix):
            ctx.call_on("smn_fit_info", h, C.byref(nn), None, None, None)
            assert nn.value == n + k
    finally:
        for h in (fused, matrix, bad):
            ctx.call_on("smn_fit_destroy", h)
