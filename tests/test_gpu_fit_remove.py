"""GPU tests of removing training points from a fitted posterior: FittedPosterior.remove and the smn_fit_remove entry
(csrc/fit_remove.hip) against the fp64 rules of _fit_append_rules.py / _fit_remove_rules.py.

The reference of a state after a removal is the oracle's one-shot posterior of the KEPT points at the ABSOLUTE ridge the state
froze at creation (post.ridge); the tolerances are the project's own for a fitted state against the oracle (_fit_append_rules.TOL:
relerr_norm < 1e-7 in fp64 at the relative ridge 1e-3, < 1e-2 in fp32 at 1e-2), no wider ones for the removal.  Shapes: n0 = 130
and 260 cross the 128-row tile, the sweep's 64-row block and, with range(0, n0, 7) and a set of KMAX + 1 rows, the 32 rows of
one pass.  Each case of the first test prints the worst error of the state after the removal and of a fresh device fit on the kept
points (profiles/r23_fit_remove.txt).

The undo test asks for the same BITS after append + remove of the appended rows.  The read-out's sums run over the padded row, so
that can only hold when the append does not grow the state: the 120-point state of that test is made with room for 256 points;
the states that do grow (120 and 128 points without a reservation) are compared to TOL."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import nngp_oracle as O  # noqa: E402  (test infrastructure only)
from _tol import relerr_norm  # noqa: E402

import _fit_append_rules as R  # noqa: E402
import _fit_remove_rules as RR  # noqa: E402
import _input_grad_rules as IR  # noqa: E402
from test_gpu_fit_append import _grad_check, make, worst_error  # noqa: E402  (the append tests' own readings and bounds)

TOL, RIDGE, W, B, LW, T = R.TOL, R.RIDGE, R.W, R.B, R.LW, R.T
CASES = [(n0, name) for n0 in (130, 260) for name in RR.index_sets(n0)]


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


def bits(outs):
    return [a.raw_numpy().view(np.uint8) for a in outs]


def kept_reference(net, kind, n, c, d, f32, keep, lam):
    """The one-shot posterior of the points `keep` of the n-point data set at the absolute ridge lam."""
    ref = R.reference(net, kind, n, n, c, d, f32)
    y = R.data(n, c, d, f32)[2]
    return R.one_shot(ref["kdd"][np.ix_(keep, keep)], ref["ktd"][:, keep], ref["ktt"], y[keep], lam)


# ----------------------------------------------------------------------------- 1. removal == the one-shot posterior of the kept points
@pytest.mark.parametrize("d", [6, 40])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("n0,name", CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("net,kind", [("mlp", "nngp"), ("mlp", "ntk"), ("resnet", "nngp")])
def test_removal_equals_the_one_shot_posterior_of_the_kept_points(ctx, net, kind, dtype, n0, name, c, d):
    idx, cap, f32, tol = RR.index_sets(n0)[name], 64, dtype == np.float32, TOL[dtype]
    keep = np.setdiff1d(np.arange(n0), idx)
    x, xt, y = R.data(n0, c, d, f32)
    what = "%s %s %s n0=%d -%s(%d) c=%d d=%d" % (net, kind, np.dtype(dtype).name, n0, name, len(idx), c, d)
    with make(ctx, net, kind, dtype, x, y, cap, ridge_rel=RIDGE[dtype]) as post:
        lam, room, nbytes = post.ridge, post.max_points, post.nbytes
        post.predict(xt), post.predict(xt[:cap], cov="full")   # (leave a prediction's columns behind the new n in the test rows)
        assert post.remove(idx) is post
        assert post.num_data == keep.size and tuple(post.x_train.shape) == (keep.size, d)
        assert np.array_equal(post.x_train.raw_numpy(), x[keep].astype(dtype))
        assert post.ridge == lam and post.max_points == room and post.nbytes == nbytes
        ref = kept_reference(net, kind, n0, c, d, f32, keep, lam)
        e_rem = worst_error(post, ref, xt, tol, what + " removed")
    with make(ctx, net, kind, dtype, x[keep], y[keep], cap, ridge_rel=0.0, ridge_abs=lam) as fresh:
        mean, var = (a.raw_numpy().astype(np.float64) for a in fresh.predict(xt))      # for the record, not asserted
        e_fresh = max(relerr_norm(mean, ref["mean"]), np.abs(var - np.diag(ref["cov"])).max() / np.abs(ref["cov"]).max(),
                      float(np.max(np.abs(fresh.quad - ref["quad"]) / np.abs(ref["quad"]))),
                      abs(fresh.logdet - ref["logdet"]) / abs(ref["logdet"]))
    print("%s: worst error removed %.3e fresh %.3e" % (what, e_rem, e_fresh))


# ----------------------------------------------------------------------------- 2. undo
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_removing_the_appended_rows_undoes_the_append_bit_for_bit(ctx, dtype):
    n0, k, c, d, cap = 120, 20, 3, 6, 32
    x, xt, y = R.data(n0 + k, c, d, dtype == np.float32)
    with make(ctx, "mlp", "nngp", dtype, x[:n0], y[:n0], cap, ridge_rel=RIDGE[dtype], reserve=256) as post:
        before, before_full = bits(post.predict(xt)), bits(post.predict(xt[:cap], cov="full"))
        quad, logdet, room, nbytes = post.quad.copy(), post.logdet, post.max_points, post.nbytes
        post.append(x[n0:], y[n0:])
        assert post.num_data == n0 + k and post.max_points == room
        post.remove(range(n0, n0 + k))
        assert post.num_data == n0 and post.max_points == room and post.nbytes == nbytes
        assert all(np.array_equal(a, b) for a, b in zip(before, bits(post.predict(xt))))
        assert all(np.array_equal(a, b) for a, b in zip(before_full, bits(post.predict(xt[:cap], cov="full"))))
        qerr, lerr = float(np.max(np.abs(post.quad - quad) / np.abs(quad))), abs(post.logdet - logdet) / abs(logdet)
        print("undo %s: quad %.3e logdet %.3e (relative, against the totals of the creation)" % (np.dtype(dtype).name, qerr, lerr))
        if dtype == np.float64:
            # the recomputed totals are the same <= 140 terms in another order: 3e-14 for quad, < 1e-12 for logdet.  (An fp32 state's
            # creation forms y^T K~^-1 y in fp32 arithmetic; the recomputation sums the same beta in fp64: they agree to fp32.)
            assert qerr <= 1e-12 and lerr <= 1e-12
        else:
            assert qerr <= TOL[dtype] and lerr <= TOL[dtype]
        assert np.array_equal(post.x_train.raw_numpy(), x[:n0].astype(dtype))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n0", [120, 128])
def test_undo_across_a_growth_agrees_to_tolerance(ctx, n0, dtype):
    k, c, d, cap, f32, tol = 20, 3, 6, 32, dtype == np.float32, TOL[dtype]
    x, xt, y = R.data(n0 + k, c, d, f32)
    with make(ctx, "mlp", "nngp", dtype, x[:n0], y[:n0], cap, ridge_rel=RIDGE[dtype]) as post:
        (mean, var), cov = (a.raw_numpy() for a in post.predict(xt)), post.predict(xt[:cap], cov="full")[1].raw_numpy()
        quad, logdet = post.quad.copy(), post.logdet
        post.append(x[n0:], y[n0:])
        assert post.max_points == 256                                      # the append grew the state
        post.remove(range(n0, n0 + k))
        assert post.num_data == n0 and post.max_points == 256
        (mean2, var2), cov2 = (a.raw_numpy() for a in post.predict(xt)), post.predict(xt[:cap], cov="full")[1].raw_numpy()
        scale = np.abs(cov).max()
        assert relerr_norm(mean2, mean) < tol and np.abs(var2 - var).max() / scale < tol and relerr_norm(cov2, cov) < tol
        assert np.max(np.abs(post.quad - quad) / np.abs(quad)) <= tol and abs(post.logdet - logdet) <= tol * abs(logdet)


# ----------------------------------------------------------------------------- 3. order does not matter
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_removed_points_appended_back_give_the_posterior_of_the_original_set(ctx, dtype):
    n0, c, d, cap, f32 = 150, 3, 6, 64, dtype == np.float32
    x, xt, y = R.data(n0, c, d, f32)
    idx = [2, 17, 40, 63, 64, 90, 127, 128, 140, 149]
    with make(ctx, "mlp", "nngp", dtype, x, y, cap, ridge_rel=RIDGE[dtype]) as post:
        lam = post.ridge
        ref = kept_reference("mlp", "nngp", n0, c, d, f32, np.arange(n0), lam)
        post.remove(idx).append(x[idx].astype(dtype), y[idx])
        assert post.num_data == n0 and post.ridge == lam
        order = np.concatenate([np.setdiff1d(np.arange(n0), idx), idx])
        assert np.array_equal(post.x_train.raw_numpy(), x[order].astype(dtype))
        worst_error(post, ref, xt, TOL[dtype], "removed 10, appended back %s" % np.dtype(dtype).name)


# ----------------------------------------------------------------------------- 4. sliding window
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_sliding_window(ctx, dtype):
    n0, k, steps, c, d, cap, f32 = 140, 5, 6, 3, 6, 64, dtype == np.float32
    n = n0 + k * steps
    x, xt, y = R.data(n, c, d, f32)
    with make(ctx, "mlp", "nngp", dtype, x[:n0], y[:n0], cap, ridge_rel=RIDGE[dtype]) as post:
        lam, room, nbytes = post.ridge, post.max_points, post.nbytes
        for s in range(steps):
            at = n0 + k * s
            post.remove(range(k)).append(x[at:at + k].astype(dtype), y[at:at + k])
            assert post.num_data == n0 and post.max_points == room and post.nbytes == nbytes
        last = np.arange(n - n0, n)
        full = R.reference("mlp", "nngp", n, n, c, d, f32)
        ref = R.one_shot(full["kdd"][np.ix_(last, last)], full["ktd"][:, last], full["ktt"], y[last], lam)
        assert np.array_equal(post.x_train.raw_numpy(), x[last].astype(dtype))
        worst_error(post, ref, xt, TOL[dtype], "window of %d after %d steps of %d %s" % (n0, steps, k, np.dtype(dtype).name))


# ----------------------------------------------------------------------------- 5. same bits
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_same_sequence_same_bits(ctx, dtype):
    n0, c, d = 260, 3, 6
    x, xt, y = R.data(n0 + 10, c, d, dtype == np.float32)
    outs = []
    for _ in range(2):
        with make(ctx, "mlp", "nngp", dtype, x[:n0], y[:n0], 32, ridge_rel=RIDGE[dtype]) as post:
            post.remove(list(range(0, n0, 7)))                              # two passes
            post.append(x[n0:], y[n0:])
            post.remove([1, 128, -1])
            mean, var = (a.raw_numpy() for a in post.predict(xt))
            cov = post.predict(xt[:32], cov="full")[1].raw_numpy()
            outs.append((mean, var, cov, post.quad.copy(), post.logdet))
    for a, b in zip(*outs):
        assert np.array_equal(np.atleast_1d(a).view(np.uint8), np.atleast_1d(b).view(np.uint8))


# ----------------------------------------------------------------------------- 6. predict_grad across a removal
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("net,kind", [("mlp", "nngp"), ("resnet", "ntk")])
def test_predict_grad_across_a_removal(ctx, net, kind, dtype):
    n0, c, d, f32 = 140, 3, 6, dtype == np.float32
    idx = [0, 30, 64, 65, 127, 128, 139]
    keep = np.setdiff1d(np.arange(n0), idx)
    x, xt, y = R.data(n0, c, d, f32)
    hyp = dict(num_hiddens=R.DEPTH[net], act="relu", w_std=W, b_std=B, last_w_std=LW)
    with make(ctx, net, kind, dtype, x, y, 16, ridge_rel=RIDGE[dtype]) as post:
        lam = post.ridge
        first = post.predict_grad(xt)                          # builds L', alpha, X^T at n0
        assert np.isfinite(first[0].raw_numpy()).all()
        post.remove(idx)
        dmean, dvar = (a.raw_numpy() for a in post.predict_grad(xt))
    with make(ctx, net, kind, dtype, x[keep], y[keep], 16, ridge_rel=0.0, ridge_abs=lam) as fresh:
        fmean, fvar = (a.raw_numpy() for a in fresh.predict_grad(xt))
    m64, v64 = IR.predict_grad(net, x[keep], y[keep], xt, kind, diag_reg=lam, absolute=True, **hyp)
    m32, v32 = IR.predict_grad(net, x[keep], y[keep], xt, kind, diag_reg=lam, absolute=True, dtype=np.float32, **hyp) if f32 else (None, None)
    what = "predict_grad %s %s n0=%d-%d" % (net, kind, n0, len(idx))
    for name, got, r64, r32 in (("removed dmean", dmean, m64, m32), ("removed dvar", dvar, v64, v32),
                                ("fresh dmean", fmean, m64, m32), ("fresh dvar", fvar, v64, v32)):
        _grad_check("%s %s" % (what, name), got, r64, r32, dtype)


# ----------------------------------------------------------------------------- 7. Student-t and MultiSPR on constant-diagonal data
def _models(method, multi, dtype, n, keep):
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood
    from smnngp.spax.models import SPR, MultiSPR
    rng = np.random.default_rng(78)
    d, c = 6, 3
    x = R.constant_norm_rows(rng.standard_normal((n, d))).astype(dtype)
    xt = R.constant_norm_rows(rng.standard_normal((T, d))).astype(dtype)
    kernel = lambda: NNGPKernel(lambda w, b, l: nt_kernels.get_mlp_kernel(R.LAYERS, 1, act="relu", w_std=w, b_std=b, last_w_std=l),   # noqa: E731
                                W, B, LW)
    lik = lambda: GaussianLikelihood() if method == "gp" else StudentTLikelihood(1.7, 2.4)   # noqa: E731
    eps = RIDGE[dtype]
    if multi:
        labels, yt = rng.integers(0, c, n), MultiSPR.label_targets(rng.integers(0, c, T), c)
        whole = MultiSPR.from_labels(kernel(), lik(), x, labels, c, 0.3, 1.7, eps=eps)
        kept = MultiSPR.from_labels(kernel(), lik(), x[keep], labels[keep], c, 0.3, 1.7, eps=eps)
        return whole, kept, xt, yt
    y, yt = rng.standard_normal(n), rng.standard_normal(T)
    return SPR(kernel(), lik(), x, y, 0.3, 1.7, eps=eps), SPR(kernel(), lik(), x[keep], y[keep], 0.3, 1.7, eps=eps), xt, yt


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("method", ["gp", "tp"])
def test_constant_diagonal_removal_equals_the_model_on_the_kept_data(ctx, method, multi, dtype):
    n, tol = 150, TOL[dtype]
    idx = [0, 3, 64, 100, 127, 128, 129, 149]
    keep = np.setdiff1d(np.arange(n), idx)
    whole, kept, xt, yt = _models(method, multi, dtype, n, keep)
    with whole.posterior(capacity=32) as post, kept.posterior(capacity=32) as fitted:
        stale_before = post.student_quad
        mask = np.zeros(n, dtype=bool)
        mask[idx] = True
        post.remove(mask)
        assert post.num_data == keep.size and abs(post.ridge - fitted.ridge) <= tol * post.ridge
        got, own, fit = post.test_nll(xt, yt), kept.test_nll(xt, yt), fitted.test_nll(xt, yt)
        print("%s multi=%s %s: removed %.9g  model %.9g  model.posterior %.9g" % (method, multi, np.dtype(dtype).name, got, own, fit))
        assert abs(got - own) <= tol * abs(own) and abs(got - fit) <= tol * abs(fit)
        if method == "tp":
            df_post, shape = post.predictive_params()
            assert df_post == 2 * 1.7 + keep.size * (3 if multi else 1)             # the degrees of freedom of the new N
            assert post.student_quad != stale_before
            assert abs(post.student_quad - fitted.student_quad) <= 1e-9 * abs(fitted.student_quad)
            assert abs(shape - kept.predictive_params()[1]) <= 1e-9 * abs(shape)
        if multi:
            assert np.array_equal(post.classify(xt), kept.classify(xt))


# ----------------------------------------------------------------------------- 8. matrix form
def test_matrix_form_removes_from_conv_kernels(ctx):
    from smnngp import nt_kernels
    from smnngp.posterior import FittedPosterior
    rng = np.random.default_rng(12)
    n, t, c, img, idx = 40, 5, 2, (5, 4, 3), [0, 17, 39]
    keep = np.setdiff1d(np.arange(n), idx)
    x, xt, y = rng.standard_normal((n,) + img), rng.standard_normal((t,) + img), rng.standard_normal((n, c))
    args = (2, "relu", W, B, LW)
    kdd, ktd, ktt = O.cnn_kernel(x, None, *args), O.cnn_kernel(xt, x, *args), O.cnn_kernel(xt, None, *args)
    fn = nt_kernels.get_cnn_kernel(2, 1, act="relu", w_std=W, b_std=B, last_w_std=LW)
    with FittedPosterior(fn, ctx.to_device(x), ctx.to_device(y), ridge_rel=1e-3, capacity=3, ctx=ctx) as post:
        lam = post.ridge
        assert abs(lam - R.frozen_ridge(kdd, 1e-3)) <= 1e-7 * lam
        post.remove(idx)
        assert post.num_data == n - 3 and tuple(post.x_train.shape) == (n - 3,) + img
        assert np.array_equal(post.x_train.raw_numpy(), x[keep])
        ref = R.one_shot(kdd[np.ix_(keep, keep)], ktd[:, keep], ktt, y[keep], lam)
        mean, var = (a.raw_numpy() for a in post.predict(xt))
        assert relerr_norm(mean, ref["mean"]) < 1e-7
        assert np.abs(var - np.diag(ref["cov"])).max() / np.abs(ref["cov"]).max() < 1e-7
        mean3, cov3 = (a.raw_numpy() for a in post.predict(xt[:3], cov="full"))
        assert relerr_norm(cov3, ref["cov"][:3, :3]) < 1e-7
        assert np.allclose(post.quad, ref["quad"], rtol=1e-7, atol=0.0) and abs(post.logdet - ref["logdet"]) <= 1e-7 * abs(ref["logdet"])
    with FittedPosterior(fn, ctx.to_device(x[keep]), ctx.to_device(y[keep]), ridge_rel=0.0, ridge_abs=lam, capacity=3, ctx=ctx) as fresh:
        fmean, fvar = (a.raw_numpy() for a in fresh.predict(xt))
        assert relerr_norm(fmean, ref["mean"]) < 1e-7 and relerr_norm(mean, fmean) < 1e-7
        assert np.abs(fvar - var).max() / np.abs(ref["cov"]).max() < 1e-7


# ----------------------------------------------------------------------------- 9. refusals through the C ABI
def _last_error(L, ctx):
    buf = C.create_string_buffer(512)
    L._lib.smn_last_error(ctx.handle, buf, 512)
    return buf.value.decode()


def test_refusals_name_the_value_and_move_nothing(L, ctx):
    n, c, d, t = 20, 2, 6, 7
    x, xt, y = R.data(n, c, d, False)
    xd, yd, xtd = ctx.to_device(x), ctx.to_device(y), ctx.to_device(xt[:t])
    quad, logdet, info = (C.c_double * c)(), C.c_double(), C.c_int()
    good, bad = C.c_void_p(), C.c_void_p()
    ctx.call("smn_fit_create", L.F64, 0, L.ACT["relu"], 1, W, B, LW, xd.ptr, n, d, d, yd.ptr, c, 1e-3, 0.0, 8, C.byref(good), None, None, None)
    ctx.call("smn_fit_create", L.F64, 0, L.ACT["relu"], 1, W, B, LW, xd.ptr, n, d, d, yd.ptr, c, 0.0, -50.0, 8, C.byref(bad), None, None, C.byref(info))
    assert info.value > 0
    rem = L._lib.smn_fit_remove
    arr = lambda *v: (C.c_int64 * len(v))(*v)   # noqa: E731

    def predict():
        mean, var, cov = ctx.empty((t, c), np.float64), ctx.empty((t,), np.float64), ctx.empty((t, t), np.float64)
        ctx.call_on("smn_fit_predict", good, xtd.ptr, t, d, mean.ptr, var.ptr, cov.ptr, t)
        return bits((mean, var, cov))

    try:
        before = predict()
        for call, word in (
                (lambda: rem(good, arr(0), 0, quad, C.byref(logdet)), "k = 0"),
                (lambda: rem(good, arr(*range(n)), n, quad, C.byref(logdet)), "k = 20"),
                (lambda: rem(good, arr(3, -1), 2, quad, C.byref(logdet)), "index -1"),
                (lambda: rem(good, arr(3, n), 2, quad, C.byref(logdet)), "index 20"),
                (lambda: rem(good, arr(5, 3, 5), 3, quad, C.byref(logdet)), "index 5 is given twice"),
                (lambda: rem(good, None, 2, quad, C.byref(logdet)), "idx_h"),
                (lambda: rem(bad, arr(3), 1, quad, C.byref(logdet)), "info = "),
        ):
            assert call() == L.EINVAL and word in _last_error(L, ctx), (word, _last_error(L, ctx))
            nn = C.c_int64()
            ctx.call_on("smn_fit_info", good, C.byref(nn), None, None, None)
            assert nn.value == n
            assert all(np.array_equal(a, b) for a, b in zip(before, predict())), word
        assert rem(None, arr(3), 1, None, None) == L.EINVAL
        assert rem(good, arr(19, 0), 2, None, None) == L.OK                 # NULL outputs are allowed; any order
        nn = C.c_int64()
        ctx.call_on("smn_fit_info", good, C.byref(nn), None, None, None)
        assert nn.value == n - 2
        assert rem(good, arr(4), 1, quad, C.byref(logdet)) == L.OK
        q2, l2 = (C.c_double * c)(), C.c_double()
        assert L._lib.smn_fit_stats(good, None, None, q2, C.byref(l2)) == L.OK and list(q2) == list(quad) and l2.value == logdet.value
    finally:
        for h in (good, bad):
            ctx.call_on("smn_fit_destroy", h)
