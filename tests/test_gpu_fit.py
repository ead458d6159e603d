"""GPU tests of the fitted posterior: the smn_fit_* entries of the C ABI (csrc/fit.hip) and FittedPosterior
(SPR.posterior / MultiSPR.posterior, predict_fn(cache=True)) against the fp64 oracle.

Reference and tolerances are those of test_gpu_parity.py::test_predict_joint_and_fused: relerr_norm < 1e-7 with the relative
ridge 1e-3 in fp64, < 1e-2 with 1e-2 in fp32; var is compared with diag(rcov) and normalised by max|rcov|.  Inputs: d = 6,
standard normal, 2 layers, (w_std, b_std, last_w_std) = (1.1, 0.4, 1.0).  The shapes are the smallest that reach each code path
(one ragged tile; test rows crossing a tile; widest Y with three chunks at capacity 128, the last of one row; a single test row),
each run at capacity 128 and 512.  The first three put x_test[0] = x_train[0]: a posterior variance far below the prior's.

Rows predicted alone against the same rows inside a larger call: measured bit-equal on an MI355X in both dtypes and across a
chunk boundary (the cross build, the solve and the read-out compute a row from that row alone, in an order that depends on
n_pad only), so the test asserts equality of bits; see profiles/r18_fit_predict.txt."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import nngp_oracle as O  # noqa: E402  (test infrastructure only)
from _tol import relerr_norm  # noqa: E402

import _multi_rules as M  # noqa: E402
import _ntk_rules as NT  # noqa: E402

D, LAYERS, W, B, LW = 6, 2, 1.1, 0.4, 1.0
TOL = {np.float64: 1e-7, np.float32: 1e-2}
RIDGE = {np.float64: 1e-3, np.float32: 1e-2}
SHAPES = [(33, 5, 1), (129, 130, 3), (300, 257, 48), (200, 1, 1)]
CAPS = [128, 512]
NETS = {"mlp": 0, "resnet": 1}
OFN = {"mlp": O.mlp_kernel, "resnet": O.dense_resnet_kernel}


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


@functools.lru_cache(maxsize=None)
def data(n, t, c, f32, dup=True):
    """(x, xt, y) as the device will see them, in fp64; dup: x_test[0] = x_train[0]."""
    rng = np.random.default_rng(1000 * n + t)
    dt = np.float32 if f32 else np.float64
    x = rng.standard_normal((n, D)).astype(dt).astype(np.float64)
    xt = rng.standard_normal((t, D)).astype(dt).astype(np.float64)
    y = rng.standard_normal((n, c)).astype(dt).astype(np.float64)
    if dup and t > 1:
        xt[0] = x[0]
    return x, xt, y


@functools.lru_cache(maxsize=None)
def reference(net, act, kind, n, t, c, f32):
    """dict(kdd, ktd, ktt, mean, cov, quad, logdet) of the oracle at the dtype's ridge (kind: "nngp" K, "ntk" Theta)."""
    x, xt, y = data(n, t, c, f32)
    args = (LAYERS, act, W, B, LW, kind)
    kdd, ktd, ktt = OFN[net](x, None, *args), OFN[net](xt, x, *args), OFN[net](xt, None, *args)
    eps = RIDGE[np.float32 if f32 else np.float64]
    mean, cov = O.predict(kdd, ktd, ktt, y, diag_reg=eps)
    kt = kdd + eps * np.trace(kdd) / n * np.eye(n)
    quad = np.array([float(y[:, k] @ np.linalg.solve(kt, y[:, k])) for k in range(c)])
    return dict(kdd=kdd, ktd=ktd, ktt=ktt, mean=mean, cov=cov, quad=quad, logdet=float(np.linalg.slogdet(kt)[1]), eps=eps)


class Fit:
    """A raw smn_fit handle (fused or from a kernel matrix) with numpy-in / numpy-out calls."""

    def __init__(self, L, ctx, dtype, c, capacity, *, x=None, y=None, net=None, act=None, ntk=False, k=None, eps=0.0, ridge_abs=0.0,
                 layers=LAYERS, hyp=(W, B, LW)):
        self.L, self.ctx, self.dtype, self.c = L, ctx, np.dtype(dtype), c
        self.code = L.dtype_code(dtype)
        self.yd = ctx.to_device(np.ascontiguousarray(y, dtype=dtype))
        self.quad_h, self.logdet_h, self.info_h, self.h = (C.c_double * max(c, 1))(), C.c_double(), C.c_int(), C.c_void_p()
        if k is None:
            self.xd = ctx.to_device(np.ascontiguousarray(x, dtype=dtype))
            n, d = self.xd.shape
            netc = NETS[net] | (L.NET_NTK if ntk else 0)
            ctx.call("smn_fit_create", self.code, netc, L.ACT[act], layers, *hyp, self.xd.ptr, n, d, d, self.yd.ptr, c, eps,
                     ridge_abs, capacity, C.byref(self.h), self.quad_h, C.byref(self.logdet_h), C.byref(self.info_h))
        else:
            self.kd = ctx.to_device(np.ascontiguousarray(k, dtype=dtype))
            n = self.kd.shape[0]
            ctx.call("smn_fit_create_from_kernel", self.code, self.kd.ptr, n, n, self.yd.ptr, c, eps, ridge_abs, capacity,
                     C.byref(self.h), self.quad_h, C.byref(self.logdet_h), C.byref(self.info_h))
        self.quad, self.logdet, self.info = np.array(list(self.quad_h))[:c], self.logdet_h.value, self.info_h.value

    def _outs(self, t, want_var, want_cov):
        mean = self.ctx.empty((t, self.c), self.dtype)
        var = self.ctx.empty((t,), self.dtype) if want_var else None
        cov = self.ctx.empty((t, t), self.dtype) if want_cov else None
        return mean, var, cov

    def predict(self, xt, var=True, cov=False):
        xd = self.ctx.to_device(np.ascontiguousarray(xt, dtype=self.dtype))
        t, d = xd.shape
        mean, v, cv = self._outs(t, var, cov)
        self.ctx.call_on("smn_fit_predict", self.h, xd.ptr, t, d, mean.ptr, v.ptr if var else None, cv.ptr if cov else None, t)
        return mean.raw_numpy(), (v.raw_numpy() if var else None), (cv.raw_numpy() if cov else None)

    def apply(self, ktd, ktt_diag=None, ktt=None, var=True, cov=False):
        kd = self.ctx.to_device(np.ascontiguousarray(ktd, dtype=self.dtype))
        t, n = kd.shape
        dg = None if ktt_diag is None else self.ctx.to_device(np.ascontiguousarray(ktt_diag, dtype=self.dtype))
        kt = None if ktt is None else self.ctx.to_device(np.ascontiguousarray(ktt, dtype=self.dtype))
        mean, v, cv = self._outs(t, var, cov)
        self.ctx.call_on("smn_fit_apply", self.h, kd.ptr, t, n, None if dg is None else dg.ptr, None if kt is None else kt.ptr, t,
                         mean.ptr, v.ptr if var else None, cv.ptr if cov else None, t)
        return mean.raw_numpy(), (v.raw_numpy() if var else None), (cv.raw_numpy() if cov else None)

    def nbytes(self):
        n, c, cap, b = C.c_int64(), C.c_int64(), C.c_int64(), C.c_size_t()
        self.ctx.call_on("smn_fit_info", self.h, C.byref(n), C.byref(c), C.byref(cap), C.byref(b))
        return n.value, c.value, cap.value, b.value

    def destroy(self):
        self.ctx.call_on("smn_fit_destroy", self.h)
        self.h = None


def check_against(ref, mean, var, cov, tol):
    scale = np.abs(ref["cov"]).max()
    assert relerr_norm(mean, ref["mean"]) < tol
    if var is not None:
        assert np.abs(var.astype(np.float64) - np.diag(ref["cov"])).max() / scale < tol
    if cov is not None:
        assert relerr_norm(cov, ref["cov"]) < tol
        assert np.array_equal(cov, cov.T)                    # symmetric to the bit, as smn_predict promises


def fused_case(L, ctx, net, act, kind, dtype, shape, cap):
    n, t, c = shape
    f32 = dtype == np.float32
    x, xt, y = data(n, t, c, f32)
    ref = reference(net, act, kind, n, t, c, f32)
    tol = TOL[dtype]
    f = Fit(L, ctx, dtype, c, cap, x=x, y=y, net=net, act=act, ntk=kind == "ntk", eps=ref["eps"])
    try:
        assert f.info == 0
        assert np.allclose(f.quad, ref["quad"], rtol=tol, atol=0.0)
        assert abs(f.logdet - ref["logdet"]) <= tol * abs(ref["logdet"])
        mean, var, cov = f.predict(xt, var=True, cov=t <= cap)
        check_against(ref, mean, var, cov, tol)
        only = f.predict(xt, var=False, cov=False)[0]        # mean alone: the same launches, the same bits
        assert np.array_equal(only, mean)
    finally:
        f.destroy()


# ----------------------------------------------------------------------------- 1. fused form
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["nngp", "ntk"])
@pytest.mark.parametrize("act", ["relu", "erf"])
@pytest.mark.parametrize("net", ["mlp", "resnet"])
def test_fused_form_against_the_oracle(L, ctx, net, act, kind, dtype, shape, cap):
    fused_case(L, ctx, net, act, kind, dtype, shape, cap)


# ----------------------------------------------------------------------------- 2. determinism, rows alone
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape,cap", [((300, 257, 48), 128), ((129, 130, 3), 512)])
def test_same_call_same_bits_and_rows_alone_equal_rows_inside(L, ctx, dtype, shape, cap):
    n, t, c = shape
    x, xt, y = data(n, t, c, dtype == np.float32)
    f = Fit(L, ctx, dtype, c, cap, x=x, y=y, net="mlp", act="relu", eps=RIDGE[dtype])
    try:
        want_cov = t <= cap
        a, b = f.predict(xt, cov=want_cov), f.predict(xt, cov=want_cov)
        for u, v in zip(a, b):
            assert (u is None and v is None) or np.array_equal(u, v)
        lo, hi = 3, 70                                        # inside the first chunk of either capacity, not tile aligned
        m, v, _ = f.predict(xt[lo:hi])
        print("rows alone vs inside (%s): max |d mean| %.3e  max |d var| %.3e"
              % (np.dtype(dtype).name, np.abs(m - a[0][lo:hi]).max(), np.abs(v - a[1][lo:hi]).max()))
        assert np.array_equal(m, a[0][lo:hi]) and np.array_equal(v, a[1][lo:hi])
        # and across a chunk boundary: the rows of the second chunk, asked for alone
        if t > cap:
            m2, v2, _ = f.predict(xt[cap:cap + 40])
            assert np.array_equal(m2, a[0][cap:cap + 40]) and np.array_equal(v2, a[1][cap:cap + 40])
    finally:
        f.destroy()


# ----------------------------------------------------------------------------- 3. against the existing route
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_agrees_with_smn_spr_predict(L, ctx, dtype, shape, cap):
    n, t, c = shape
    f32 = dtype == np.float32
    x, xt, y = data(n, t, c, f32)
    ref = reference("mlp", "relu", "nngp", n, t, c, f32)
    tol, eps = TOL[dtype], RIDGE[dtype]
    xd, xtd, yd = (ctx.to_device(np.ascontiguousarray(a, dtype=dtype)) for a in (x, xt, y))
    mean_d, cov_d = ctx.empty((t, c), dtype), ctx.empty((t, t), dtype)
    quad, logdet, info = (C.c_double * c)(), C.c_double(), C.c_int()
    ctx.call("smn_spr_predict", xd.dcode, 0, L.ACT["relu"], LAYERS, W, B, LW, xd.ptr, n, D, xtd.ptr, t, D, D, yd.ptr, c, eps, 0.0,
             mean_d.ptr, cov_d.ptr, t, quad, C.byref(logdet), C.byref(info))
    old_mean, old_cov = mean_d.raw_numpy(), cov_d.raw_numpy()
    f = Fit(L, ctx, dtype, c, cap, x=x, y=y, net="mlp", act="relu", eps=eps)
    try:
        mean, var, cov = f.predict(xt, cov=t <= cap)
    finally:
        f.destroy()
    scale = np.abs(ref["cov"]).max()
    print("%s n=%d t=%d c=%d cap=%d  mean err: joint %.3e fitted %.3e   var err: joint %.3e fitted %.3e"
          % (np.dtype(dtype).name, n, t, c, cap, relerr_norm(old_mean, ref["mean"]), relerr_norm(mean, ref["mean"]),
             np.abs(np.diag(old_cov) - np.diag(ref["cov"])).max() / scale, np.abs(var - np.diag(ref["cov"])).max() / scale))
    assert np.abs(mean.astype(np.float64) - old_mean).max() / np.abs(ref["mean"]).max() < 2 * tol
    if cov is not None:
        assert np.abs(cov.astype(np.float64) - old_cov).max() / scale < 2 * tol
    assert np.abs(var.astype(np.float64) - np.diag(old_cov)).max() / scale < 2 * tol
    assert np.allclose(f.quad, np.array(list(quad)), rtol=2 * tol, atol=0.0)


# ----------------------------------------------------------------------------- 4. matrix form
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["nngp", "ntk"])
def test_matrix_form_reproduces_the_fused_references(L, ctx, dtype, kind, cap):
    n, t, c = 129, 130, 3
    f32 = dtype == np.float32
    ref = reference("mlp", "relu", kind, n, t, c, f32)
    _, _, y = data(n, t, c, f32)
    tol = TOL[dtype]
    kdd = np.tril(ref["kdd"]).astype(dtype)                 # the lower triangle is all the entry may read
    kdd[np.triu_indices(n, 1)] = np.nan
    f = Fit(L, ctx, dtype, c, cap, k=kdd, y=y, eps=ref["eps"])
    try:
        assert np.array_equal(f.kd.raw_numpy(), kdd, equal_nan=True)            # k_d is not modified
        assert f.info == 0 and np.allclose(f.quad, ref["quad"], rtol=tol, atol=0.0)
        assert abs(f.logdet - ref["logdet"]) <= tol * abs(ref["logdet"])
        diag = np.diag(ref["ktt"]).astype(dtype)
        mean, var, _ = f.apply(ref["ktd"], ktt_diag=diag)
        check_against(ref, mean, var, None, tol)
        ktt_lower = np.tril(ref["ktt"]).astype(dtype)
        mean2, var2, cov2 = f.apply(ref["ktd"], ktt=ktt_lower, cov=t <= cap)
        assert np.array_equal(mean2, mean) and np.array_equal(var2, var)         # diagonal alone == whole K_tt alone
        check_against(ref, mean2, var2, cov2, tol)
        assert np.array_equal(f.kd.raw_numpy(), kdd, equal_nan=True)
    finally:
        f.destroy()


# ----------------------------------------------------------------------------- 5. conv kernels through FittedPosterior
@pytest.mark.parametrize("family,shape,layers", [("cnn", (7, 5, 4, 3), 2), ("conv_resnet", (6, 8, 8, 1), 1)])
def test_conv_posterior_against_the_oracle(ctx, family, shape, layers):
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NNGPKernel
    from smnngp.spax.likelihoods import GaussianLikelihood
    from smnngp.spax.models import MultiSPR
    rng = np.random.default_rng(5)
    n, t, c = shape[0], 4, 2
    x, xt = rng.standard_normal(shape), rng.standard_normal((t,) + shape[1:])
    y = rng.standard_normal((n, c))
    fac = nt_kernels.get_cnn_kernel if family == "cnn" else nt_kernels.get_conv_resnet_kernel
    kernel = NNGPKernel(lambda w, b, l: fac(layers, 1, act="relu", w_std=w, b_std=b, last_w_std=l), W, B, LW)
    model = MultiSPR(kernel, GaussianLikelihood(), x, y, eps=1e-3)
    rmean, rcov = M.predict(family, x, y, xt, layers, "relu", W, B, LW, 1e-3)
    with model.posterior(capacity=3) as post:                # two chunks for the diagonal
        mean, var = post.predict(xt)
        assert relerr_norm(mean.raw_numpy(), rmean) < 1e-7
        assert np.abs(var.raw_numpy() - np.diag(rcov)).max() / np.abs(rcov).max() < 1e-7
        with pytest.raises(ValueError, match="capacity = 3"):
            post.predict(xt, cov="full")
    with model.posterior(capacity=8) as post:
        mean, cov = post.predict(xt, cov="full")
        assert relerr_norm(mean.raw_numpy(), rmean) < 1e-7 and relerr_norm(cov.raw_numpy(), rcov) < 1e-7


# ----------------------------------------------------------------------------- 6. model level
def _model(kind, method, multi, dtype):
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NNGPKernel, NTKKernel
    from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood
    from smnngp.spax.models import SPR, MultiSPR
    n, t, c = 70, 45, (3 if multi else 1)
    # no duplicated point here: test_nll divides by the predictive variance, and at x_test[0] = x_train[0] the ORACLE's cross
    # entry Theta(x, x) comes from the generic formula at correlation 1, which loses half the digits (nngp_oracle._fix_diag:
    # ~1e-6 on Kdot in fp64) -- relative to a variance of 1e-3 that is the reference's error, not the device's.  The
    # norm-wise cases above keep the duplicate.
    x, xt, y = data(n, t, c, dtype == np.float32, False)
    yt = np.random.default_rng(9).standard_normal((t, c))
    kcls = NTKKernel if kind == "ntk" else NNGPKernel
    kernel = kcls(lambda w, b, l: nt_kernels.get_mlp_kernel(LAYERS, 1, act="relu", w_std=w, b_std=b, last_w_std=l), W, B, LW)
    lik = GaussianLikelihood() if method == "gp" else StudentTLikelihood(1.7, 2.4)
    eps = RIDGE[dtype]
    if multi:
        model = MultiSPR(kernel, lik, x.astype(dtype), y, 0.3, 1.7, eps=eps)
    else:
        model = SPR(kernel, lik, x.astype(dtype), y[:, 0], 0.3, 1.7, eps=eps)
    return model, x, y, xt, yt


def _ref_nll(kind, method, x, y, xt, yt, eps, y_mean, y_std):
    """test_nll of SPR / MultiSPR in fp64: O.spr_test_nll / _multi_rules.predictive_nll for K; for Theta the same head on
    _ntk_rules.predict (d from Theta WITHOUT eps, as the NNGP head has K)."""
    c = y.shape[1]
    if kind == "nngp" and c == 1:
        return O.spr_test_nll(x, y[:, 0], xt, yt[:, 0], y_mean, y_std, kernel="mlp", num_hiddens=LAYERS, act="relu", w_std=W,
                              b_std=B, last_w_std=LW, eps=eps, method=method, alpha=1.7, beta=2.4)
    if kind == "nngp":
        return M.predictive_nll("mlp", x, y, xt, yt, LAYERS, "relu", method, W, B, LW, eps, 1.7, 2.4, y_mean, y_std)
    n = x.shape[0]
    mean, cov = NT.predict("mlp", x, y, xt, LAYERS, "relu", W, B, LW, eps)
    ys, ms, var = yt * y_std + y_mean, mean.reshape(-1, c) * y_std + y_mean, np.diag(cov) * y_std ** 2
    if method == "gp":
        lp = O.normal_logpdf(ys, ms, np.sqrt(var)[:, None])
    else:
        nu, s = 2 * 1.7, 2.4 / 1.7
        khat = s * NT.theta("mlp", x, None, LAYERS, "relu", W, B, LW) + 1e-6 * np.eye(n)
        d = nu + float(np.sum(y * np.linalg.solve(khat, y)))
        lp = O.student_t_logpdf(ys, nu + n * c, ms, np.sqrt(d / (nu + n * c) * s * var)[:, None])
    return -float(np.mean(np.sum(lp, axis=1)))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("method", ["gp", "tp"])
@pytest.mark.parametrize("kind", ["nngp", "ntk"])
def test_model_posterior_test_nll_classify_sample_snapshot(ctx, kind, method, multi, dtype):
    model, x, y, xt, yt = _model(kind, method, multi, dtype)
    tol = TOL[dtype]
    ytm = yt if multi else yt[:, 0]
    ref = _ref_nll(kind, method, x, y, xt, yt, RIDGE[dtype], 0.3, 1.7)
    with model.posterior(capacity=16) as post:                # 45 test points: three chunks
        assert post.info == 0 and post.num_data == 70 and post.capacity == 16 and post.nbytes > 0
        got, own = post.test_nll(xt, ytm), model.test_nll(xt.astype(dtype), ytm)
        assert abs(got - ref) <= tol * abs(ref), (got, ref)
        assert abs(got - own) <= tol * abs(own), (got, own)
        if multi:
            assert np.array_equal(post.classify(xt), model.classify(xt.astype(dtype)))
            labels = np.argmax(yt, axis=1)
            assert post.accuracy(xt, labels) == model.accuracy(xt.astype(dtype), labels)
        else:
            with pytest.raises(NotImplementedError):
                post.classify(xt)
        with pytest.raises(ValueError, match="capacity = 16"):
            post.sample(3, xt, 2)
    with model.posterior(capacity=64) as post:
        # sample == sample_posterior's composition run by hand on predict(cov="full"), bit for bit
        draws = post.sample((11, 5), xt, 4, jitter=1e-3).raw_numpy()
        mean, cov = post.predict(xt, cov="full")
        t, c = mean.shape
        info = C.c_int()
        ctx.call("smn_cholesky", cov.dcode, cov.ptr, t, t, t, t, 0.0, 1e-3, C.byref(info), None)
        assert info.value == 0
        df_post, shape = model.predictive_params()
        out = ctx.empty((4, t, c) if multi else (4, t), mean.dtype)
        ctx.call("smn_mvn_draws", mean.dcode, mean.ptr, cov.ptr, t, t, c, 4, df_post or 0.0, shape, 11, 5, None, None, out.ptr)
        assert np.isfinite(draws).all() and np.array_equal(draws, out.raw_numpy())
        # a snapshot: moving the model's variables afterwards changes model.predict and leaves the posterior alone
        before, var_before = (a.raw_numpy() for a in post.predict(xt))
        model_before = np.asarray(model.predict(xt.astype(dtype))[0])
        model.kernel.w_std.assign(model.kernel.w_std.constraint.inverse(np.asarray(1.9)))
        after, var_after = (a.raw_numpy() for a in post.predict(xt))
        assert np.array_equal(before, after) and np.array_equal(var_before, var_after)
        assert not np.array_equal(model_before, np.asarray(model.predict(xt.astype(dtype))[0]))
        assert post.hyper["w_std"] == pytest.approx(W, rel=1e-12)


# ----------------------------------------------------------------------------- 7. not positive definite
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_matrix_that_is_not_positive_definite_gives_info_and_nan(L, ctx, dtype):
    rng = np.random.default_rng(2)
    n, t, c = 40, 7, 2
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = np.linspace(0.5, 2.0, n)
    ev[3] = -0.7                                              # one negative eigenvalue
    k = (q * ev) @ q.T
    f = Fit(L, ctx, dtype, c, 4, k=np.tril(k), y=rng.standard_normal((n, c)))
    try:
        assert f.info > 0 and np.isnan(f.logdet) and np.isnan(f.quad).all()
        ktd = rng.standard_normal((t, n))
        mean, var, _ = f.apply(ktd, ktt_diag=np.ones(t))
        assert np.isnan(mean).all() and np.isnan(var).all()
        f2 = f.apply(ktd[:3], ktt=np.eye(3), cov=True)
        assert all(np.isnan(a).all() for a in f2)
    finally:
        f.destroy()                                           # still destroys cleanly (SMN_OK)


# ----------------------------------------------------------------------------- 8. refusals
def _last_error(L, ctx):
    buf = C.create_string_buffer(512)
    L._lib.smn_last_error(ctx.handle, buf, 512)
    return buf.value.decode()


def test_refusals_name_the_argument(L, ctx):
    n, c, cap, dtype = 33, 1, 4, np.float64
    x, xt, y = data(n, 5, c, False)
    f = Fit(L, ctx, dtype, c, cap, x=x, y=y, net="mlp", act="relu", eps=1e-3)
    try:
        xd = ctx.to_device(xt)
        mean, var, cov = ctx.empty((5, c), dtype), ctx.empty((5,), dtype), ctx.empty((5, 5), dtype)
        raw = L._lib.smn_fit_predict
        assert raw(f.h, xd.ptr, 5, D, mean.ptr, None, cov.ptr, 5) == L.EINVAL          # cov_d with t > capacity
        assert "cov_d" in _last_error(L, ctx) and "capacity = 4" in _last_error(L, ctx)
        assert raw(f.h, xd.ptr, 3, D, mean.ptr, None, cov.ptr, 2) == L.EINVAL          # ldcov < t
        assert "ldcov" in _last_error(L, ctx)
        assert raw(f.h, xd.ptr, 5, D - 1, mean.ptr, var.ptr, None, 0) == L.EINVAL      # ldxt < d
        assert "ldxt" in _last_error(L, ctx)
        assert raw(f.h, xd.ptr, 0, D, mean.ptr, var.ptr, None, 0) == L.EINVAL          # t = 0
        assert "t = 0" in _last_error(L, ctx)
        assert raw(f.h, None, 5, D, mean.ptr, var.ptr, None, 0) == L.EINVAL and "xt_d" in _last_error(L, ctx)
        assert raw(f.h, xd.ptr, 5, D, None, var.ptr, None, 0) == L.EINVAL and "mean_d" in _last_error(L, ctx)
        ap = L._lib.smn_fit_apply
        kd = ctx.to_device(np.zeros((5, n)))
        assert ap(f.h, kd.ptr, 5, n - 1, var.ptr, None, 0, mean.ptr, var.ptr, None, 0) == L.EINVAL and "ldk" in _last_error(L, ctx)
        assert ap(f.h, kd.ptr, 3, n, None, None, 0, mean.ptr, var.ptr, None, 0) == L.EINVAL and "var_d" in _last_error(L, ctx)
        assert ap(f.h, kd.ptr, 3, n, var.ptr, None, 0, mean.ptr, None, cov.ptr, 3) == L.EINVAL and "k_tt_d" in _last_error(L, ctx)
        # the state still works after the refusals
        assert np.isfinite(f.predict(xt)[0]).all()
    finally:
        f.destroy()
    # creation: c = 49 (SMN_ENOTSUP, as everywhere else), capacity < 1, ldx < d
    xd, h = ctx.to_device(x), C.c_void_p()
    y49 = ctx.to_device(np.zeros((n, 49)))
    create = L._lib.smn_fit_create

    def make(c_, cap_, ldx, yd):
        return create(ctx.handle, L.F64, 0, 0, LAYERS, W, B, LW, xd.ptr, n, ldx, D, yd.ptr, c_, 1e-3, 0.0, cap_, C.byref(h), None, None,
                      None)
    assert make(49, 8, D, y49) == L.ENOTSUP and "c = 49" in _last_error(L, ctx) and not h.value
    assert make(1, 0, D, y49) == L.EINVAL and "capacity" in _last_error(L, ctx) and not h.value
    assert make(1, 8, D - 1, y49) == L.EINVAL and "ldx" in _last_error(L, ctx) and not h.value
    kd = ctx.to_device(np.eye(n))
    rc = L._lib.smn_fit_create_from_kernel(ctx.handle, L.F64, kd.ptr, n, n - 1, y49.ptr, 1, 0.0, 0.0, 8, C.byref(h), None, None, None)
    assert rc == L.EINVAL and "ldk" in _last_error(L, ctx) and not h.value
    # a state made from a kernel matrix has no inputs to build a cross kernel from
    f = Fit(L, ctx, np.float64, 1, 8, k=np.eye(n), y=y)
    try:
        with pytest.raises(L.SmnError, match="smn_fit_apply"):
            f.predict(xt)
    finally:
        f.destroy()


# ----------------------------------------------------------------------------- 9. predict_fn(cache=True)
@pytest.mark.parametrize("get,kind", [("nngp", "nngp"), ("ntk_gp", "ntk")])
def test_predict_fn_cache(ctx, get, kind):
    from smnngp import nt_kernels, predict
    n, t, c = 129, 130, 3
    x, xt, y = data(n, t, c, False)
    ref = reference("mlp", "relu", kind, n, t, c, False)
    kfn = nt_kernels.get_mlp_kernel(LAYERS, act="relu", w_std=W, b_std=B, last_w_std=LW)
    pf = predict.gradient_descent_mse_ensemble(kfn, x, y, diag_reg=1e-3, cache=True, cache_capacity=64)
    res = pf(x_test=xt, get=get)                              # 130 > 64 with a covariance: the state is made with capacity 130
    assert relerr_norm(np.asarray(res[0]), ref["mean"]) < 1e-7 and relerr_norm(np.asarray(res[1]), ref["cov"]) < 1e-7
    assert np.allclose(res.quad, ref["quad"], rtol=1e-7) and res.info == 0
    # a second, different x_test from the same state
    xt2 = np.random.default_rng(77).standard_normal((9, D))
    args = (LAYERS, "relu", W, B, LW, kind)
    m2, c2 = O.predict(ref["kdd"], OFN["mlp"](xt2, x, *args), OFN["mlp"](xt2, None, *args), y, diag_reg=1e-3)
    got = pf(x_test=xt2, get=get)
    assert relerr_norm(np.asarray(got[0]), m2) < 1e-7 and relerr_norm(np.asarray(got[1]), c2) < 1e-7
    assert relerr_norm(np.asarray(pf(x_test=xt2, get=get, compute_cov=False)), m2) < 1e-7
    # cache=False: the bits of a predict_fn made without the keyword
    a = predict.gradient_descent_mse_ensemble(kfn, x, y, diag_reg=1e-3, cache=False)(x_test=xt2, get=get)
    b = predict.gradient_descent_mse_ensemble(kfn, x, y, diag_reg=1e-3)(x_test=xt2, get=get)
    assert np.array_equal(np.asarray(a[0]), np.asarray(b[0])) and np.array_equal(np.asarray(a[1]), np.asarray(b[1]))


@pytest.mark.parametrize("cap", [64, 512])
def test_any_other_callable_takes_the_matrix_form(ctx, cap):
    """A kernel function that is neither KernelFn nor CnnKernelFn (here: the MLP kernel behind a lambda, as
    test_gpu_parity.py::test_predict_joint_and_fused wraps it): K_dd through the callable at creation, then per chunk
    kernel_fn(x_chunk, x_train) and the diagonal of kernel_fn(x_chunk, None) -- through predict_fn(cache=True) and through
    FittedPosterior itself, chunked."""
    from smnngp import nt_kernels, predict
    from smnngp.posterior import FittedPosterior
    n, t, c = 129, 130, 3
    x, xt, y = data(n, t, c, False)
    ref = reference("mlp", "relu", "nngp", n, t, c, False)
    kfn = nt_kernels.get_mlp_kernel(LAYERS, act="relu", w_std=W, b_std=B, last_w_std=LW)
    foreign = lambda a, b, g: kfn(a, b, g)   # noqa: E731
    pf = predict.gradient_descent_mse_ensemble(foreign, x, y, diag_reg=1e-3, cache=True, cache_capacity=cap)
    mean, cov = pf(x_test=xt)
    assert relerr_norm(np.asarray(mean), ref["mean"]) < 1e-7 and relerr_norm(np.asarray(cov), ref["cov"]) < 1e-7
    assert relerr_norm(np.asarray(pf(x_test=xt, compute_cov=False)), ref["mean"]) < 1e-7
    xd, yd = ctx.to_device(x), ctx.to_device(y)
    with FittedPosterior(foreign, xd, yd, ridge_rel=1e-3, capacity=cap, ctx=ctx) as post:
        assert not post.fused and post.info == 0 and np.allclose(post.quad, ref["quad"], rtol=1e-7)
        m, v = post.predict(xt)                                   # diagonal: three chunks at capacity 64
        check_against(ref, m.raw_numpy(), v.raw_numpy(), None, 1e-7)


def test_inputs_that_are_not_two_dimensional_and_a_positional_learning_rate(ctx):
    from smnngp import nt_kernels, predict
    from smnngp.posterior import FittedPosterior
    n, t, c = 33, 5, 1
    x, xt, y = data(n, t, c, False)
    kfn = nt_kernels.get_mlp_kernel(LAYERS, act="relu", w_std=W, b_std=B, last_w_std=LW)
    xd, yd = ctx.to_device(x), ctx.to_device(y)
    x3, xt3 = ctx.to_device(x.reshape(n, 2, 3)), ctx.to_device(xt.reshape(t, 2, 3))   # [N, 2, 3] is read as [N, 6]: a view, no copy
    with FittedPosterior(kfn, xd, yd, ridge_rel=1e-3, capacity=4, ctx=ctx) as flat, \
            FittedPosterior(kfn, x3, yd, ridge_rel=1e-3, capacity=4, ctx=ctx) as cube:
        a, b = flat.predict(xt), cube.predict(xt3)
        assert np.array_equal(a[0].raw_numpy(), b[0].raw_numpy()) and np.array_equal(a[1].raw_numpy(), b[1].raw_numpy())
        check_against(reference("mlp", "relu", "nngp", n, t, c, False), a[0].raw_numpy(), a[1].raw_numpy(), None, 1e-7)
    # learning_rate as the sixth positional argument, as before the keyword `cache` existed: the bits of the keyword form
    pos = predict.gradient_descent_mse_ensemble(kfn, x, y, 1e-3, False, 3.0)(t=2.0, x_test=xt)
    key = predict.gradient_descent_mse_ensemble(kfn, x, y, 1e-3, False, learning_rate=3.0)(t=2.0, x_test=xt)
    one = predict.gradient_descent_mse_ensemble(kfn, x, y, 1e-3, False)(t=2.0, x_test=xt)
    assert np.array_equal(pos[0], key[0]) and np.array_equal(pos[1], key[1]) and not np.array_equal(pos[0], one[0])


# ----------------------------------------------------------------------------- 10. lifetime
def test_create_and_destroy_many_states_and_the_context_still_works(L, ctx):
    n, t, c = 33, 5, 1
    x, xt, y = data(n, t, c, False)
    for _ in range(50):
        f = Fit(L, ctx, np.float64, c, 128, x=x, y=y, net="mlp", act="relu", eps=1e-3)
        nn, cc, cap, nbytes = f.nbytes()
        assert (nn, cc, cap) == (n, c, 128) and nbytes > 0
        f.destroy()
    # two live states and other calls on the context in between: a state that lived in workspace slots would be overwritten
    a = Fit(L, ctx, np.float64, c, 128, x=x, y=y, net="mlp", act="relu", eps=1e-3)
    first = a.predict(xt)
    fused_case(L, ctx, "resnet", "erf", "ntk", np.float64, (129, 130, 3), 128)
    fused_case(L, ctx, "mlp", "relu", "nngp", np.float32, (300, 257, 48), 128)
    again = a.predict(xt)
    a.destroy()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    check_against(reference("mlp", "relu", "nngp", n, t, c, False), first[0], first[1], None, 1e-7)
