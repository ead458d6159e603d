"""predict_fn(t=...) on the GPU against tests/_gd_rules.py, in fp32 and fp64, over t in {0, 1, 50, 1e4, inf}.

Tolerance (measured per case, not fixed): e32 is the error of the rules evaluated in float32 (LAPACK eigh, kernel build
included) against the same rules in float64, per case, time and output; means relative to max|mean_ref| over the case's
times, covariances relative to max|K_**|.  The device must satisfy
    err <= 16 * max(e32, 4 u32) * (u_dtype / u32):
rounding error is first-order linear in u, so the float32 LAPACK run is the yardstick of both precisions; the factor 16
covers Jacobi against tridiagonal QR, the MFMA summation order and the extra factorisation.  Every (err, e32, ratio) is
printed; the table of the implementing run is profiles/r15_gd_predict.txt.
"""
import functools

import numpy as np
import pytest

import _gd_rules as R

pytestmark = pytest.mark.gpu

TIMES = np.array([0.0, 1.0, 50.0, 1e4, np.inf])
U32 = float(np.finfo(np.float32).eps)
FACTOR = 16.0
DTYPES = [np.float32, np.float64]

# name: kind, hyper-parameters, N, T, input shape, C, diag_reg, absolute ridge, gets
CASES = {
    "mlp_relu": ("mlp", dict(num_hiddens=2, act="relu", w_std=1.3, b_std=0.4, last_w_std=0.9), 40, 7, (5,), 2, 1e-2, False, ("nngp", "ntk")),
    "mlp_erf": ("mlp", dict(num_hiddens=3, act="erf", w_std=1.5, b_std=0.3, last_w_std=1.0), 130, 9, (6,), 1, 1e-3, False, ("nngp", "ntk")),
    "resnet_relu": ("dense_resnet", dict(num_hiddens=2, act="relu", w_std=1.1, b_std=0.2, last_w_std=1.0), 257, 33, (12,), 3, 1e-4, False, ("nngp", "ntk")),
    "cnn_relu": ("cnn", dict(num_hiddens=2, act="relu", w_std=1.3, b_std=0.4, last_w_std=1.0), 24, 5, (6, 6, 2), 1, 1e-2, False, ("nngp",)),
    "mlp_abs_ridge": ("mlp", dict(num_hiddens=2, act="relu", w_std=1.3, b_std=0.4, last_w_std=0.9), 40, 7, (5,), 2, 3e-2, True, ("nngp", "ntk")),
}
PARAMS = [(name, get) for name, c in CASES.items() for get in c[8]]


@pytest.fixture(scope="module")
def ctx():
    from smnngp import _lib
    return _lib.default_context()


@functools.lru_cache(maxsize=None)
def data(name):
    kind, hyp, n, t, shape, c, diag_reg, absolute, _ = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    x = rng.standard_normal((n + t,) + shape)
    y = rng.standard_normal((n, c))
    return x, y


@functools.lru_cache(maxsize=None)
def rules(name, get, dtype):
    """(means, covs, evals) of the rules in `dtype`, computed once per case and shared read-only."""
    kind, hyp, n, t, shape, c, diag_reg, absolute, _ = CASES[name]
    x, y = data(name)
    k, th = R.joint_kernels(kind, x, get if get == "nngp" else ("nngp", "ntk"), dtype=dtype, **hyp)
    out = R.gd_predict(k, th, n, y, TIMES, diag_reg, absolute, dtype=dtype, with_evals=True)
    scale_c = float(np.abs(np.asarray(k, np.float64)[n:, n:]).max())
    for a in out:
        a.setflags(write=False)
    return out + (scale_c,)


def kernel_fn_of(name):
    from smnngp import nt_kernels
    kind, hyp = CASES[name][:2]
    h = dict(hyp)
    make = {"mlp": nt_kernels.get_mlp_kernel, "dense_resnet": nt_kernels.get_dense_resnet_kernel, "cnn": nt_kernels.get_cnn_kernel}[kind]
    return make(h.pop("num_hiddens"), **h)


def predict_fn_of(name, dtype, **kw):
    from smnngp.predict import gradient_descent_mse_ensemble
    kind, hyp, n, t, shape, c, diag_reg, absolute, _ = CASES[name]
    x, y = data(name)
    fn = gradient_descent_mse_ensemble(kernel_fn_of(name), x[:n].astype(dtype), y.astype(dtype), diag_reg=diag_reg,
                                       diag_reg_absolute_scale=absolute, **kw)
    return fn, x[n:].astype(dtype)


def bounds(name, get, dtype):
    """Per time: (bound on the mean error, bound on the covariance error, e32 mean, e32 cov, scale mean, scale cov)."""
    m64, c64, _, sc = rules(name, get, np.float64)
    m32, c32, _, _ = rules(name, get, np.float32)
    sm = float(np.abs(m64).max())
    ratio_u = float(np.finfo(dtype).eps) / U32
    out = []
    for j in range(len(TIMES)):
        em = float(np.abs(m32[j].astype(np.float64) - m64[j]).max()) / sm
        ec = float(np.abs(c32[j].astype(np.float64) - c64[j]).max()) / sc
        out.append((FACTOR * max(em, 4 * U32) * ratio_u, FACTOR * max(ec, 4 * U32) * ratio_u, em, ec, sm, sc))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,get", PARAMS)
def test_times_against_the_rules(ctx, name, get, dtype):
    kind, hyp, n, t, shape, c, diag_reg, absolute, _ = CASES[name]
    fn, xt = predict_fn_of(name, dtype)
    m64, c64, lam64, _ = rules(name, get, np.float64)
    res = fn(t=TIMES, x_test=xt, get=get, compute_cov=True)
    mean, cov = res
    assert res.info == 0 and mean.shape == (len(TIMES), t, c) and cov.shape == (len(TIMES), t, t) and mean.dtype == dtype
    bnd = bounds(name, get, dtype)
    u = float(np.finfo(dtype).eps)
    bad = []
    for j, tm in enumerate(TIMES):
        bm, bc, em, ec, sm, sc = bnd[j]
        err_m = float(np.abs(mean[j].astype(np.float64) - m64[j]).max()) / sm
        err_c = float(np.abs(cov[j].astype(np.float64) - c64[j]).max()) / sc
        print("gd %-13s %-4s %-7s t=%-7g mean err=%.2e e32=%.2e ratio=%6.3f | cov err=%.2e e32=%.2e ratio=%6.3f"
              % (name, get, np.dtype(dtype).name, tm, err_m, em, err_m * FACTOR / bm, err_c, ec, err_c * FACTOR / bc))
        if not (err_m <= bm and err_c <= bc):
            bad.append((tm, err_m, bm, err_c, bc))
        # an array call is the stacked scalar calls, bit for bit; mean-only calls give the same mean
        one = fn(t=float(tm), x_test=xt, get=get, compute_cov=True)
        assert one[0].shape == (t, c) and np.array_equal(one[0], mean[j]) and np.array_equal(one[1], cov[j])
        # symmetric to the bit or to 4u
        assert np.abs(cov[j] - cov[j].T).max() <= 4 * u * sc
    assert not bad, bad
    assert np.array_equal(fn(t=TIMES, x_test=xt, get=get, compute_cov=False), mean)
    # t = 0: mean 0 and K_** exactly (the block of the device's own joint kernel build)
    assert np.array_equal(mean[0], np.zeros((t, c), dtype))
    x, _ = data(name)
    k_j = kernel_fn_of(name)(x.astype(dtype), None, "nngp" if get == "nngp" else ("nngp", "ntk"))   # the build predict_fn runs
    k_ss = np.asarray(k_j if get == "nngp" else k_j[0])[n:, n:]
    assert np.array_equal(cov[0], np.tril(k_ss) + np.tril(k_ss, -1).T)
    # the nngp variance never grows with training time
    if get == "nngp":
        var = np.stack([np.diag(cov[j]) for j in range(len(TIMES))]).astype(np.float64)
        assert (np.diff(var, axis=0) <= 4 * u * sc).all()
    assert res.evals.shape == (n,) and res.evals.dtype == dtype and np.all(np.diff(res.evals) >= 0)
    # t = inf against the existing t = None path, within the same bound
    none = fn(t=None, x_test=xt, get=get, compute_cov=True)
    bm, bc = bnd[-1][:2]
    d_m = float(np.abs(np.asarray(none[0], np.float64).reshape(t, c) - mean[-1]).max()) / bnd[-1][4]
    d_c = float(np.abs(np.asarray(none[1], np.float64) - cov[-1]).max()) / bnd[-1][5]
    print("gd %-13s %-4s %-7s t=inf vs t=None: mean %.2e (bound %.2e) cov %.2e (bound %.2e)" % (name, get, np.dtype(dtype).name, d_m, bm, d_c, bc))
    assert d_m <= bm and d_c <= bc


@pytest.mark.parametrize("dtype", DTYPES)
def test_learning_rate_is_a_time_scale(ctx, dtype):
    fn3, xt = predict_fn_of("mlp_relu", dtype, learning_rate=3.0)
    fn1, _ = predict_fn_of("mlp_relu", dtype)
    for get in ("nngp", "ntk"):
        a = fn3(t=np.array([1.0, 50.0]), x_test=xt, get=get)
        b = fn1(t=np.array([3.0, 150.0]), x_test=xt, get=get)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_evals_are_eigh_pd_of_the_regularised_block(ctx):
    from smnngp import spectral
    kind, hyp, n, t, shape, c, diag_reg, absolute, _ = CASES["mlp_erf"]
    fn, xt = predict_fn_of("mlp_erf", np.float64)
    res = fn(t=1.0, x_test=xt, get="ntk")
    x, _ = data("mlp_erf")
    th = np.asarray(kernel_fn_of("mlp_erf")(x[:n], None, "ntk"))
    w = spectral.eigh_pd(R.regularised(th, diag_reg), ctx)[0]
    # the same solver on the same matrix, except that the ridge is added by the factorisation there and on the host here
    # (trace summed in another order: the shift moves by <= n u rho <= n u lambda_max, and by Weyl so does every eigenvalue)
    assert np.abs(res.evals - w).max() <= 2 * n * np.finfo(np.float64).eps * w.max()


def test_not_positive_definite_train_block_gives_nan(ctx):
    """Two identical training rows and no ridge, fp32: the train block is singular.  The rows are all ones and the layer
    program doubles the variance per layer (w_std = 2, no bias), so K(x0, x0) = 4 exactly, its pivot's square root is exact and
    the second pivot is 4 - (K(x1, x0) / 2)^2, which does not exceed 0 while K(x1, x0) >= 4."""
    from smnngp import nt_kernels
    from smnngp.predict import gradient_descent_mse_ensemble
    rng = np.random.default_rng(9)
    x = rng.standard_normal((20, 4)).astype(np.float32)
    x[0] = x[1] = 1.0
    y = rng.standard_normal((20, 1)).astype(np.float32)
    xt = rng.standard_normal((3, 4)).astype(np.float32)
    fn = gradient_descent_mse_ensemble(nt_kernels.get_mlp_kernel(2, act="relu", w_std=2.0, b_std=0.0), x, y, diag_reg=0.0)
    res = fn(t=np.array([1.0, np.inf]), x_test=xt, get="nngp")
    print("gd not-PD: info = %d" % res.info)
    assert res.info != 0
    assert np.isnan(res[0]).all() and np.isnan(res[1]).all() and res[0].shape == (2, 3, 1)


def test_bad_times_are_refused(ctx):
    fn, xt = predict_fn_of("mlp_relu", np.float64)
    for bad in (-1.0, np.nan, np.zeros((2, 2)), np.array([])):
        with pytest.raises(ValueError):
            fn(t=bad, x_test=xt)
    with pytest.raises(NotImplementedError):
        fn(t=1.0, x_test=xt, get="both")
