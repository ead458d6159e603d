"""smn_eigh_pd on the GPU: LAPACK's acceptance ratios for a symmetric eigensolver, in fp32 and fp64.

With u = eps(dtype), all in float64 arithmetic on the values the device saw and returned:
    r_A = ||A - V L V^T||_1 / (n u ||A||_1),   r_O = ||V^T V - I||_1 / (n u),   r_l = max|l - l_ref| / (n u l_max),
l_ref = float64 eigvalsh of the device's input.  All three must be <= 10 (LAPACK's own test programs accept 50); the ratios of
numpy.linalg.eigh in the same dtype are printed beside them for orientation.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import nngp_oracle as O
from _windows import in_window, out_window

pytestmark = pytest.mark.gpu

BOUND = 10.0
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def ctx():
    from smnngp import _lib
    return _lib.default_context()


@functools.lru_cache(maxsize=None)
def ntk_block(n, diag_reg=1e-3):
    """NTK train block + relative ridge, as the prediction tests regularise it (float64)."""
    rng = np.random.default_rng(100 + n)
    x = rng.standard_normal((n, 6))
    th = O.mlp_kernel(x, None, num_hiddens=2, act="relu", w_std=1.3, b_std=0.4, last_w_std=1.0, get="ntk")
    a = th + diag_reg * np.trace(th) / n * np.eye(n)
    a.setflags(write=False)
    return a


def ratios(a, w, v, dtype):
    a = np.asarray(a, np.float64)
    a = np.tril(a) + np.tril(a, -1).T
    w, v = np.asarray(w, np.float64), np.asarray(v, np.float64)
    n, u = a.shape[0], float(np.finfo(dtype).eps)
    one = lambda m: np.abs(m).sum(axis=0).max()
    r_a = one(a - (v * w) @ v.T) / (n * u * one(a))
    r_o = one(v.T @ v - np.eye(n)) / (n * u)
    ref = np.linalg.eigvalsh(a)
    r_l = np.abs(w - ref).max() / (n * u * ref.max())
    return r_a, r_o, r_l


def device_eigh(ctx, a, dtype, max_sweeps=0):
    ad = ctx.to_device(np.ascontiguousarray(a, dtype=dtype))
    n = a.shape[0]
    w, v = ctx.empty((n,), dtype), ctx.empty((n, n), dtype)
    info, sweeps = C.c_int(12345), C.c_int(-7)
    ctx.call("smn_eigh_pd", ad.dcode, ad.ptr, n, n, w.ptr, v.ptr, n, max_sweeps, C.byref(info), C.byref(sweeps))
    return w.numpy(), v.numpy(), info.value, sweeps.value


def check(ctx, name, a, dtype):
    a_seen = np.ascontiguousarray(a, dtype=dtype)
    w, v, info, sweeps = device_eigh(ctx, a_seen, dtype)
    lw, lv = np.linalg.eigh(a_seen)
    dev, lap = ratios(a_seen, w, v, dtype), ratios(a_seen, lw, lv, dtype)
    print("eigh %-14s %-7s n=%4d sweeps=%2d  device r_A=%.3f r_O=%.3f r_l=%.3f   LAPACK r_A=%.3f r_O=%.3f r_l=%.3f"
          % (name, np.dtype(dtype).name, a.shape[0], sweeps, *dev, *lap))
    assert info == 0
    assert np.all(np.diff(w) >= 0), "eigenvalues must ascend"
    assert max(dev) <= BOUND, dev
    return w, v


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 2, 33, 130, 257, 512])
def test_a_ntk_blocks(ctx, n, dtype):
    check(ctx, "A ntk+ridge", ntk_block(n), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_b_window_with_guard_bands(ctx, dtype):
    n = 130
    a = np.ascontiguousarray(ntk_block(n), dtype=dtype)
    aw = in_window(ctx, a, layout="unaligned", ld=n + 7)
    vw = out_window(ctx, n, n, dtype, layout="unaligned", ld=n + 7)
    ww = out_window(ctx, 1, n, dtype, layout="unaligned")
    info = C.c_int(-5)
    ctx.call("smn_eigh_pd", aw.dev.dcode, aw.ptr, n, aw.ld, ww.ptr, vw.ptr, vw.ld, 0, C.byref(info), None)
    v, w = vw.result("v"), ww.result("w")[0]
    aw.assert_guard_untouched(what="a")          # A is not modified, and neither is its NaN guard
    assert np.array_equal(aw.inside(aw.download()), a)
    r = ratios(a, w, v, dtype)
    print("eigh B window        %-7s n= 130 ld=137  device r_A=%.3f r_O=%.3f r_l=%.3f" % (np.dtype(dtype).name, *r))
    assert info.value == 0 and max(r) <= BOUND, (info.value, r)
    w0, v0, _, _ = device_eigh(ctx, a, dtype)
    assert np.array_equal(w0, w) and np.array_equal(v0, v), "the window call must give the contiguous call's bits"


@pytest.mark.parametrize("dtype", DTYPES)
def test_c_clustered_spectrum(ctx, dtype):
    n = 96
    u, _ = np.linalg.qr(np.random.default_rng(5).standard_normal((n, 5)))
    a = 0.5 * np.eye(n) + (u * np.array([3.0, 3.0, 3.0, 1.0, 1.0])) @ u.T      # 91 equal eigenvalues
    check(ctx, "C clustered", a, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_d_graded_spectrum(ctx, dtype):
    n = 64
    q, _ = np.linalg.qr(np.random.default_rng(6).standard_normal((n, n)))
    lam = np.logspace(0, -10 if dtype == np.float64 else -4, n)
    a = (q * lam) @ q.T
    check(ctx, "D graded", 0.5 * (a + a.T), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_e_not_positive_definite(ctx, dtype):
    n = 40
    d = np.ones(n)
    d[-1] = -1.0
    w, v, info, _ = device_eigh(ctx, np.diag(d), dtype)
    print("eigh E not PD        %-7s n=  40 info=%d" % (np.dtype(dtype).name, info))
    assert info > 0            # the failing pivot, 1-based as everywhere in the library: 40
    assert np.isnan(w).all() and np.isnan(v).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_f_same_bits_twice(ctx, dtype):
    a = ntk_block(257)
    w1, v1, i1, s1 = device_eigh(ctx, a, dtype)
    w2, v2, i2, s2 = device_eigh(ctx, a, dtype)
    assert (i1, s1) == (i2, s2) and i1 == 0
    assert np.array_equal(w1.view(np.uint8), w2.view(np.uint8)) and np.array_equal(v1.view(np.uint8), v2.view(np.uint8))


@pytest.mark.parametrize("dtype", DTYPES)
def test_g_sweep_limit_is_reported_not_fatal(ctx, dtype):
    a = ntk_block(257)
    w, v, info, sweeps = device_eigh(ctx, a, dtype, max_sweeps=1)
    assert info == -1 and sweeps == 1
    assert np.isfinite(w).all() and np.isfinite(v).all()
    w2, v2, info2, _ = device_eigh(ctx, a, dtype)        # the same context goes on working
    assert info2 == 0 and max(ratios(np.asarray(a, dtype), w2, v2, dtype)) <= BOUND


def test_h_leading_dimensions_refused_by_name(ctx):
    from smnngp import _lib
    n = 8
    a = ctx.to_device(np.eye(n))
    w, v = ctx.empty((n,), np.float64), ctx.empty((n, n), np.float64)
    info = C.c_int()
    for args, name in (((a.ptr, n, n - 1, w.ptr, v.ptr, n), "lda"), ((a.ptr, n, n, w.ptr, v.ptr, n - 1), "ldv")):
        with pytest.raises(_lib.SmnError) as e:
            ctx.call("smn_eigh_pd", _lib.F64, *args, 0, C.byref(info), None)
        assert e.value.code == _lib.EINVAL and name in str(e.value) and "smn_eigh_pd" in str(e.value)


@pytest.mark.parametrize("dtype", DTYPES)
def test_spectral_eigh_pd_round_trip(ctx, dtype):
    from smnngp import spectral
    a = np.ascontiguousarray(ntk_block(130), dtype=dtype)
    res = spectral.eigh_pd(a, ctx)
    w, v = res
    assert res.info == 0 and res.sweeps >= 1 and w.dtype == dtype and v.shape == (130, 130)
    assert max(ratios(a, w, v, dtype)) <= BOUND
    lr = spectral.max_learning_rate(a, 130 * 2, ctx=ctx)
    assert abs(lr - 2.0 * 260 / (float(w[-1]) + 1e-12)) <= 1e-6 * lr
