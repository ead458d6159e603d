"""Windowed C-ABI tests: every entry point that takes a leading dimension runs once on exactly sized contiguous buffers and
once on windows into larger allocations (tests/_windows.py), in the same context.

Unless a test says otherwise the result inside the window must be BIT-IDENTICAL to the contiguous call (the leading dimension
and the base pointer must not reach the arithmetic), every byte of an output window's guard must be what it was, and input
windows carry NaN in their padding columns and in the rows before and after, so an over-read poisons the result.  The one
exception is smn_cholesky where its documented alignment rule selects the other route (see there).  No tolerance is
introduced here.

Layouts: "aligned" keeps every vector path and the in-place factorisation eligible; "unaligned" (col_off = 1, odd ld) is used
for the entries whose header comment states no alignment rule."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _windows as W  # noqa: E402
from _tol import relerr_norm  # noqa: E402

DTYPES = [np.float64, np.float32]
BOTH = ("aligned", "unaligned")
HYP = (1.3, 0.4, 0.9)          # w_std, b_std, last_w_std
D = 6


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


# ----------------------------------------------------------------------------- plumbing
class Plain:
    """An exactly sized contiguous device buffer with the interface of a window."""

    def __init__(self, ctx, host):
        host = np.ascontiguousarray(host)
        self.host0 = host.copy()
        self.dev = ctx.to_device(host)
        self.ptr = self.dev.ptr
        self.ld = host.shape[-1]

    def result(self, what=None):
        return self.dev.raw_numpy().reshape(self.host0.shape)


def _interior(rows, cols, dtype, seed):
    return W.pattern(rows, cols, dtype, seed + 101)


def out_buf(ctx, layout, rows, cols, dtype, seed=0, data=None, **kw):
    """Output operand: a window in `layout`, or (layout None) the contiguous twin that starts from the same contents."""
    data = _interior(rows, cols, dtype, seed) if data is None else np.asarray(data, dtype=dtype).reshape(rows, cols)
    if layout is None:
        return Plain(ctx, data)
    return W.out_window(ctx, rows, cols, dtype, layout, data=data, seed=seed, **kw)


def in_buf(ctx, layout, data, **kw):
    data = np.asarray(data)
    if layout is None:
        return Plain(ctx, data if data.ndim > 1 else data[None, :])
    return W.in_window(ctx, data, layout, **kw)


def images_buf(ctx, layout, x):
    """Images have no leading dimension: one NaN guard image before and after the n images."""
    flat = x.reshape(x.shape[0], -1)
    if layout is None:
        return Plain(ctx, flat)
    return W.in_window(ctx, flat, "block", rows_before=1, rows_after=1)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, "%s: %d of %d elements differ from the contiguous call, first at %s: %r vs %r" % (
        what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def assert_same_scalars(got, want, what):
    assert np.array_equal(bits(np.asarray(got, np.float64)), bits(np.asarray(want, np.float64))), (what, got, want)


def _inputs(n, d, dtype, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(dtype)


def _net(L, net, act, layers):
    return (L.NET_MLP if net == "mlp" else L.NET_DENSE_RESNET, L.ACT[act], layers) + HYP


def _spd(rng, n, cond=1e3):
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (q * np.geomspace(1.0, cond, n)) @ q.T


def _kernel_like(n, dtype, seed, c=1):
    """x, y and a positive definite kernel-like matrix K = x x^T / d + 1 (jitter comes from the call)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, D))
    k = (x @ x.T / D + 1.0).astype(dtype)
    y = rng.standard_normal((n, c)).astype(dtype)
    return x.astype(dtype), y, k


def _nan_above_diagonal(a):
    a = np.array(a, copy=True)
    a[np.triu_indices(a.shape[0], 1)] = np.nan
    return a


# ----------------------------------------------------------------------------- builds
NETS = [("mlp", "relu", 1, "nngp"), ("mlp", "erf", 2, "both"), ("resnet", "relu", 2, "both"), ("resnet", "erf", 1, "nngp")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("net,act,layers,get", NETS)
@pytest.mark.parametrize("mode", ["full", "lower", "cross"])
@pytest.mark.parametrize("n", [1, 129, 200])
def test_kernel_mlp(L, ctx, dtype, net, act, layers, get, mode, n):
    n2 = 70 if mode == "cross" else n
    x1, x2 = _inputs(n, D, dtype, n), _inputs(n2, D, dtype, n + 1)
    mask = L.GET_NNGP | (L.GET_NTK if get == "both" else 0)
    fill = L.FILL_LOWER if mode == "lower" else L.FILL_FULL

    def run(layout):
        a = in_buf(ctx, layout, x1)
        b = in_buf(ctx, layout, x2) if mode == "cross" else None
        k = out_buf(ctx, layout, n, n2, dtype, 1)
        t = out_buf(ctx, layout, n, n2, dtype, 2) if get == "both" else None
        ctx.call("smn_kernel_mlp", L.dtype_code(dtype), *_net(L, net, act, layers), a.ptr, n, a.ld, b.ptr if b else None,
                 n2 if b else 0, b.ld if b else 0, D, mask, fill, k.ptr, t.ptr if t else None, k.ld)
        return [o.result("smn_kernel_mlp %s" % nm) for o, nm in ((k, "nngp"), (t, "ntk")) if o is not None]

    want = run(None)
    assert all(np.isfinite(np.tril(w) if mode == "lower" else w).all() for w in want)
    for layout in BOTH:
        for g, w in zip(run(layout), want):
            if mode == "lower":          # FILL_LOWER: the lower triangle and the guard
                g, w = np.tril(g), np.tril(w)
            assert_same_bits(g, w, "smn_kernel_mlp %s %s" % (mode, layout))
    if mode == "full":
        assert all(np.array_equal(w, w.T) for w in want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("entry", ["smn_kernel_mlp_rows", "smn_kernel_mlp_lower_rows"])
@pytest.mark.parametrize("rb,re", [(37, 170), (128, 200)])      # off a tile boundary (the re-pad branch reads x + rb * ldx), and on one
def test_kernel_mlp_rows(L, ctx, dtype, entry, rb, re):
    n = 200
    x = _inputs(n, D, dtype, 7)
    cols = re if entry.endswith("lower_rows") else n

    def run(layout):
        a = in_buf(ctx, layout, x)
        k = out_buf(ctx, layout, re - rb, cols, dtype, 1)
        t = out_buf(ctx, layout, re - rb, cols, dtype, 2)
        ctx.call(entry, L.dtype_code(dtype), *_net(L, "mlp", "erf", 2), a.ptr, n, a.ld, D, rb, re, L.GET_NNGP | L.GET_NTK,
                 k.ptr, t.ptr, k.ld)
        return k.result(entry + " nngp"), t.result(entry + " ntk")

    # lower_rows: what lies right of the diagonal inside the written range is unspecified and not compared
    keep = (np.arange(cols)[None, :] <= rb + np.arange(re - rb)[:, None]) if entry.endswith("lower_rows") else np.ones((re - rb, cols), bool)
    want = run(None)
    assert all(np.isfinite(w[keep]).all() for w in want)
    for layout in BOTH:
        for g, w in zip(run(layout), want):
            assert_same_bits(np.where(keep, g, 0), np.where(keep, w, 0), "%s [%d,%d) %s" % (entry, rb, re, layout))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("n", [1, 129, 200])
def test_gram(L, ctx, dtype, cross, n):
    n2 = 70 if cross else n
    x1, x2 = _inputs(n, D, dtype, n), _inputs(n2, D, dtype, n + 1)

    def run(layout):
        a = in_buf(ctx, layout, x1)
        b = in_buf(ctx, layout, x2) if cross else None
        k0 = out_buf(ctx, layout, n, n2, dtype, 1)
        q1 = out_buf(ctx, layout, 1, n, dtype, 2)               # 1-D outputs: guards on both sides
        q2 = out_buf(ctx, layout, 1, n2, dtype, 3) if cross else None
        ctx.call("smn_gram", L.dtype_code(dtype), a.ptr, n, a.ld, b.ptr if b else None, n2 if b else 0, b.ld if b else 0, D,
                 k0.ptr, k0.ld, q1.ptr, q2.ptr if q2 else None)
        return [o.result("smn_gram %s" % nm) for o, nm in ((k0, "k0"), (q1, "q1"), (q2, "q2")) if o is not None]

    want = run(None)
    assert all(np.isfinite(w).all() for w in want)
    for layout in BOTH:
        for g, w in zip(run(layout), want):
            assert_same_bits(g, w, "smn_gram %s" % layout)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("net,act,layers,get", NETS)
@pytest.mark.parametrize("n,sym", [(1, 1), (129, 1), (200, 1), (200, 0), (129, 0)])
def test_recursion(L, ctx, dtype, net, act, layers, get, n, sym):
    """smn_recursion streams 16-byte vectors: the aligned layout only (the unaligned ones are refused, below)."""
    n2 = n if sym else 70
    x1 = _inputs(n, D, np.float64, n)
    x2 = x1 if sym else _inputs(n2, D, np.float64, n + 1)
    k0 = (x1 @ x2.T / D).astype(dtype)
    q1, q2 = ((x1 * x1).sum(1) / D).astype(dtype), ((x2 * x2).sum(1) / D).astype(dtype)
    mask = L.GET_NNGP | (L.GET_NTK if get == "both" else 0)

    def run(layout):
        a = in_buf(ctx, layout, k0)
        u, v = in_buf(ctx, layout, q1), in_buf(ctx, layout, q2)
        k = out_buf(ctx, layout, n, n2, dtype, 1)
        t = out_buf(ctx, layout, n, n2, dtype, 2) if get == "both" else None
        ctx.call("smn_recursion", L.dtype_code(dtype), *_net(L, net, act, layers), a.ptr, n, n2, a.ld, u.ptr, v.ptr, sym, mask,
                 k.ptr, t.ptr if t else None, k.ld)
        return [o.result("smn_recursion %s" % nm) for o, nm in ((k, "nngp"), (t, "ntk")) if o is not None]

    want = run(None) if k0.shape[1] % (16 // np.dtype(dtype).itemsize) == 0 else None   # (a contiguous ld must be aligned too)
    got = run("aligned")
    assert all(np.isfinite(g).all() for g in got)
    if want is None:                   # n2 is no multiple of 16 bytes: the contiguous twin is a second aligned window with another ld
        al = 16 // np.dtype(dtype).itemsize
        a = in_buf(ctx, "aligned", k0, ld=(n2 + 3 * al) // al * al, col_off=0)
        u, v = in_buf(ctx, None, q1), in_buf(ctx, None, q2)
        k = out_buf(ctx, "aligned", n, n2, dtype, 1, ld=(n2 + 5 * al) // al * al, col_off=2 * al)
        t = out_buf(ctx, "aligned", n, n2, dtype, 2, ld=(n2 + 5 * al) // al * al, col_off=2 * al) if get == "both" else None
        ctx.call("smn_recursion", L.dtype_code(dtype), *_net(L, net, act, layers), a.ptr, n, n2, a.ld, u.ptr, v.ptr, sym, mask,
                 k.ptr, t.ptr if t else None, k.ld)
        want = [o.result("smn_recursion twin") for o in (k, t) if o is not None]
    for g, w in zip(got, want):
        assert_same_bits(g, w, "smn_recursion aligned")
        if sym:
            assert np.array_equal(g, g.T)


@pytest.mark.parametrize("dtype", DTYPES)
def test_recursion_refuses_unaligned_pointers_and_leading_dimensions(L, ctx, dtype):
    n = 8
    al = 16 // np.dtype(dtype).itemsize
    big = ctx.to_device(np.ones((4 * n, 4 * n), dtype))
    q = ctx.to_device(np.ones(n, dtype))
    isz = np.dtype(dtype).itemsize
    off = C.c_void_p(big.ptr.value + isz)                       # one element in: not 16-byte aligned
    ok_ld, odd_ld = 2 * n, 2 * n + 1
    assert ok_ld % al == 0 and odd_ld % al != 0
    base = ("smn_recursion", L.dtype_code(dtype)) + _net(L, "mlp", "relu", 1)
    calls = {"k0 pointer": base + (off, n, n, ok_ld, q.ptr, q.ptr, 1, L.GET_NNGP, big.ptr, None, ok_ld),
             "out pointer": base + (big.ptr, n, n, ok_ld, q.ptr, q.ptr, 1, L.GET_NNGP, off, None, ok_ld),
             "ntk pointer": base + (big.ptr, n, n, ok_ld, q.ptr, q.ptr, 1, L.GET_NNGP | L.GET_NTK, big.ptr, off, ok_ld),
             "ldk0": base + (big.ptr, n, n, odd_ld, q.ptr, q.ptr, 1, L.GET_NNGP, big.ptr, None, ok_ld),
             "ldk": base + (big.ptr, n, n, ok_ld, q.ptr, q.ptr, 1, L.GET_NNGP, big.ptr, None, odd_ld)}
    for what, call in calls.items():
        with pytest.raises(L.SmnError) as e:
            ctx.call(*call)
        assert e.value.code == L.EINVAL, what


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("entry,shape,depth", [("smn_kernel_cnn", (5, 6, 6, 2), 2), ("smn_kernel_cnn", (3, 32, 32, 3), 1),
                                               ("smn_kernel_conv_resnet", (4, 8, 8, 2), 1)])
def test_conv_kernels(L, ctx, dtype, cross, entry, shape, depth):
    n, H, Wd, Ch = shape
    n2 = 2 if cross else n
    rng = np.random.default_rng(n)
    x1 = rng.standard_normal(shape).astype(dtype)
    x2 = rng.standard_normal((n2, H, Wd, Ch)).astype(dtype)

    def run(layout):
        a = images_buf(ctx, layout, x1)
        b = images_buf(ctx, layout, x2) if cross else None
        k = out_buf(ctx, layout, n, n2, dtype, 1)
        ctx.call(entry, L.dtype_code(dtype), L.ACT["relu"], depth, *HYP, a.ptr, n, b.ptr if b else None, n2 if b else 0, H, Wd, Ch,
                 L.FILL_FULL, k.ptr, k.ld)
        return k.result(entry)

    want = run(None)
    assert np.isfinite(want).all()
    for layout in BOTH:
        assert_same_bits(run(layout), want, "%s %s" % (entry, layout))


# ----------------------------------------------------------------------------- factorisation, solves, heads
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_total,n_factor", [(256, 256), (384, 256), (200, 200), (237, 200)])
def test_cholesky(L, ctx, dtype, n_total, n_factor):
    """Lower triangle of the factor, the B L^-T rows and the lower triangle of the Schur block inside the window, plus the
    guard; the strict upper triangle is not specified.  Positive-definite input."""
    import scipy.linalg as sla
    a64 = _spd(np.random.default_rng(n_total + n_factor), n_total)
    a = a64.astype(dtype)
    al = 16 // np.dtype(dtype).itemsize
    tile_sized = n_total % 128 == 0 and n_factor % 128 == 0
    keep = np.tril(np.ones((n_total, n_total), bool))
    keep[n_factor:, :n_factor] = True

    def run(layout):
        # the tile-sized matrices sit at lda = n_total + 144 in the aligned layout: eligible for the in-place route
        kw = dict(ld=n_total + 144) if layout == "aligned" and tile_sized else {}
        m = out_buf(ctx, layout, n_total, n_total, dtype, 1, data=a, **kw)
        info, logdet = C.c_int(-1), C.c_double()
        ctx.call("smn_cholesky", L.dtype_code(dtype), m.ptr, n_total, n_factor, m.ld, 0, 0.0, 0.0, C.byref(info), C.byref(logdet))
        assert info.value == 0
        inplace = tile_sized and m.ld % al == 0 and m.ptr.value % 16 == 0
        return m.result("smn_cholesky"), logdet.value, inplace

    want, want_ld, want_inplace = run(None)
    assert want_inplace == tile_sized
    for layout in BOTH:
        got, got_ld, inplace = run(layout)
        assert inplace == (tile_sized and layout == "aligned")
        if inplace == want_inplace:
            assert_same_bits(np.where(keep, got, 0), np.where(keep, want, 0), "smn_cholesky %s" % layout)
            assert_same_scalars(got_ld, want_ld, "logdet")
        else:
            # The documented alignment rule sends this window through the padded-copy route and the contiguous call through
            # the in-place one: another schedule, not the same bits.  Compared with the fp64 NumPy reference instead, at the
            # tolerance test_gpu_parity.py::test_cholesky_and_schur holds this entry to.
            tol = 1e-9 if dtype == np.float64 else 5e-3
            g = got.astype(np.float64)
            l = np.linalg.cholesky(a64[:n_factor, :n_factor])
            assert abs(got_ld - 2 * np.log(np.diag(l)).sum()) < tol * max(1.0, abs(got_ld))
            assert relerr_norm(np.tril(g[:n_factor, :n_factor]), l) < tol
            if n_total > n_factor:
                w = sla.solve_triangular(l, a64[:n_factor, n_factor:], lower=True).T
                assert relerr_norm(g[n_factor:, :n_factor], w) < tol
                assert relerr_norm(np.tril(g[n_factor:, n_factor:]), np.tril(a64[n_factor:, n_factor:] - w @ w.T)) < tol


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("nrhs", [1, 45])
def test_trsm(L, ctx, dtype, trans, nrhs):
    n = 200
    rng = np.random.default_rng(nrhs)
    l = _nan_above_diagonal(np.linalg.cholesky(_spd(rng, n, cond=100.0))).astype(dtype)   # nothing above the diagonal is read
    b = rng.standard_normal((n, nrhs)).astype(dtype)

    def run(layout):
        lw = in_buf(ctx, layout, l)
        bw = out_buf(ctx, layout, n, nrhs, dtype, 1, data=b)
        ctx.call("smn_trsm", L.dtype_code(dtype), lw.ptr, n, lw.ld, bw.ptr, nrhs, bw.ld, trans)
        return bw.result("smn_trsm")

    want = run(None)
    assert np.isfinite(want).all()
    for layout in BOTH:
        assert_same_bits(run(layout), want, "smn_trsm trans=%d %s" % (trans, layout))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [0, 3])                 # 0: smn_lml; 3: smn_lml_multi
@pytest.mark.parametrize("n", [1, 129, 200])
def test_lml(L, ctx, dtype, c, n):
    _, y, k = _kernel_like(n, dtype, n, max(c, 1))
    k = _nan_above_diagonal(k)                          # K is given by its lower triangle
    df, scale = (4.0, 1.5) if c == 0 else (0.0, 1.0)

    def run(layout):
        kw = in_buf(ctx, layout, k)
        yd = ctx.to_device(y)
        lp, quad, logdet, info = C.c_double(), C.c_double(), C.c_double(), C.c_int(-1)
        if c == 0:
            ctx.call("smn_lml", L.dtype_code(dtype), kw.ptr, n, kw.ld, yd.ptr, 0.1, df, scale, C.byref(lp), C.byref(quad),
                     C.byref(logdet), C.byref(info))
            out = [lp.value, quad.value, logdet.value]
        else:
            cols = (C.c_double * c)()
            ctx.call("smn_lml_multi", L.dtype_code(dtype), kw.ptr, n, kw.ld, yd.ptr, c, 0.1, df, scale, C.byref(lp), C.byref(quad),
                     cols, C.byref(logdet), C.byref(info))
            out = [lp.value, quad.value, logdet.value] + list(cols)
        assert info.value == 0
        if layout is not None:                              # K may be overwritten, its surroundings may not
            kw.assert_guard_untouched(what="K of the log-marginal likelihood")
        return out

    want = run(None)
    assert np.isfinite(want).all()
    for layout in BOTH:
        assert_same_scalars(run(layout), want, "lml c=%d %s" % (c, layout))


def _joint(n, t, c, dtype, seed):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n + t, D))
    kj = (z @ z.T / D + 1.0).astype(dtype)
    return z[:n].astype(dtype), z[n:].astype(dtype), rng.standard_normal((n, c)).astype(dtype), kj


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,t,c", [(1, 1, 1), (129, 130, 3), (200, 1, 3), (200, 130, 1)])
def test_predict(L, ctx, dtype, n, t, c):
    _, _, y, kj = _joint(n, t, c, dtype, n + t)
    kj = _nan_above_diagonal(kj)

    def run(layout):
        kw = in_buf(ctx, layout, kj)
        yd = ctx.to_device(y)
        mean = out_buf(ctx, None if layout is None else "block", t, c, dtype, 1)       # [t, c] has no leading dimension
        cov = out_buf(ctx, layout, t, t, dtype, 2)
        quad, logdet, info = (C.c_double * c)(), C.c_double(), C.c_int(-1)
        ctx.call("smn_predict", L.dtype_code(dtype), kw.ptr, n, t, kw.ld, yd.ptr, c, 1e-2, 1e-3, mean.ptr, cov.ptr, cov.ld, quad,
                 C.byref(logdet), C.byref(info))
        assert info.value == 0
        if layout is not None:
            kw.assert_guard_untouched(what="joint kernel of smn_predict")
        return mean.result("mean"), cov.result("cov"), list(quad) + [logdet.value]

    want = run(None)
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
    for layout in BOTH:
        mean, cov, scal = run(layout)
        assert_same_bits(mean, want[0], "smn_predict mean %s" % layout)
        assert_same_bits(cov, want[1], "smn_predict cov %s" % layout)
        assert np.array_equal(cov, cov.T)                   # full and symmetric inside the window
        assert_same_scalars(scal, want[2], "smn_predict scalars %s" % layout)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 129, 200])
def test_spr_loss(L, ctx, dtype, n):
    x, y, _ = _kernel_like(n, dtype, n)

    def run(layout):
        xw = in_buf(ctx, layout, x)
        yd = ctx.to_device(y)
        lp, quad, logdet, info = C.c_double(), C.c_double(), C.c_double(), C.c_int(-1)
        ctx.call("smn_spr_loss", L.dtype_code(dtype), *_net(L, "mlp", "relu", 2), xw.ptr, n, xw.ld, D, yd.ptr, 0.1, 4.0, 1.5,
                 C.byref(lp), C.byref(quad), C.byref(logdet), C.byref(info))
        assert info.value == 0
        return [lp.value, quad.value, logdet.value]

    want = run(None)
    assert np.isfinite(want).all()
    for layout in BOTH:
        assert_same_scalars(run(layout), want, "smn_spr_loss %s" % layout)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,t,c", [(1, 1, 1), (129, 130, 3), (200, 1, 3), (200, 130, 1)])
def test_spr_predict(L, ctx, dtype, n, t, c):
    x, xt, y, _ = _joint(n, t, c, dtype, n + t)

    def run(layout):
        xw, xtw = in_buf(ctx, layout, x), in_buf(ctx, layout, xt)
        yd = ctx.to_device(y)
        mean = out_buf(ctx, None if layout is None else "block", t, c, dtype, 1)
        cov = out_buf(ctx, layout, t, t, dtype, 2)
        quad, logdet, info = (C.c_double * c)(), C.c_double(), C.c_int(-1)
        ctx.call("smn_spr_predict", L.dtype_code(dtype), *_net(L, "resnet", "erf", 1), xw.ptr, n, xw.ld, xtw.ptr, t, xtw.ld, D,
                 yd.ptr, c, 1e-2, 1e-3, mean.ptr, cov.ptr, cov.ld, quad, C.byref(logdet), C.byref(info))
        assert info.value == 0
        return mean.result("mean"), cov.result("cov"), list(quad) + [logdet.value]

    want = run(None)
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
    for layout in BOTH:
        mean, cov, scal = run(layout)
        assert_same_bits(mean, want[0], "smn_spr_predict mean %s" % layout)
        assert_same_bits(cov, want[1], "smn_spr_predict cov %s" % layout)
        assert np.array_equal(cov, cov.T)
        assert_same_scalars(scal, want[2], "smn_spr_predict scalars %s" % layout)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,t,c", [(129, 130, 3), (200, 1, 1)])
def test_spr_predict_batch(L, ctx, dtype, n, t, c):
    nprob = 3
    x, xt, y, _ = _joint(n, t, c, dtype, n + t)
    arr = lambda v: (C.c_double * nprob)(*v)   # noqa: E731
    al = 16 // np.dtype(dtype).itemsize

    def run(layout):
        xw, xtw = in_buf(ctx, layout, x), in_buf(ctx, layout, xt)
        yd = ctx.to_device(y)
        blk = None if layout is None else "block"
        # [nprob, t, c], [nprob, t, ldcov] and [nprob, t]: guards around the whole block; the ldcov padding inside the block is
        # the guard right of each row
        ldcov = t if layout is None else ((t + al) // al * al if layout == "aligned" else t + 3)
        mean = out_buf(ctx, blk, nprob * t, c, dtype, 1)
        cov = out_buf(ctx, blk, nprob * t, t, dtype, 2, **({} if layout is None else dict(ld=ldcov)))
        var = out_buf(ctx, blk, 1, nprob * t, dtype, 3)
        quad, logdet, info = (C.c_double * (nprob * c))(), arr([0] * nprob), (C.c_int * nprob)(-1, -1, -1)
        ctx.call("smn_spr_predict_batch", L.dtype_code(dtype), L.NET_MLP, L.ACT["relu"], 2, nprob, arr([1.0, 1.3, 1.6]),
                 arr([0.2, 0.4, 0.1]), arr([0.9, 1.0, 1.1]), xw.ptr, n, xw.ld, xtw.ptr, t, xtw.ld, D, yd.ptr, c,
                 arr([1e-2, 2e-2, 3e-2]), arr([1e-3, 0.0, 1e-2]), mean.ptr, cov.ptr, ldcov, var.ptr, quad, logdet, info)
        assert list(info) == [0] * nprob
        return mean.result("mean_d"), cov.result("cov_d"), var.result("var_d"), list(quad) + list(logdet)

    want = run(None)
    assert all(np.isfinite(w).all() for w in want[:3])
    for layout in BOTH:
        got = run(layout)
        for g, w, nm in zip(got[:3], want[:3], ("mean", "cov", "var")):
            assert_same_bits(g, w, "smn_spr_predict_batch %s %s" % (nm, layout))
        assert_same_scalars(got[3], want[3], "smn_spr_predict_batch scalars %s" % layout)


# ----------------------------------------------------------------------------- gradient and leave-one-out entries
def _posterior(n, c, dtype, seed):
    """k0 = x x^T / d, its diagonal, a symmetric -K~^-1 and A = K~^-1 Y of a well conditioned K~ (fp64 NumPy, rounded)."""
    x, y, k = _kernel_like(n, np.float64, seed, c)
    kt = k + 0.1 * np.eye(n)
    kinv = np.linalg.inv(kt)
    kinv = 0.5 * (kinv + kinv.T)
    k0 = x @ x.T / D
    return x.astype(dtype), y.astype(dtype), k0.astype(dtype), np.diag(k0).astype(dtype), (-kinv).astype(dtype), (kinv @ y).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [0, 3])                 # 0: smn_lml_grad_terms; 3: smn_lml_grad_terms_multi
@pytest.mark.parametrize("net,act,layers", [("mlp", "relu", 2), ("resnet", "erf", 1)])
def test_lml_grad_terms(L, ctx, dtype, c, net, act, layers):
    n = 129
    _, _, k0, q, nkinv, alpha = _posterior(n, max(c, 1), dtype, 3)

    def run(layout):
        k0w, kiw = in_buf(ctx, layout, k0), in_buf(ctx, layout, nkinv)
        qd, ad = ctx.to_device(q), ctx.to_device(alpha)
        terms = (C.c_double * 4)()
        if c == 0:
            ctx.call("smn_lml_grad_terms", L.dtype_code(dtype), *_net(L, net, act, layers), k0w.ptr, n, k0w.ld, qd.ptr, kiw.ptr,
                     kiw.ld, ad.ptr, 1.7, terms)
        else:
            ctx.call("smn_lml_grad_terms_multi", L.dtype_code(dtype), *_net(L, net, act, layers), k0w.ptr, n, k0w.ld, qd.ptr,
                     kiw.ptr, kiw.ld, ad.ptr, c, 1.7, terms)
        return list(terms)

    want = run(None)
    assert np.isfinite(want).all()
    for layout in BOTH:
        assert_same_scalars(run(layout), want, "lml_grad_terms c=%d %s" % (c, layout))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [0, 3])                 # 0: smn_kernel_cnn_grad_terms; 3: its _multi form
def test_kernel_cnn_grad_terms(L, ctx, dtype, c):
    n, shape = 129, (129, 6, 6, 2)
    _, _, _, _, nkinv, alpha = _posterior(n, max(c, 1), dtype, 4)
    nkinv = _nan_above_diagonal(nkinv)                 # the lower triangle is read
    x = np.random.default_rng(5).standard_normal(shape).astype(dtype)

    def run(layout):
        xw, kiw = images_buf(ctx, layout, x), in_buf(ctx, layout, nkinv)
        ad = ctx.to_device(alpha)
        terms = (C.c_double * 4)()
        head = (L.dtype_code(dtype), L.ACT["relu"], 2) + HYP + (xw.ptr, n) + shape[1:] + (kiw.ptr, kiw.ld, ad.ptr)
        if c == 0:
            ctx.call("smn_kernel_cnn_grad_terms", *head, 1.7, terms)
        else:
            ctx.call("smn_kernel_cnn_grad_terms_multi", *head, c, 1.7, terms)
        return list(terms)

    want = run(None)
    assert np.isfinite(want).all()
    for layout in BOTH:
        assert_same_scalars(run(layout), want, "kernel_cnn_grad_terms c=%d %s" % (c, layout))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [1, 3])
def test_spr_kinv(L, ctx, dtype, c):
    """The header ties ldkinv to a multiple of 16 bytes: the -K~^-1 output takes the aligned layout; x takes both."""
    n = 129
    x, y, _ = _kernel_like(n, dtype, 6, c)

    def run(layout):
        xw = in_buf(ctx, layout, x)
        yd = ctx.to_device(y)
        if layout is None:       # the contiguous call: an exactly sized matrix whose rows are a multiple of 16 bytes
            al = 16 // np.dtype(dtype).itemsize
            nk = out_buf(ctx, "aligned", n, n, dtype, 1, ld=(n + al - 1) // al * al, col_off=0, rows_before=0)
        else:
            nk = out_buf(ctx, "aligned", n, n, dtype, 1)
        a = out_buf(ctx, None if layout is None else "block", n, c, dtype, 2)
        logdet, info = C.c_double(), C.c_int(-1)
        ctx.call("smn_spr_kinv", L.dtype_code(dtype), *_net(L, "mlp", "relu", 2), xw.ptr, n, xw.ld, D, yd.ptr, c, 0.1, nk.ptr, nk.ld,
                 a.ptr, C.byref(logdet), C.byref(info))
        assert info.value == 0
        return np.tril(nk.result("neg_kinv")), a.result("alpha"), logdet.value     # the lower triangle is valid

    want = run(None)
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
    for layout in BOTH:
        nk, a, ld = run(layout)
        assert_same_bits(nk, want[0], "smn_spr_kinv -K~^-1 %s" % layout)
        assert_same_bits(a, want[1], "smn_spr_kinv A %s" % layout)
        assert_same_scalars(ld, want[2], "smn_spr_kinv logdet")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c,df", [(1, 0.0), (3, 5.0)])
def test_loo_head(L, ctx, dtype, c, df):
    n = 129
    _, y, _, _, nkinv, alpha = _posterior(n, c, dtype, 8)
    nkinv = _nan_above_diagonal(nkinv)                 # only the lower triangle is read
    low = np.tril(np.ones((n, n), bool))

    def run(layout):
        kiw = in_buf(ctx, layout, nkinv)
        ad, yd = ctx.to_device(alpha), ctx.to_device(y)
        blk = None if layout is None else "block"
        mean = out_buf(ctx, blk, n, c, dtype, 1)
        s2 = out_buf(ctx, blk, 1, n, dtype, 2)
        g = out_buf(ctx, layout, n, n, dtype, 3)
        lam, dh = C.c_double(), (C.c_double * 2)()
        ctx.call("smn_loo_head", L.dtype_code(dtype), kiw.ptr, kiw.ld, ad.ptr, yd.ptr, n, c, df, 1.5, C.byref(lam), mean.ptr, s2.ptr,
                 dh, g.ptr, g.ld)
        return mean.result("loo_mean"), s2.result("loo_scale2"), np.where(low, g.result("seed G"), 0), [lam.value] + list(dh)

    want = run(None)
    assert all(np.isfinite(np.asarray(w)).all() for w in want)
    for layout in BOTH:
        got = run(layout)
        for gg, w, nm in zip(got[:3], want[:3], ("mean", "scale2", "G")):
            assert_same_bits(gg, w, "smn_loo_head %s %s" % (nm, layout))
        assert_same_scalars(got[3], want[3], "smn_loo_head scalars %s" % layout)


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_cnn_input_grad(L, ctx, dtype):
    n, n_grad, shape = 129, 5, (129, 6, 6, 2)
    rng = np.random.default_rng(9)
    x = rng.standard_normal(shape).astype(dtype)
    gbar = rng.standard_normal((n, n))
    gbar = _nan_above_diagonal(gbar + gbar.T).astype(dtype)          # only the lower triangle is read

    def run(layout):
        xw, gw = images_buf(ctx, layout, x), in_buf(ctx, layout, gbar)
        gx = out_buf(ctx, None if layout is None else "block", n_grad, int(np.prod(shape[1:])), dtype, 1)
        ctx.call("smn_kernel_cnn_input_grad", L.dtype_code(dtype), L.ACT["erf"], 2, *HYP, xw.ptr, n, *shape[1:], gw.ptr, gw.ld, n_grad,
                 gx.ptr)
        return gx.result("gx")

    want = run(None)
    assert np.isfinite(want).all()
    for layout in BOTH:
        assert_same_bits(run(layout), want, "smn_kernel_cnn_input_grad %s" % layout)


# ----------------------------------------------------------------------------- leading dimensions that are too small
def test_too_small_leading_dimensions_are_refused(L, ctx):
    """One call per entry and per leading-dimension argument with ld = extent - 1: SMN_EINVAL and a message that names the
    argument.  Every buffer is allocated for the natural layout, so a library without the check would alias rows inside its
    own buffers and never leave them."""
    n, t, c, d, nprob = 8, 3, 2, 4, 2
    H = Wd = 8
    Ch = 1
    rng = np.random.default_rng(0)
    pool = lambda: ctx.to_device(0.5 + rng.random(1 << 17))     # noqa: E731  1 MiB of fp64: larger than any operand below
    x, xt, y, k, k2, o1, o2, o3, q, stage = (pool() for _ in range(10))
    f64 = L.F64
    net = (L.NET_MLP, L.ACT["relu"], 1) + HYP
    conv = (L.ACT["relu"], 1) + HYP
    dbl = lambda *v: (C.c_double * len(v))(*v)   # noqa: E731
    ones = dbl(*([1.0] * nprob))
    sc = [C.c_double() for _ in range(8)]
    r = [C.byref(s) for s in sc]
    info, infos = C.c_int(), (C.c_int * nprob)()
    ri = C.byref(info)
    terms, dh, outs = (C.c_double * 8)(), (C.c_double * 2)(), (C.c_double * 8)()
    labels = (C.c_int * t)(0, 1, 0)
    cols1 = (C.c_int64 * 2)(0, 1)
    I, B = 4, 3

    def mlp(ldx1, ldx2, ldk, cross=True):
        return ("smn_kernel_mlp", f64) + net + (x.ptr, n, ldx1, xt.ptr if cross else None, t if cross else 0, ldx2, d, L.GET_NNGP,
                                                L.FILL_FULL, o1.ptr, None, ldk)

    def gram(ldx1, ldx2, ldk, cross=True):
        return ("smn_gram", f64, x.ptr, n, ldx1, xt.ptr if cross else None, t if cross else 0, ldx2, d, o1.ptr, ldk, o2.ptr,
                o3.ptr if cross else None)

    def rows(entry, ldx, ldk):
        return (entry, f64) + net + (x.ptr, n, ldx, d, 2, 6, L.GET_NNGP, o1.ptr, None, ldk)

    def predict(ldk, ldcov):
        return ("smn_predict", f64, k.ptr, n, t, ldk, y.ptr, c, 0.0, 0.1, o1.ptr, o2.ptr, ldcov, outs, r[0], ri)

    def spr_predict(ldx, ldxt, ldcov):
        return ("smn_spr_predict", f64) + net + (x.ptr, n, ldx, xt.ptr, t, ldxt, d, y.ptr, c, 0.0, 0.1, o1.ptr, o2.ptr, ldcov, outs,
                                                 r[0], ri)

    def spr_predict_batch(ldx, ldxt, ldcov):
        return ("smn_spr_predict_batch", f64, net[0], net[1], net[2], nprob, ones, ones, ones, x.ptr, n, ldx, xt.ptr, t, ldxt, d,
                y.ptr, c, ones, ones, o1.ptr, o2.ptr, ldcov, o3.ptr, outs, dbl(0, 0), infos)

    def grad_terms(ldk0, ldkinv, multi=False):
        tail = (c, 1.0, terms) if multi else (1.0, terms)
        return ("smn_lml_grad_terms_multi" if multi else "smn_lml_grad_terms", f64) + net + (k.ptr, n, ldk0, q.ptr, k2.ptr, ldkinv,
                                                                                                y.ptr) + tail

    def cnn_terms(ldkinv, multi=False):
        tail = (c, 1.0, terms) if multi else (1.0, terms)
        return ("smn_kernel_cnn_grad_terms_multi" if multi else "smn_kernel_cnn_grad_terms", f64) + conv + (
            x.ptr, n, H, Wd, Ch, k2.ptr, ldkinv, y.ptr) + tail

    def loo_head(ldkinv, ldg):
        return ("smn_loo_head", f64, k2.ptr, ldkinv, y.ptr, y.ptr, n, c, 0.0, 1.0, r[0], o1.ptr, o2.ptr, dh, o3.ptr, ldg)

    def loo_multi(ldk, ldg):
        return ("smn_loo_multi", f64, k.ptr, n, ldk, y.ptr, c, 0.1, 0.0, 1.0, r[0], o1.ptr, o2.ptr, dh, r[1], ri, o3.ptr, ldg)

    def kinv(ldx, ldkinv):
        return ("smn_spr_kinv", f64) + net + (x.ptr, n, ldx, d, y.ptr, c, 0.1, o1.ptr, ldkinv, o2.ptr, r[0], ri)

    def elbo(ldk, ldg):
        return ("smn_svsp_elbo_grad", f64, k.ptr, ldk, I, B, 2, q.ptr, q.ptr, 1e-3, 1.0, 100.0, labels, 4, 0.0, 1.0, 1, 0, None, None,
                r[0], r[1], o1.ptr, o2.ptr, r[2], r[3], r[4], r[5], o3.ptr, ldg, ri)

    loss_tail = (y.ptr, 0.1, 0.0, 1.0)
    calls = [
        ("ldx1", mlp(d - 1, d, t)), ("ldx2", mlp(d, d - 1, t)), ("ldk", mlp(d, d, t - 1)), ("ldk", mlp(d, 0, n - 1, cross=False)),
        ("ldx", rows("smn_kernel_mlp_rows", d - 1, n)), ("ldk", rows("smn_kernel_mlp_rows", d, n - 1)),
        ("ldx", rows("smn_kernel_mlp_lower_rows", d - 1, n)), ("ldk", rows("smn_kernel_mlp_lower_rows", d, 5)),
        ("ldx", ("smn_kernel_mlp_shard", f64) + net + (x.ptr, n, d - 1, d, 1, 0, 128, L.GET_NNGP, stage.ptr, None)),
        ("ldx", ("smn_kernel_mlp_shard_cols", f64) + net + (x.ptr, n, d - 1, d, 1, 0, 1, cols1, L.GET_NNGP, stage.ptr, None)),
        ("ldx1", gram(d - 1, d, t)), ("ldx2", gram(d, d - 1, t)), ("ldk", gram(d, d, t - 1)), ("ldk", gram(d, 0, n - 1, cross=False)),
        ("ldk0", ("smn_recursion", f64) + net + (k.ptr, n, n, n - 1, q.ptr, q.ptr, 1, L.GET_NNGP, o1.ptr, None, n)),
        ("ldk", ("smn_recursion", f64) + net + (k.ptr, n, n, n, q.ptr, q.ptr, 1, L.GET_NNGP, o1.ptr, None, n - 1)),
        ("ldk", ("smn_kernel_cnn", f64) + conv + (x.ptr, n, None, 0, H, Wd, Ch, L.FILL_FULL, o1.ptr, n - 1)),
        ("ldk", ("smn_kernel_cnn", f64) + conv + (x.ptr, n, xt.ptr, t, H, Wd, Ch, L.FILL_FULL, o1.ptr, t - 1)),
        ("ldk", ("smn_kernel_conv_resnet", f64) + conv + (x.ptr, n, None, 0, H, Wd, Ch, L.FILL_FULL, o1.ptr, n - 1)),
        ("ldk", ("smn_kernel_conv_resnet", f64) + conv + (x.ptr, n, xt.ptr, t, H, Wd, Ch, L.FILL_FULL, o1.ptr, t - 1)),
        ("lda", ("smn_cholesky", f64, k.ptr, n, n, n - 1, 0, 0.0, 0.0, ri, r[0])),
        ("ldl", ("smn_trsm", f64, k.ptr, n, n - 1, o1.ptr, c, c, 0)), ("ldb", ("smn_trsm", f64, k.ptr, n, n, o1.ptr, c, c - 1, 0)),
        ("lds", ("smn_transpose", f64, o1.ptr, n, k.ptr, t - 1, n, t)), ("ldd", ("smn_transpose", f64, o1.ptr, n - 1, k.ptr, t, n, t)),
        ("ldk", ("smn_lml", f64, k.ptr, n, n - 1, y.ptr, 0.1, 0.0, 1.0, r[0], r[1], r[2], ri)),
        ("ldk", ("smn_lml_multi", f64, k.ptr, n, n - 1, y.ptr, c, 0.1, 0.0, 1.0, r[0], r[1], outs, r[2], ri)),
        ("ldk", predict(n + t - 1, t)), ("ldcov", predict(n + t, t - 1)),
        ("ldx", ("smn_spr_loss", f64) + net + (x.ptr, n, d - 1, d) + loss_tail + (r[0], r[1], r[2], ri)),
        ("ldx", ("smn_spr_loss_multi", f64) + net + (x.ptr, n, d - 1, d, y.ptr, c, 0.1, 0.0, 1.0, r[0], r[1], outs, r[2], ri)),
        ("ldx", spr_predict(d - 1, d, t)), ("ldxt", spr_predict(d, d - 1, t)), ("ldcov", spr_predict(d, d, t - 1)),
        ("ldx", ("smn_spr_loss_batch", f64, net[0], net[1], net[2], nprob, ones, ones, ones, x.ptr, n, d - 1, d, y.ptr, ones, None, None,
                 outs, None, None, infos)),
        ("ldx", spr_predict_batch(d - 1, d, t)), ("ldxt", spr_predict_batch(d, d - 1, t)), ("ldcov", spr_predict_batch(d, d, t - 1)),
        ("ldk0", grad_terms(n - 1, n)), ("ldkinv", grad_terms(n, n - 1)),
        ("ldk0", grad_terms(n - 1, n, True)), ("ldkinv", grad_terms(n, n - 1, True)),
        ("ldx", ("smn_spr_loss_grad", f64) + net + (x.ptr, n, d - 1, d) + loss_tail + (r[0], r[1], ri, terms)),
        ("ldx", ("smn_spr_loss_grad_multi", f64) + net + (x.ptr, n, d - 1, d, y.ptr, c, 0.1, 0.0, 1.0, r[0], outs, r[1], ri, terms)),
        ("ldx", ("smn_spr_loss_grad_batch", f64, net[0], net[1], net[2], nprob, ones, ones, ones, x.ptr, n, d - 1, d, y.ptr, ones, None,
                 None, None, None, infos, terms)),
        ("ldkinv", cnn_terms(n - 1)), ("ldkinv", cnn_terms(n - 1, True)),
        ("ldkinv", loo_head(n - 1, n)), ("ldg", loo_head(n, n - 1)),
        ("ldk", loo_multi(n - 1, n)), ("ldg", loo_multi(n, n - 1)),
        ("ldx", ("smn_spr_loo_grad", f64) + net + (x.ptr, n, d - 1, d, y.ptr, c, 0.1, 0.0, 1.0, r[0], dh, ri, terms, o1.ptr, o2.ptr)),
        ("ldx", kinv(d - 1, n)), ("ldkinv", kinv(d, n - 2)),            # (n - 2: a multiple of 16 bytes, so the size is what refuses it)
        ("ldk", elbo(I + B - 1, I + B)), ("ldg", elbo(I + B, I + B - 1)),
        ("ldg", ("smn_kernel_cnn_input_grad", f64) + conv + (x.ptr, n, H, Wd, Ch, k2.ptr, n - 1, 2, o1.ptr)),
        ("ldk", ("smn_unpack_lower_blocks", f64, stage.ptr, n, 1, 128, o1.ptr, n - 1)),
        ("ldk", ("smn_shard_exchange_cols_to", f64, stage.ptr, stage.ptr, n, 1, 1, cols1, 0, o1.ptr, n - 1)),
        ("ldk", ("smn_shard_scatter_cols", f64, stage.ptr, n, 1, 1, cols1, 0, o1.ptr, n - 1)),
    ]
    for arg, call in calls:
        with pytest.raises(L.SmnError) as e:
            ctx.call(*call)
        msg = str(e.value).split(call[0] + ":", 1)[-1].strip()      # what smn_last_error returned
        assert e.value.code == L.EINVAL, (call[0], arg, str(e.value))
        assert msg and (arg + " =") in msg, (call[0], arg, str(e.value))
