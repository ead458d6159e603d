"""The Gram cache of smn_spr_loss (kernel_build.hip gram_cache_plan / build_acc_kernel, include/smnngp.h): from the second
call on one x the context keeps the raw MFMA accumulators of x x^T and later calls run the layer recursion over them.  Every
result here is compared with `==` against a FRESH context (its first call: the fused build, cache never warm) on the same
inputs, and smn_gram_cache_stats proves which path ran."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# one shape with n % 128 != 0 and d % 32 != 0 (210 half tiles), one above the look-ahead threshold (split build, 128-row tiles)
SHAPES = [(2500, 50), (14400, 48)]
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture()
def ctx(L):
    c = L.Context()
    yield c
    c.close()


def spr_loss(L, ctx, x, y, net="mlp", act="relu", depth=2, w=1.0, b=0.3, lw=1.0, eps=1e-2, df=0.0, scale=1.0):
    lp, quad, logdet, info = C.c_double(), C.c_double(), C.c_double(), C.c_int()
    n, d = x.shape
    ctx.call("smn_spr_loss", x.dcode, L.NET_MLP if net == "mlp" else L.NET_DENSE_RESNET, L.ACT[act], depth, w, b, lw, x.ptr, n, d, d,
             y.ptr, eps, df, scale, C.byref(lp), C.byref(quad), C.byref(logdet), C.byref(info))
    return lp.value, quad.value, logdet.value, info.value


def cold(L, xh, yh, **kw):
    """The same call as the first call of a context of its own."""
    c = L.Context()
    try:
        x, y = c.to_device(xh), c.to_device(yh)
        out = spr_loss(L, c, x, y, **kw)
        del x, y
        return out
    finally:
        c.close()


def stats(ctx):
    h, m, b = C.c_int64(), C.c_int64(), C.c_size_t()
    ctx.call("smn_gram_cache_stats", C.byref(h), C.byref(m), C.byref(b))
    return h.value, m.value, b.value


def same(a, b):
    """tuples of (logpdf, quad, logdet, info) with NaN == NaN"""
    return np.array_equal(np.array(a), np.array(b), equal_nan=True)


def data(dtype, n, d, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)).astype(dtype), rng.standard_normal((n, 1)).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d", SHAPES)
def test_every_hyper_parameter_moves_over_one_cached_gram(L, ctx, dtype, n, d):
    """Five calls on one x, each with its own (net, act, depth, w_std, b_std, last_w_std, eps, df, y): every call equals the
    cold result for its own parameters, and from the third on they are cache hits."""
    xh, yh = data(dtype, n, d, 31)
    y2h = (yh * 0.5 + 1.0).astype(dtype)
    x, y, y2 = ctx.to_device(xh), ctx.to_device(yh), ctx.to_device(y2h)
    calls = [
        dict(net="mlp", act="relu", depth=2, w=1.0, b=0.3, lw=1.0, eps=1e-2),
        dict(net="mlp", act="erf", depth=3, w=1.3, b=0.1, lw=0.7, eps=3e-2),
        dict(net="resnet", act="relu", depth=1, w=0.9, b=0.2, lw=1.1, eps=1e-1, df=4.0, scale=1.5),
        dict(net="mlp", act="relu", depth=4, w=1.2, b=0.0, lw=1.0, eps=5e-2),
        dict(net="resnet", act="erf", depth=2, w=1.1, b=0.4, lw=0.9, eps=2e-2),
    ]
    for i, kw in enumerate(calls):
        yy, yyh = (y2, y2h) if i % 2 else (y, yh)
        got = spr_loss(L, ctx, x, yy, **kw)
        ref = cold(L, xh, yyh, **kw)
        assert ref[3] == 0, (i, ref)
        assert same(got, ref), (i, got, ref)
    hits, misses, nbytes = stats(ctx)
    assert hits >= 3 and misses == 2 and nbytes > 0, (hits, misses, nbytes)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d", SHAPES)
def test_an_element_overwritten_in_place_is_seen(L, ctx, dtype, n, d):
    """One element of x rewritten in the same buffer between calls (also: -0.0 for +0.0, a bit pattern apart and nothing else):
    the result of a cold context on the new x, a miss; unchanged again: a hit."""
    xh, yh = data(dtype, n, d, 32)
    xh[n // 2, 1] = 0.0
    x, y = ctx.to_device(xh), ctx.to_device(yh)
    for _ in range(3):
        warm = spr_loss(L, ctx, x, y)
    h0, m0, _ = stats(ctx)
    assert h0 == 1 and same(warm, cold(L, xh, yh))
    es = np.dtype(dtype).itemsize
    for (r, c, v) in [(n - 1, d - 1, 2.5), (n // 2, 1, -0.0)]:
        xh[r, c] = v
        one = np.array([v], dtype=dtype)
        ctx.call("smn_memcpy_h2d", C.c_void_p(x.ptr.value + es * (r * d + c)), one.ctypes.data_as(C.c_void_p), es)
        h1, m1, _ = stats(ctx)
        got = spr_loss(L, ctx, x, y)
        h2, m2, _ = stats(ctx)
        assert (h2, m2) == (h1, m1 + 1), (h1, m1, h2, m2)
        assert same(got, cold(L, xh, yh)), (r, c, v)
        again = spr_loss(L, ctx, x, y)       # the accumulators of the new x are stored by this call
        assert same(again, got)
        h3, m3, _ = stats(ctx)
        assert same(spr_loss(L, ctx, x, y), got)
        assert stats(ctx)[:2] == (h3 + 1, m3)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_freed_and_reallocated_x_is_compared_by_content(L, ctx, dtype):
    """x freed and another array of the same shape allocated -- usually at the same address: a pointer proves nothing."""
    n, d = SHAPES[0]
    xh, yh = data(dtype, n, d, 33)
    x, y = ctx.to_device(xh), ctx.to_device(yh)
    for _ in range(3):
        spr_loss(L, ctx, x, y)
    assert stats(ctx)[0] == 1
    old_ptr = x.ptr.value
    del x
    x2h = data(dtype, n, d, 34)[0]
    x2 = ctx.to_device(x2h)
    print("re-allocated x at the same address: %s" % (x2.ptr.value == old_ptr))
    got = spr_loss(L, ctx, x2, y)
    assert stats(ctx)[0] == 1                # not a hit
    assert same(got, cold(L, x2h, yh))
    del x2
    x3 = ctx.to_device(x2h)                  # the same content in yet another allocation: a hit once the accumulators are stored
    assert same(spr_loss(L, ctx, x3, y), got)
    assert same(spr_loss(L, ctx, x3, y), got)
    assert stats(ctx)[0] == 2


def test_other_shapes_dtypes_and_entry_points_between_two_calls(L, ctx):
    """Interleaved shapes and dtypes start cold for their own key; smn_spr_predict, smn_kernel_mlp and smn_spr_loss_batch on
    other inputs (they rewrite workspace slots 0-3) between two loss calls leave the cache alone: the second is a hit."""
    (n, d), (n2, d2) = SHAPES[0], (2700, 40)
    xh, yh = data(np.float32, n, d, 35)
    ah, bh = data(np.float64, n2, d2, 36)
    x, y, a, b = ctx.to_device(xh), ctx.to_device(yh), ctx.to_device(ah), ctx.to_device(bh)
    ref_x, ref_a = cold(L, xh, yh), cold(L, ah, bh)
    for _ in range(2):                       # alternating keys: every call starts cold, every result is the cold one
        assert same(spr_loss(L, ctx, x, y), ref_x)
        assert same(spr_loss(L, ctx, a, b), ref_a)
    assert stats(ctx)[0] == 0
    for _ in range(3):
        assert same(spr_loss(L, ctx, x, y), ref_x)
    h0, m0, _ = stats(ctx)
    assert h0 == 1
    # other entry points on other inputs
    oh, ph = data(np.float32, 900, d, 37)
    th = data(np.float32, 64, d, 38)[0]
    o, p, t = ctx.to_device(oh), ctx.to_device(ph), ctx.to_device(th)
    mean, cov = ctx.empty((64, 1), np.float32), ctx.empty((64, 64), np.float32)
    quad, logdet, info = C.c_double(), C.c_double(), C.c_int()
    ctx.call("smn_spr_predict", L.F32, L.NET_MLP, L.ACT["relu"], 2, 1.0, 0.3, 1.0, o.ptr, 900, d, t.ptr, 64, d, d, p.ptr, 1, 1e-3, 0.0,
             mean.ptr, cov.ptr, 64, C.byref(quad), C.byref(logdet), C.byref(info))
    assert info.value == 0
    k = ctx.empty((900, 900), np.float32)
    ctx.call("smn_kernel_mlp", L.F32, L.NET_MLP, L.ACT["erf"], 2, 1.0, 0.3, 1.0, o.ptr, 900, d, None, 0, 0, d, L.GET_NNGP, L.FILL_FULL,
             k.ptr, None, 900)
    nb = 3
    arr = lambda v: (C.c_double * nb)(*v)
    lps, infos = (C.c_double * nb)(), (C.c_int * nb)()
    ctx.call("smn_spr_loss_batch", L.F32, L.NET_MLP, L.ACT["relu"], 2, nb, arr([1.0, 1.1, 1.2]), arr([0.1, 0.2, 0.3]), arr([1.0] * nb),
             o.ptr, 900, d, d, p.ptr, arr([1e-2] * nb), None, None, lps, None, None, infos)
    assert list(infos) == [0] * nb
    assert same(spr_loss(L, ctx, x, y), ref_x)
    assert stats(ctx)[:2] == (h0 + 1, m0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d", SHAPES)
def test_a_failed_factorisation_on_a_cached_call_leaves_the_context_usable(L, ctx, dtype, n, d):
    """eps = -5 (info != 0; above the look-ahead threshold the factorisation gives up while the corner is still in flight) on a
    cached call, then a good call: equal to cold."""
    xh, yh = data(dtype, n, d, 39)
    x, y = ctx.to_device(xh), ctx.to_device(yh)
    ref = cold(L, xh, yh)
    for _ in range(3):
        assert same(spr_loss(L, ctx, x, y), ref)
    bad = spr_loss(L, ctx, x, y, eps=-5.0)
    assert bad[3] != 0 and np.isnan(bad[0])
    assert same(bad, cold(L, xh, yh, eps=-5.0))
    assert same(spr_loss(L, ctx, x, y), ref)
    assert stats(ctx)[0] >= 2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d", SHAPES)
def test_the_two_switches_bypass_the_cache_with_the_same_bits(L, ctx, dtype, n, d):
    xh, yh = data(dtype, n, d, 40)
    x, y = ctx.to_device(xh), ctx.to_device(yh)
    ref = cold(L, xh, yh)
    for _ in range(3):
        assert same(spr_loss(L, ctx, x, y), ref)
    h0, m0, b0 = stats(ctx)
    assert h0 == 1 and b0 > 0
    try:
        ctx.call("smn_debug_split_build", 0)     # one build launch with the chip to itself: bypassed, not dropped
        assert same(spr_loss(L, ctx, x, y), ref)
        assert same(spr_loss(L, ctx, x, y), ref)
    finally:
        ctx.call("smn_debug_split_build", 1)
    assert stats(ctx) == (h0, m0, b0)
    assert same(spr_loss(L, ctx, x, y), ref)
    assert stats(ctx)[:2] == (h0 + 1, m0)
    try:
        ctx.call("smn_debug_gram_cache", 0)      # bypassed and dropped
        assert stats(ctx)[2] == 0
        assert same(spr_loss(L, ctx, x, y), ref)
        assert stats(ctx) == (h0 + 1, m0, 0)
    finally:
        ctx.call("smn_debug_gram_cache", 1)
    for _ in range(3):
        assert same(spr_loss(L, ctx, x, y), ref)
    assert stats(ctx)[:2] == (h0 + 2, m0 + 2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_small_problems_keep_the_fused_path(L, ctx, dtype):
    """Below 2560 padded rows (kernel_build.hip kGramCacheMinRows) nothing is kept."""
    for n, d in [(245, 6), (2048, 64), (2304, 3072 if dtype == np.float32 else 128)]:
        xh, yh = data(dtype, n, d, 41)
        x, y = ctx.to_device(xh), ctx.to_device(yh)
        outs = [spr_loss(L, ctx, x, y) for _ in range(3)]
        assert outs[0][3] == 0 and same(outs[1], outs[0]) and same(outs[2], outs[0])
        assert stats(ctx) == (0, 0, 0)
