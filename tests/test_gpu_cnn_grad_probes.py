"""The image-pair contraction of csrc/cnn_grad.hip (cgrad_pair_kernel<T, ACT, NP, EXACT, MULTI>, its per-image tables
cgrad_q_kernel, the pair walk and the reduction) held PAIR BY PAIR to a high-precision reference, in f32 and f64, relu and erf.

smn_kernel_cnn_grad_terms and smn_kernel_cnn_grad_terms_multi take any matrix as neg_kinv_d.  A seed that is zero except
G[n,m] = g (m <= n), with alpha = 0 and coef = 0, returns terms[0..2] = m g dK~_nm / d{w_std, b_std, last_w_std} (m = 2 off the
diagonal, 1 on it) and terms[3] = g [n == m]: one call reads one image pair's three tangents.  Images are generated in fp64 and
rounded once to the storage type.  The entries above this one (smn_spr_cnn_loss_grad*, smn_spr_cnn_loo_grad) are not probed here:
test_gpu_cnn_grad.py (SPR.loss_and_grad against central differences, the non-PD and b_std == 0 contracts), test_gpu_multi.py and
test_gpu_loo.py (the bit-identity of the fused entries with build + factorisation + this contraction) carry the result to them.

Reference and allowance (tests/_cnn_probe_rules.py, checked on the host by test_cnn_probe_host.py, which also shows that the
allowance rejects seven kinds of slip in a pair kernel):
    ref        the forward-mode rules in np.longdouble on the device's own images (stored in T, widened)
    scale      s_nm = max(|ref_nm|, sqrt(|ref_nn ref_mm|)), per term
    yardstick  Y = max over the probed pairs of |rules_T - ref| / s_nm, per case and term; it comes from the rules alone
    allowance  |device - ref| / s_nm <= 16 max(Y, 4 u_T), every probed pair; no additive term was needed (the exact duplicate
               pair (3, 1) included: the first-order error of a correlation that is 1 only to rounding cancels in the NNGP tangents)
    terms[3]   exactly g (c g for the rank-C form) or 0.0
    dense      a full symmetric seed: each term within 16 max(Y, 4 u) sum_nm m |G_nm| s_nm, the same bits twice
Every case prints its largest error / (max(Y, 4u) s) (run with -s); profiles/r29_cnn_grad_probes.txt holds that table.

Grid of (a), w_std, b_std, last_w_std = 1.3, 0.4, 0.9: five images (0-2 random, 3 a copy of 1, 4 zero outside a central block),
all 15 pairs, through both entries, as H x W x C - layers per form of cgrad_launch (pixels per lane, ragged / exact last lane):
    1 ragged    1x1x3-4  5x7x2-1  6x6x1-2               1 exact     8x8x1-4  1x64x2-2  64x1x3-1
    4 ragged    9x8x2-1  12x12x1-4  3x50x3-2            4 exact     16x16x1-2  4x64x2-4  16x16x3-1
    16 ragged   17x16x2-1  20x20x3-2  31x33x1-4  1x1024x1-2         16 exact   32x32x3-4  16x64x1-1  1024x1x2-2
(b) b_std == 0 on the same five images at 6x6, 8x8, 12x12, 20x20, 32x32 (x1, 2 layers).  (c) n = 160 at 6x6x1 and 32x32x1 (waves
that walk two pairs), n = 1531 at 6x6x1 (the tiled pair order).  (d) rank-C seeds, c = 1, 3, 48.  (e) seeds carried by alpha.
(f) dense seeds at n = 160.  (g) what the entries read."""
import ctypes as C
import functools

import numpy as np
import pytest

import _cnn_probe_rules as P

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]
LD = np.longdouble


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


# ------------------------------------------------------------------------------------------------------ device calls
_DEV = {}


def _dev(ctx, key, make):
    """Device copies shared by the tests of this file (images, zero seeds); never written except through Seed below."""
    if key not in _DEV:
        _DEV[key] = ctx.to_device(np.ascontiguousarray(make()))
    return _DEV[key]


def _terms(L, ctx, T, act, layers, b_std, xd, shape, gd, ld, ad, coef, nc=None):
    """One call of smn_kernel_cnn_grad_terms (nc None) or smn_kernel_cnn_grad_terms_multi."""
    n, h, w, c = shape
    out = (C.c_double * 4)()
    head = (L.dtype_code(T), L.ACT[act], layers, P.W, b_std, P.LW, xd.ptr, n, h, w, c, gd.ptr, ld, ad.ptr)
    if nc is None:
        ctx.call("smn_kernel_cnn_grad_terms", *head, coef, out)
    else:
        ctx.call("smn_kernel_cnn_grad_terms_multi", *head, nc, coef, out)
    return np.array(out[:], np.float64)


class Seed:
    """An n x n device matrix of zeros in which one entry at a time is set and cleared again."""

    def __init__(self, ctx, n, T):
        self.ctx, self.n, self.T = ctx, n, T
        self.d = _dev(ctx, ("seed", n, T), lambda: np.zeros((n, n), T))
        self.zero = np.zeros(1, T)

    def _put(self, i, j, v):
        assert 0 <= i < self.n and 0 <= j < self.n
        p = C.c_void_p(self.d.ptr.value + (i * self.n + j) * self.zero.itemsize)
        self.ctx.call("smn_memcpy_h2d", p, v.ctypes.data_as(C.c_void_p), v.itemsize)

    def probe(self, i, j, g, call):
        self._put(i, j, np.asarray([g], self.T))
        try:
            return call(self.d)
        finally:
            self._put(i, j, self.zero)


def _run_probes(L, ctx, T, key, x, layers, act, b_std, i, j, nc=None):
    """[E, 4]: the four terms of one probe call per pair (i, j), and the seed values g [E]."""
    n = x.shape[0]
    xd = _dev(ctx, ("x",) + key, lambda: x)
    ad = _dev(ctx, ("zeros", n, nc or 1, T), lambda: np.zeros((n, nc or 1), T))
    seed = Seed(ctx, n, T)
    g = P.seed_values(T, len(i))
    out = np.empty((len(i), 4))
    for e in range(len(i)):
        out[e] = seed.probe(int(i[e]), int(j[e]), g[e],
                            lambda gd: _terms(L, ctx, T, act, layers, b_std, xd, x.shape, gd, n, ad, 0.0, nc))
    return out, g


def _hold(tag, T, out, g, i, j, ref, s, y, nc=1):
    ratio, problems = P.check(T, out, g, i, j, ref, s, y, nc)
    at = [int(np.argmax(r)) for r in ratio]
    print("\n[probe] %-44s E %3d  Y/u %s  max err/(max(Y,4u) s) %s  at %s" % (
        tag, len(i), " ".join("%5.1f" % v for v in y / P.U[T]), " ".join("%6.3f" % r.max() for r in ratio),
        " ".join("(%d,%d)" % (i[a], j[a]) for a in at)))
    assert not problems, (tag, problems[:8])
    return ratio.max(axis=1)


@functools.lru_cache(maxsize=None)
def _five_reference(shape, act, b_std, T):
    h, w, c, layers = shape
    return P.reference(P.five_images(h, w, c, T), layers, act, b_std, *P.ALL15, T)


def _name(T):
    return np.dtype(T).name


# ------------------------------------------------------------------------------ a. every pair of five images, every form
@pytest.mark.parametrize("nc", [None, 2], ids=["single", "c2"])
@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("act", P.ACTS)
@pytest.mark.parametrize("shape", P.SHAPES, ids=[P.shape_id(s) for s in P.SHAPES])
def test_every_pair_of_five_images(L, ctx, shape, act, T, nc):
    h, w, c, layers = shape
    i, j = P.ALL15
    ref, s, y = _five_reference(shape, act, P.B, T)
    out, g = _run_probes(L, ctx, T, ("five", h, w, c, T), P.five_images(h, w, c, T), layers, act, P.B, i, j, nc)
    _hold("%s %s %s %s np%d-%s" % ((P.shape_id(shape), act, _name(T), "c=%s" % nc) + P.form_of(h, w)), T, out, g, i, j, ref, s, y,
          nc or 1)


# --------------------------------------------------------------------------------------------------- b. b_std == 0
@pytest.mark.parametrize("nc", [None, 2], ids=["single", "c2"])
@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("act", P.ACTS)
@pytest.mark.parametrize("shape", P.B0_SHAPES, ids=[P.shape_id(s) for s in P.B0_SHAPES])
def test_zero_bias_on_the_zero_border_set(L, ctx, shape, act, T, nc):
    """b_std == 0 exactly: the border pixels of image 4 have zero variance (where ReLU is not differentiable).  terms[1] is exactly
    0.0, everything is finite, terms 0 and 2 within the allowance of the guarded rules."""
    h, w, c, layers = shape
    i, j = P.ALL15
    ref, s, y = _five_reference(shape, act, 0.0, T)
    out, g = _run_probes(L, ctx, T, ("five", h, w, c, T), P.five_images(h, w, c, T), layers, act, 0.0, i, j, nc)
    _hold("b0 %s %s %s %s" % (P.shape_id(shape), act, _name(T), "c=%s" % nc), T, out, g, i, j, ref, s, y, nc or 1)
    assert not out[:, 1].any() and not np.signbit(out[:, 1]).any()


# ------------------------------------------------------------------------------------- c. waves that walk several pairs
@functools.lru_cache(maxsize=None)
def _many_reference(n, shape, act, T, which):
    h, w, c, layers = shape
    i, j = P.walk_pairs() if which == "walk" else P.tiled_pairs()
    return P.reference(P.many_images(n, h, w, c, T), layers, act, P.B, i, j, T)


@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("act", P.ACTS)
@pytest.mark.parametrize("shape", [(6, 6, 1, 2), (32, 32, 1, 2)], ids=["6x6x1-L2", "32x32x1-L2"])
def test_waves_that_walk_two_pairs(L, ctx, shape, act, T):
    """n = 160: 12 880 pairs on the largest plain grid (2048 workgroups), so wave v walks the pairs v and v + 8192; the 48 fixed
    pairs of _cnn_probe_rules.walk_pairs hold both pairs of six waves (state that is not reset between them shows in the second)."""
    h, w, c, layers = shape
    i, j = P.walk_pairs()
    ref, s, y = _many_reference(P.WALK_N, shape, act, T, "walk")
    x = P.many_images(P.WALK_N, h, w, c, T)
    out, g = _run_probes(L, ctx, T, ("many", P.WALK_N, h, w, c, T), x, layers, act, P.B, i, j)
    _hold("walk160 %s %s %s" % (P.shape_id(shape), act, _name(T)), T, out, g, i, j, ref, s, y)


@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("act", P.ACTS)
def test_the_tiled_pair_order(L, ctx, act, T):
    """n = 1531 at 6x6x1 (the shape of test_gpu_cnn_grad's tiled-order test): 32 fixed pairs, references for those alone."""
    shape = (6, 6, 1, 2)
    i, j = P.tiled_pairs()
    ref, s, y = _many_reference(P.TILED_N, shape, act, T, "tiled")
    x = P.many_images(P.TILED_N, 6, 6, 1, T)
    out, g = _run_probes(L, ctx, T, ("many", P.TILED_N, 6, 6, 1, T), x, 2, act, P.B, i, j)
    _hold("tiled1531 %s %s %s" % (P.shape_id(shape), act, _name(T)), T, out, g, i, j, ref, s, y)


# ------------------------------------------------------------------------------------------------ d. the rank-C form
@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("act", P.ACTS)
@pytest.mark.parametrize("nc", [1, 3, 48])
@pytest.mark.parametrize("shape", [(6, 6, 1, 2), (16, 16, 1, 2)], ids=["6x6x1-L2", "16x16x1-L2"])
def test_rank_c_matrix_seed_returns_c_times_the_pair(L, ctx, shape, nc, act, T):
    """smn_kernel_cnn_grad_terms_multi with alpha = 0: g_c = c (-K~^-1)_nm rounded once in T, so every probe returns c m g dK~ and
    terms[3] = c g exactly; c = 1 returns the single-column entry's bits."""
    h, w, c, layers = shape
    i, j = P.ALL15
    ref, s, y = _five_reference(shape, act, P.B, T)
    x = P.five_images(h, w, c, T)
    out, g = _run_probes(L, ctx, T, ("five", h, w, c, T), x, layers, act, P.B, i, j, nc)
    _hold("rankC c=%d %s %s %s" % (nc, P.shape_id(shape), act, _name(T)), T, out, g, i, j, ref, s, y, nc)
    if nc == 1:
        single, _ = _run_probes(L, ctx, T, ("five", h, w, c, T), x, layers, act, P.B, i, j)
        assert single.tobytes() == out.tobytes()


# -------------------------------------------------------------------------------------------- e. seeds carried by alpha
@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("act", P.ACTS)
@pytest.mark.parametrize("nc", [None, 3], ids=["single", "c3"])
@pytest.mark.parametrize("shape", [(6, 6, 1, 2), (16, 16, 1, 2)], ids=["6x6x1-L2", "16x16x1-L2"])
def test_seeds_carried_by_alpha(L, ctx, shape, nc, act, T):
    """neg_kinv = 0, coef = 1, A non-zero in the rows n and m only: G = A A^T has the entries (n,n), (m,m), (n,m) and its mirror;
    the three combine as the rules say, within 16 max(Y, 4u) sum m |G| s.  tr G within (3 + c) u sum |G_ii| (coef = 1 is exact: one
    product and one fused multiply-add per column, in T)."""
    h, w, c, layers = shape
    x = P.five_images(h, w, c, T)
    xd = _dev(ctx, ("x", "five", h, w, c, T), lambda: x)
    zd = _dev(ctx, ("seed", 5, T), lambda: np.zeros((5, 5), T))
    ii, jj = P.ALL15
    ref, s, y = _five_reference(shape, act, P.B, T)
    at = {(int(a), int(b)): e for e, (a, b) in enumerate(zip(ii, jj))}
    yy = np.maximum(y, P.floor(T))
    cols = nc or 1
    worst = 0.0
    for e, (n, m) in enumerate(zip(ii.tolist(), jj.tolist())):
        a = np.zeros((5, cols), T)
        a[n] = P.seed_values(T, cols, 100 + e)
        if m != n:
            a[m] = P.seed_values(T, cols, 200 + e)
        t = _terms(L, ctx, T, act, layers, P.B, xd, x.shape, zd, 5, ctx.to_device(a), 1.0, nc)
        ents = [(n, n)] if m == n else [(n, n), (m, m), (n, m)]
        al = a.astype(LD)
        gm = np.array([(al[p] * al[q]).sum() for p, q in ents])
        mm = np.array([1 if p == q else 2 for p, q in ents], LD)
        idx = [at[p] for p in ents]
        expected = (mm * gm * ref[:, idx]).sum(axis=1)
        bound = (mm * np.abs(gm) * s[:, idx]).sum(axis=1).astype(np.float64)
        err = np.abs(t[:3].astype(LD) - expected).astype(np.float64)
        worst = max(worst, float(np.max(err / (yy * bound))))
        assert np.isfinite(t).all() and (err <= P.FACTOR * yy * bound).all(), (n, m, err / (yy * bound))
        tr = float(sum(v for v, (p, q) in zip(gm, ents) if p == q))
        assert abs(t[3] - tr) <= (3 + cols) * P.U[T] * tr, (n, m, t[3], tr)
    print("\n[alpha] c=%s %s %s %s  max err/(max(Y,4u) sum m|G|s) %.3f" % (nc, P.shape_id(shape), act, _name(T), worst))


# --------------------------------------------------------------------------------------------------- f. dense seeds
def _dense_call(L, ctx, T, shape, act, nc=None, nk=None, ld=None):
    h, w, c, layers = shape
    n = P.DENSE_N
    x = P.many_images(n, h, w, c, T)
    xd = _dev(ctx, ("x", "many", n, h, w, c, T), lambda: x)
    g, a = P.dense_seed(n, T)
    gd = _dev(ctx, ("dense-g", n, T), lambda: g) if nk is None else ctx.to_device(nk)
    ad = _dev(ctx, ("dense-a", n, T), lambda: a)
    return _terms(L, ctx, T, act, layers, P.B, xd, x.shape, gd, ld or n, ad, P.COEF, nc)


@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("act", P.ACTS)
@pytest.mark.parametrize("shape", P.DENSE_SHAPES, ids=[P.shape_id(s) for s in P.DENSE_SHAPES])
def test_dense_seed(L, ctx, shape, act, T):
    """A random symmetric matrix seed and a random alpha (coef = 0.7) at n = 160: every pair, the mirror factor and both reduction
    stages of the realistic call, each term within 16 max(Y, 4u) sum m |G| s.  tr G within (4 u_T + 64 * 2^-53) sum_i (|coef
    alpha_i^2| + |G_ii|): coef, the product and the fused multiply-add round once each in T, and a diagonal term passes fewer than
    64 fp64 additions (its wave's, 32 partials per thread of the second stage, the shuffle tree, the cross-wave sums).  A second call
    returns the same bits; c = 1 of the rank-C form returns the single-column bits."""
    h, w, c, layers = shape
    expected, bound, y = P.dense_reference(h, w, c, layers, act, P.DENSE_N, T)
    t = _dense_call(L, ctx, T, shape, act)
    yy = np.maximum(y, P.floor(T))
    err = np.abs(t[:3].astype(LD) - expected[:3]).astype(np.float64)
    ratio = err / (yy * bound.astype(np.float64))
    print("\n[dense] n=%d %s %s %s  Y/u %s  err/(max(Y,4u) sum m|G|s) %s" % (
        P.DENSE_N, P.shape_id(shape), act, _name(T), " ".join("%5.1f" % v for v in y / P.U[T]), " ".join("%6.3f" % r for r in ratio)))
    assert np.isfinite(t).all() and (ratio <= P.FACTOR).all(), ratio
    g, a = P.dense_seed(P.DENSE_N, T)
    mag = float((LD(P.COEF) * a.astype(LD)[:, 0] ** 2 + np.abs(np.diag(g).astype(LD))).sum())
    assert abs(t[3] - float(expected[3])) <= (4 * P.U[T] + 64 * 2.0 ** -53) * mag, (t[3], expected[3])
    assert _dense_call(L, ctx, T, shape, act).tobytes() == t.tobytes()
    assert _dense_call(L, ctx, T, shape, act, nc=1).tobytes() == t.tobytes()


# ------------------------------------------------------------------------------------------- g. what the entries read
@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("act", P.ACTS)
@pytest.mark.parametrize("nc", [None, 1], ids=["single", "c1"])
def test_what_is_read(L, ctx, nc, act, T):
    """include/smnngp.h at smn_kernel_cnn_grad_terms: neg_kinv_d is read in the lower triangle only -- NaN strictly above the
    diagonal changes no bit -- and through its leading dimension: ldkinv = n + 3 with NaN in the three extra columns changes no bit."""
    shape, n = P.DENSE_SHAPES[0], P.DENSE_N
    clean = _dense_call(L, ctx, T, shape, act, nc)
    g, _ = P.dense_seed(n, T)
    bad = g.copy()
    bad[np.triu_indices(n, 1)] = np.nan
    assert _dense_call(L, ctx, T, shape, act, nc, nk=bad).tobytes() == clean.tobytes()
    wide = np.full((n, n + 3), np.nan, T)
    wide[:, :n] = g
    assert _dense_call(L, ctx, T, shape, act, nc, nk=wide, ld=n + 3).tobytes() == clean.tobytes()
    seed = Seed(ctx, n, T)
    h, w, c, layers = shape
    xd = _dev(ctx, ("x", "many", n, h, w, c, T), lambda: P.many_images(n, h, w, c, T))
    zd = _dev(ctx, ("zeros", n, 1, T), lambda: np.zeros((n, 1), T))
    for i, j in ((0, 1), (3, 100), (0, n - 1), (n - 2, n - 1), (63, 64)):        # a seed above the diagonal returns nothing
        t = seed.probe(i, j, np.asarray(-0.75, T), lambda gd: _terms(L, ctx, T, act, layers, P.B, xd, (n, h, w, c), gd, n, zd, 0.0, nc))
        assert not t.any() and not np.signbit(t).any(), (i, j, t)
