"""The 64 x 64-tile contraction of csrc/grad.hip (grad_contract_tile, grad_contract_tile_ntk, their MULTI forms, the per-row
tables of grad_tables_row) held ENTRY BY ENTRY to a high-precision reference, in f32 and f64, NNGP and NTK.

smn_lml_grad_terms and smn_lml_grad_terms_multi take any matrix as neg_kinv_d.  A seed that is zero except G[i,j] = g (j <= i),
with alpha = 0 and coef = 0, returns terms[0..2] = m g dK~_ij / d{w_std, b_std, last_w_std} (m = 2 off the diagonal, 1 on it) and
terms[3] = g [i == j]: one call reads one entry of the tangent matrices.  k0 and q are built on the host in fp64 and rounded once
to the storage type, so the contraction is the only device arithmetic under test.  The existing bit-identity tests
(test_gpu_grad_batch.py, test_gpu_multi.py, test_gpu_ntk_gp.py) carry the result to the in-place batch form and smn_spr_loss_grad*.

Reference and allowance (tests/_grad_probe_rules.py, checked on the host by test_grad_probe_host.py):
    ref        the forward-mode rules in np.longdouble on the device's own inputs (k0, q in the storage type T, widened)
    scale      s_ij = max(|ref_ij|, sqrt(|ref_ii ref_jj|)), per term
    yardstick  Y = max over the probed entries of |rules_T - ref| / s_ij, per case and term: what a careful libm evaluation in T
               loses; it comes from the reference alone
    allowance  |device - ref| / s_ij <= 16 max(Y, 4 u_T), every entry; 16 is the margin the project gives a device path over a
               same-precision host yardstick (asin_abs, v_rsq-based roots and fused multiply-adds against libm).  One documented
               approximation has its own absolute error added, not a wider factor: the ReLU tangent of Theta between EXACTLY
               duplicate rows off the diagonal, where the device's correlation is 1 only to rounding
               (_grad_probe_rules.duplicate_allowance, ~ sqrt(u) s_ij; here: the all-zero rows under b_std > 0, which are
               duplicates of each other; measured 1.6e-9 s in f64)
    terms[3]   exactly g or 0.0
    dense      a full symmetric seed: each term within 16 max(Y, 4 u) sum_ij m_ij |G_ij| s_ij, the same bits twice
Every case prints its largest error / (max(Y, 4u) s) (run with -s); profiles/r28_grad_probes.txt holds that table.

Cases: the four nets of test_gpu_kernel_budget.NETS (depths 3, 6, 2, 1) at w_std, b_std, last_w_std = 1.4, 0.3, 0.8.  Every lower
entry at n = 65 (one full tile and a 1-wide ragged tile row: every (wave, register-row) slot w + 4 r, both 32-row passes of the
NTK form, the diagonal rule, and entry (64, 64) that every padded lane is clamped to) and at n = 1, 63, 64 for MLP relu; a fixed
selection at n = 200 (10 tiles); the rank-C form; seeds carried by alpha; dense seeds at n = 200 and 1300 (210 tiles); what the
entries read; zero input rows with b_std > 0 and with b_std == 0; nearly duplicate rows."""
import ctypes as C
import functools

import numpy as np
import pytest

import _grad_probe_rules as G

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]
GETS = ["nngp", "ntk"]
FACTOR = 16.0
LD = np.longdouble


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


def _floor(T):
    return 4.0 * G.U[T]


# ------------------------------------------------------------------------------------------------------ device calls
_DEV = {}


def _dev(ctx, key, make):
    """Device copies shared by the tests of this file (inputs, zero seeds); never written except through Seed below."""
    if key not in _DEV:
        _DEV[key] = tuple(ctx.to_device(np.ascontiguousarray(a)) for a in make())
    return _DEV[key]


def _inputs_dev(ctx, kind, n, T, gap=None):
    return _dev(ctx, ("in", kind, n, T, gap), lambda: G.inputs(kind, n, T, gap))


def _terms(L, ctx, T, net, act, layers, get, b_std, k0d, qd, n, gd, ad, coef, c=None):
    """One call of smn_lml_grad_terms (c None) or smn_lml_grad_terms_multi."""
    netc = (L.NET_MLP if net == "mlp" else L.NET_DENSE_RESNET) | (L.NET_NTK if get == "ntk" else 0)
    out = (C.c_double * 4)()
    head = (L.dtype_code(T), netc, L.ACT[act], layers, G.W, b_std, G.LW, k0d.ptr, n, n, qd.ptr, gd.ptr, n, ad.ptr)
    if c is None:
        ctx.call("smn_lml_grad_terms", *head, coef, out)
    else:
        ctx.call("smn_lml_grad_terms_multi", *head, c, coef, out)
    return np.array(out[:], np.float64)


class Seed:
    """An n x n device matrix of zeros in which one entry at a time is set and cleared again."""

    def __init__(self, ctx, n, T):
        self.ctx, self.n, self.T = ctx, n, T
        self.d = ctx.to_device(np.zeros((n, n), T))
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


def _seed_values(T, count, seed=0):
    """Seed values of either sign in [1/2, 3/2), exact in T."""
    rng = np.random.default_rng([count, seed])
    return ((0.5 + rng.random(count)) * np.where(rng.random(count) < 0.5, -1.0, 1.0)).astype(T)


def _run_probes(L, ctx, T, net, act, layers, get, b_std, kind, n, i, j, gap=None, c=None):
    """[E, 4]: the four terms of one probe call per entry (i, j), and the seed values g [E]."""
    k0d, qd = _inputs_dev(ctx, kind, n, T, gap)
    (ad,) = _dev(ctx, ("zeros", n, c or 1, T), lambda: (np.zeros((n, c or 1), T),))
    seed = Seed(ctx, n, T)
    g = _seed_values(T, len(i))
    out = np.empty((len(i), 4))
    for e in range(len(i)):
        out[e] = seed.probe(int(i[e]), int(j[e]), g[e],
                            lambda gd: _terms(L, ctx, T, net, act, layers, get, b_std, k0d, qd, n, gd, ad, 0.0, c))
    return out, g


def _hold(tag, T, out, g, i, j, ref, s, y, extra, nc=1):
    """Every probe within 16 max(Y, 4u) s (+ extra, _grad_probe_rules.duplicate_allowance) of the reference; terms[3] exact.
    Returns the largest (error - extra) / (max(Y, 4u) s) per term."""
    assert np.isfinite(out).all(), tag
    m = np.where(i == j, 1.0, 2.0)
    gl = g.astype(LD)
    gc = (g.dtype.type(nc) * g).astype(np.float64)                    # the rank-C form rounds nc * g once, in T
    assert np.array_equal(out[:, 3], np.where(i == j, gc, 0.0)), tag + ": terms[3]"
    dev = out[:, :3].T.astype(LD) / (nc * m * gl)
    err = np.abs(dev - ref)
    if extra.any():
        with np.errstate(divide="ignore", invalid="ignore"):
            print("\n[dupl]  %-58s exact duplicates off the diagonal: max err/s %s  allowance/s %s (u = %.3g)" % (
                tag, " ".join("%9.3g" % v for v in np.where(extra > 0, err / s, 0).max(axis=1)),
                " ".join("%9.3g" % v for v in np.where(extra > 0, extra / s, 0).max(axis=1)), G.U[T]))
        assert (err <= FACTOR * np.maximum(y, _floor(T))[:, None] * s + extra).all(), tag
        err = np.maximum(err - extra, 0)
    yy = np.maximum(y, _floor(T))[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(s > 0, err / (yy * s), np.where(err == 0, 0.0, np.inf)).astype(np.float64)
    at = [int(np.argmax(r)) for r in ratio]
    print("\n[probe] %-58s E %4d  Y/u %s  max err/(max(Y,4u) s) %s  at %s" % (
        tag, len(i), " ".join("%6.1f" % v for v in y / G.U[T]), " ".join("%6.3f" % r.max() for r in ratio),
        " ".join("(%d,%d)" % (i[a], j[a]) for a in at)))
    assert (err <= FACTOR * yy * s).all(), (tag, ratio.max(axis=1), [(int(i[a]), int(j[a])) for a in at])
    return ratio.max(axis=1)


# ----------------------------------------------------------------------------------------------- 1. entrywise probes
PROBE_CASES = [(cid, kind, n, b, net) for cid, kind, n, _, b, _, nets in G.probe_sets() for net in nets]
_SETS = {cid: e for cid, _, _, _, _, e, _ in G.probe_sets()}


@functools.lru_cache(maxsize=None)
def _reference(net, act, layers, b_std, kind, n, T, get, cid, gap=None):
    i, j = _SETS[cid] if gap is None else (G.DUP_PAIRS + 1, G.DUP_PAIRS)
    k0, q = G.inputs(kind, n, T, gap)
    return G.reference(net, act, layers, b_std, k0, q, i, j, T, get)


@pytest.mark.parametrize("get", GETS)
@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("cid,kind,n,b_std,net", PROBE_CASES, ids=["%s-%s-%s%d" % ((c[0],) + c[4]) for c in PROBE_CASES])
def test_single_entry_probes(L, ctx, cid, kind, n, b_std, net, T, get):
    """all65 / all1 / all63 / all64: every lower entry.  geometry200: the selection of _grad_probe_rules.geometry_entries.  zero65:
    all-zero input rows at 0, 31 and 64 under b_std > 0 (q = b_std^2 there).  zero65-b0: the same under b_std == 0 exactly, where
    the contract of include/smnngp.h holds: every value finite, terms[1] = 0, and exactly nothing from an entry of a zero row."""
    i, j = _SETS[cid]
    ref, s, y, extra = _reference(*net, b_std, kind, n, T, get, cid)
    out, g = _run_probes(L, ctx, T, *net, get, b_std, kind, n, i, j)
    _hold("%s %s-%s%d %s %s" % ((cid,) + net + (get, np.dtype(T).name)), T, out, g, i, j, ref, s, y, extra)
    if b_std == 0.0:
        hit = np.isin(i, G.ZERO_ROWS) | np.isin(j, G.ZERO_ROWS)
        assert not out[:, 1].any() and not out[hit][:, :3].any()


# ------------------------------------------------------------------------------------------------ 2. the rank-C form
@pytest.mark.parametrize("get", GETS)
@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("net", G.NETS, ids=G.NET_IDS)
def test_rank_c_matrix_seed_returns_c_times_the_entry(L, ctx, net, T, get):
    """smn_lml_grad_terms_multi, c = 3, alpha = 0: g_c = c (-K~^-1)_ij, so every probe returns c g (...), terms[3] = c g."""
    i, j = _SETS["all65"]
    ref, s, y, extra = _reference(*net, G.B, "sep", 65, T, get, "all65")
    out, g = _run_probes(L, ctx, T, *net, get, G.B, "sep", 65, i, j, c=3)
    _hold("all65 c=3 %s-%s%d %s %s" % (net + (get, np.dtype(T).name)), T, out, g, i, j, ref, s, y, extra, nc=3)


ALPHA_PAIRS = [(64, 0), (64, 63), (63, 62), (32, 31), (31, 0), (40, 7), (64, 64), (0, 0)] + [(int(a), int(b)) for a, b in zip(
    *np.sort(np.random.default_rng(65).integers(0, 65, size=(2, 24)), axis=0)[::-1])]


def _alpha_seed_check(L, ctx, T, net, get, c):
    """Seeds carried by alpha alone (neg_kinv = 0, coef = 0.7): A has the two non-zero rows (i, j) of a pair, G = coef A A^T has
    the entries (i,i), (j,j), (i,j) and its mirror; against the reference, not against the matrix seeds."""
    n = 65
    net_, act, layers = net
    k0d, qd = _inputs_dev(ctx, "sep", n, T)
    (zd,) = _dev(ctx, ("zeros", n, n, T), lambda: (np.zeros((n, n), T),))
    dg = np.arange(n)
    k0, q = G.inputs("sep", n, T)
    ref_d = G.entry_tangents(net_, act, layers, G.W, G.B, G.LW, k0, q, dg, dg, LD, get)
    rng = np.random.default_rng([c or 0, 11])
    worst = 0.0
    assert len(ALPHA_PAIRS) == 32
    for i, j in ALPHA_PAIRS:
        a = np.zeros((n, c or 1), T)
        a[i] = _seed_values(T, c or 1, int(rng.integers(1 << 30)))
        if j != i:
            a[j] = _seed_values(T, c or 1, int(rng.integers(1 << 30)))
        t = _terms(L, ctx, T, net_, act, layers, get, G.B, k0d, qd, n, zd, ctx.to_device(a), G.COEF, c)
        ei, ej = (np.array([i, j, i]), np.array([i, j, j])) if j != i else (np.array([i]), np.array([i]))
        gm = LD(G.COEF) * (a.astype(LD)[ei] * a.astype(LD)[ej]).sum(axis=1)
        m = np.where(ei == ej, LD(1), LD(2))
        ref = G.entry_tangents(net_, act, layers, G.W, G.B, G.LW, k0, q, ei, ej, LD, get)
        val = G.entry_tangents(net_, act, layers, G.W, G.B, G.LW, k0, q, ei, ej, T, get)
        s = G.scales(ref, ref_d, ei, ej)
        yy = np.maximum(G.yardstick(val, ref, s), _floor(T))
        bound = (m * np.abs(gm) * s).sum(axis=1).astype(np.float64)
        err = np.abs(t[:3].astype(LD) - (m * gm * ref).sum(axis=1)).astype(np.float64)
        worst = max(worst, float(np.max(err / (yy * bound))))
        assert np.isfinite(t).all() and (err <= FACTOR * yy * bound).all(), (i, j, err / (yy * bound))
        # tr G: coef rounded to T, one product and one fused multiply-add per column
        tr, tra = float(gm[ei == ej].sum()), float(np.abs(gm[ei == ej]).sum())
        assert abs(t[3] - tr) <= (3 + (c or 1)) * G.U[T] * tra, (i, j, t[3], tr)
    print("\n[alpha] c=%s %s-%s%d %s %s  max err/(max(Y,4u) bound) %.3f" % ((c,) + net + (get, np.dtype(T).name, worst)))


@pytest.mark.parametrize("get", GETS)
@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("net", G.NETS, ids=G.NET_IDS)
@pytest.mark.parametrize("c", [None, 3], ids=["single", "c3"])
def test_seeds_carried_by_alpha(L, ctx, c, net, T, get):
    _alpha_seed_check(L, ctx, T, net, get, c)


# --------------------------------------------------------------------------------------------------- 3. dense seeds
@functools.lru_cache(maxsize=None)
def _dense_reference(net, act, layers, b_std, n, T, get, kind="sep", keep=None):
    return G.dense_reference(net, act, layers, b_std, n, T, get, kind, None if keep is None else np.array(keep))


def _dense_call(L, ctx, T, net, get, b_std, kind, n, c=None, keep=None, nk=None):
    k0, q = G.inputs(kind, n, T)
    g, a = G.dense_seed(n, T)
    g = g if nk is None else nk
    if c is not None and c > 1:
        a = np.ascontiguousarray(np.stack([np.roll(a, r) for r in range(c)], axis=1))     # [n, c] row-major
    if keep is not None:
        kp = np.array(keep)
        arrs = [np.ascontiguousarray(v) for v in (k0[np.ix_(kp, kp)], q[kp], g[np.ix_(kp, kp)], a[kp])]
        k0d, qd, gd, ad = (ctx.to_device(v) for v in arrs)
        n = len(kp)
    else:
        k0d, qd = _inputs_dev(ctx, kind, n, T)
        gd, ad = _dev(ctx, ("seed", n, T, c), lambda: (G.dense_seed(n, T)[0], a))
        if nk is not None:
            gd = ctx.to_device(g)
    return _terms(L, ctx, T, *net, get, b_std, k0d, qd, n, gd, ad, G.COEF, c)


def _trace_allow(T, n, rows=None):
    g, a = G.dense_seed(n, T)
    mag = LD(G.COEF) * a.astype(LD) ** 2 + np.abs(np.diag(g).astype(LD))
    return (4 * G.U[T] + 16 * 2.0 ** -53) * float((mag if rows is None else mag[list(rows)]).sum())


def _hold_dense(tag, T, t, expected, bound, y):
    yy = np.maximum(y, _floor(T))
    err = np.abs(t[:3].astype(LD) - expected[:3]).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / (yy * bound.astype(np.float64)), np.where(err == 0, 0.0, np.inf))
    print("\n[dense] %-50s Y/u %s  err/(max(Y,4u) sum m|G|s) %s" % (tag, " ".join("%6.1f" % v for v in y / G.U[T]),
                                                                   " ".join("%6.3f" % r for r in ratio)))
    assert np.isfinite(t).all(), tag
    for k in range(3):
        assert err[k] <= FACTOR * yy[k] * float(bound[k]), (tag, k, ratio)
    return ratio


@pytest.mark.parametrize("get", GETS)
@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("net", G.NETS, ids=G.NET_IDS)
@pytest.mark.parametrize("n", G.DENSE_N)
def test_dense_seed(L, ctx, n, net, T, get):
    """A random symmetric matrix seed and a random alpha (coef = 0.7): the summation, the mirror factor and both reduction stages
    of the realistic call.  tr G within (4 u_T + 16 * 2^-53) sum_i (|coef alpha_i^2| + |G_ii|): coef, the product and the fused
    multiply-add round once each in T, and a diagonal term passes at most 16 fp64 additions with a non-zero partner (one per
    thread, the two shuffle trees, the cross-wave sums).  A second call returns the same bits; c = 1 of the rank-C form returns
    the single-column bits."""
    expected, bound, y = _dense_reference(*net, G.B, n, T, get)
    t = _dense_call(L, ctx, T, net, get, G.B, "sep", n)
    _hold_dense("n=%d %s-%s%d %s %s" % ((n,) + net + (get, np.dtype(T).name)), T, t, expected, bound, y)
    g, a = G.dense_seed(n, T)
    assert abs(t[3] - float(expected[3])) <= _trace_allow(T, n), (t[3], expected[3])
    assert _dense_call(L, ctx, T, net, get, G.B, "sep", n).tobytes() == t.tobytes()
    assert _dense_call(L, ctx, T, net, get, G.B, "sep", n, c=1).tobytes() == t.tobytes()


# ------------------------------------------------------------------------------------------- 4. what the entries read
@pytest.mark.parametrize("get", GETS)
@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("c", [None, 3], ids=["single", "c3"])
def test_what_is_read(L, ctx, c, T, get):
    """include/smnngp.h at smn_lml_grad_terms: neg_kinv_d is read in the lower triangle and, whole, in the 64 x 64 blocks on the
    diagonal (where entries above the diagonal are weighted 0 and must be finite: smn_loo_head writes those blocks whole);
    no tile strictly above the block diagonal is touched."""
    n, net = 200, G.NETS[0]
    k0d, qd = _inputs_dev(ctx, "sep", n, T)
    (ad,) = _dev(ctx, ("zeros", n, c or 1, T), lambda: (np.zeros((n, c or 1), T),))
    seed = Seed(ctx, n, T)
    for i, j in ((3, 10), (62, 63), (130, 191), (3, 100), (0, 199), (63, 64)):   # above the diagonal: in a diagonal tile, in an upper tile
        t = seed.probe(i, j, np.asarray(-0.75, T), lambda gd: _terms(L, ctx, T, *net, get, G.B, k0d, qd, n, gd, ad, 0.0, c))
        assert not t.any() and not np.signbit(t).any(), (i, j, t)
    g, _ = G.dense_seed(n, T)
    clean = _dense_call(L, ctx, T, net, get, G.B, "sep", n, c)
    bad = g.copy()
    for tr in range(4):
        bad[tr * 64:(tr + 1) * 64, (tr + 1) * 64:] = np.nan              # every tile strictly above the block diagonal
        blk = bad[tr * 64:(tr + 1) * 64, tr * 64:(tr + 1) * 64]
        blk[np.triu_indices(blk.shape[0], 1, blk.shape[1])] = 1e30        # finite and arbitrary above the diagonal of a diagonal block
    t = _dense_call(L, ctx, T, net, get, G.B, "sep", n, c, nk=bad)
    assert t.tobytes() == clean.tobytes(), (t, clean)


# ------------------------------------------------------------------------------------------- 5. zero rows, b_std == 0
LIVE = tuple(r for r in range(65) if r not in G.ZERO_ROWS)


@pytest.mark.parametrize("get", GETS)
@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("net", G.NETS, ids=G.NET_IDS)
def test_zero_rows_under_zero_bias_dense_seed(L, ctx, net, T, get):
    """b_std == 0 exactly, all-zero input rows at 0, 31, 64 (q = 0 at every layer): every returned value finite, terms[1] = 0, and
    for terms[0] and terms[2] what the same seed returns with the zero rows and columns deleted (the tile layout differs, so
    within the dense-seed allowance, not to the bit); G_ii of a zero row still counts in terms[3]."""
    expected, bound, y = _dense_reference(*net, 0.0, 65, T, get, "zero")
    exp_live, bound_live, y_live = _dense_reference(*net, 0.0, 65, T, get, "zero", LIVE)
    assert (np.abs(expected[:3] - exp_live[:3]) <= 1e-17 * bound).all()    # the rules: the zero rows contribute nothing
    tag = "zero65-b0 %s-%s%d %s %s" % (net + (get, np.dtype(T).name))
    t = _dense_call(L, ctx, T, net, get, 0.0, "zero", 65)
    _hold_dense(tag, T, t, expected, bound, y)
    d = _dense_call(L, ctx, T, net, get, 0.0, "zero", 65, keep=LIVE)
    _hold_dense(tag + " rows deleted", T, d, exp_live, bound_live, y_live)
    assert t[1] == 0.0 and d[1] == 0.0
    yy = np.maximum(np.maximum(y, y_live), _floor(T))
    for k in (0, 2):
        assert abs(t[k] - d[k]) <= FACTOR * yy[k] * float(bound[k]), (k, t, d)
    assert abs(t[3] - float(expected[3])) <= _trace_allow(T, 65) and abs(d[3] - float(exp_live[3])) <= _trace_allow(T, 65, LIVE)
    assert abs(float(expected[3] - exp_live[3])) > 0.1              # the G_ii of the zero rows are in the first and not in the second


MODEL_HYP = dict(w_std=1.4, b_std=0.0, last_w_std=0.8, eps=5e-2)


@functools.lru_cache(maxsize=None)
def _model_data():
    rng = np.random.default_rng(65)
    x = rng.standard_normal((65, G.D))
    x[list(G.ZERO_ROWS)] = 0.0
    y = np.sin(x[:, 0]) + 0.3 * rng.standard_normal(65)
    return x, y


@functools.lru_cache(maxsize=None)
def _model_fd(net, act, layers, get):
    """(loss, central differences in w_std, last_w_std, eps) of the oracle loss, relative step 1e-5."""
    from oracle import nngp_oracle as O
    x, y = _model_data()
    kfn = O.mlp_kernel if net == "mlp" else O.dense_resnet_kernel

    def loss(**h):
        with np.errstate(all="ignore"):
            k = kfn(x, None, layers, act, h["w_std"], h["b_std"], h["last_w_std"], get)
        return -O.mvn_logpdf(y, k + h["eps"] * np.eye(65)) / 65

    fd = {}
    for key in ("w_std", "last_w_std", "eps"):
        step = 1e-5 * MODEL_HYP[key]
        fd[key] = (loss(**dict(MODEL_HYP, **{key: MODEL_HYP[key] + step})) - loss(**dict(MODEL_HYP, **{key: MODEL_HYP[key] - step}))) / (2 * step)
    return loss(**MODEL_HYP), fd


@pytest.mark.parametrize("get", GETS)
@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("net", G.NETS, ids=G.NET_IDS)
def test_model_gradient_with_zero_rows_and_zero_bias(net, T, get):
    """SPR.loss_and_grad() (Gaussian head) on such data: finite throughout, and the central differences of the oracle loss in
    w_std, last_w_std and eps to the project's 2e-6 (f64) / 1e-2 (f32) of max(scale, |ref|)."""
    from smnngp import nt_kernels
    from smnngp.spax.kernels import NNGPKernel, NTKKernel
    from smnngp.spax.likelihoods import GaussianLikelihood
    from smnngp.spax.models import SPR
    family, act, layers = net
    base = nt_kernels.get_mlp_kernel if family == "mlp" else nt_kernels.get_dense_resnet_kernel
    x, y = _model_data()
    with np.errstate(divide="ignore"):          # a value of exactly 0 is stored as raw = -inf (softplus-inverse of 0)
        kernel = (NTKKernel if get == "ntk" else NNGPKernel)(
            lambda w, b, l: base(layers, 1, act=act, w_std=w, b_std=b, last_w_std=l), MODEL_HYP["w_std"], 0.0, MODEL_HYP["last_w_std"])
        model = SPR(kernel, GaussianLikelihood(), x.astype(T), y.astype(T), 0.0, 1.0, eps=MODEL_HYP["eps"])
        loss, grads = model.loss_and_grad()
    ref_loss, fd = _model_fd(family, act, layers, get)
    assert np.isfinite(loss) and set(grads) == set(model.vars()) and all(np.isfinite(v) for v in grads.values()), (loss, grads)
    f64 = T == np.float64
    print("\n[model] %s-%s%d %s %s loss %.12g ref %.12g" % (net + (get, np.dtype(T).name, loss, ref_loss)))
    assert abs(loss - ref_loss) < (1e-9 if f64 else 1e-3) * max(1.0, abs(ref_loss))
    names = {id(v): k for k, v in model.vars().items()}
    scale = max(abs(v) for v in fd.values())
    for key, var in (("w_std", kernel.w_std), ("last_w_std", kernel.last_w_std), ("eps", model.eps)):
        got = grads[names[id(var)]] / float(var.constraint.grad(var.value))
        err = abs(got - fd[key]) / max(scale, abs(fd[key]))
        print("[model]   d/d%s %.12g ref %.12g err %.3g" % (key, got, fd[key], err))
        assert err < (2e-6 if f64 else 1e-2), (key, got, fd[key])


# ------------------------------------------------------------------------------------------- 6. nearly duplicate rows
@pytest.mark.parametrize("get", GETS)
@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("net", G.NETS, ids=G.NET_IDS)
def test_nearly_duplicate_rows(L, ctx, net, T, get):
    """32 pairs (p, p + 1) of rows at input correlation 1 - gap, three of them across a tile edge (rows 63 / 64, 127 / 128, 191 /
    192); entry (p + 1, p) of each.  The same allowance with Y over the 32 pairs of one gap: the f32 NumPy evaluation loses the
    same digits, so the yardstick carries the 1 / sqrt(1 - c^2) growth of the ReLU tangent of Theta."""
    p = G.DUP_PAIRS
    for gap in G.DUP_GAPS[T]:
        ref, s, y, extra = _reference(*net, G.B, "dup", G.DUP_N, T, get, None, gap)
        out, g = _run_probes(L, ctx, T, *net, get, G.B, "dup", G.DUP_N, p + 1, p, gap)
        assert not extra.any()
        r = _hold("dup gap=%g %s-%s%d %s %s" % ((gap,) + net + (get, np.dtype(T).name)), T, out, g, p + 1, p, ref, s, y, extra)
        yy = np.maximum(y, _floor(T))
        print("[dup] gap %g %s-%s%d %s %s  Y/u %s  device err/u %s" % (
            (gap,) + net + (get, np.dtype(T).name, " ".join("%7.1f" % v for v in y / G.U[T]),
                            " ".join("%7.1f" % v for v in r * yy / G.U[T]))))
