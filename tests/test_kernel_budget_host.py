"""tests/_kernel_budget.py (the NumPy port of the fixture's error-budget rule, the input generators and the entry selection)
against the mpmath fixture, against mpmath itself at 40 digits, and against its own claims.  CPU only.

test_gpu_kernel_budget.py holds multi-tile builds to these budgets; this file is what lets it trust them."""
import importlib.util
import os
import sys

import numpy as np
import pytest

import _kernel_budget as KB

HERE = os.path.dirname(os.path.abspath(__file__))
GEN = os.path.join(HERE, "golden", "make_mp_golden.py")
Z = np.load(os.path.join(HERE, "golden", "nngp_mp_golden.npz"))
SETS32 = [str(s) for s in Z["cmp_sets"] if "f32" in [str(v) for v in Z["cmp_%s_dtypes" % str(s)]]]
NETS = (("mlp", "relu", 3), ("mlp", "erf", 6), ("resnet", "relu", 2), ("resnet", "erf", 1))   # the GPU file's sets
HYP = (1.4, 0.3, 0.8)


def _gen():
    mp = pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_mp_golden", GEN)
    mod = importlib.util.module_from_spec(spec)
    keep, sys.dont_write_bytecode = sys.dont_write_bytecode, True   # no __pycache__ next to the fixture
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.dont_write_bytecode = keep
    return mp, mod


# ----------------------------------------------------------------------------- the port against the fixture
@pytest.mark.parametrize("name", SETS32)
@pytest.mark.parametrize("net", ["mlp", "resnet"])
@pytest.mark.parametrize("act", ["relu", "erf"])
def test_port_reproduces_fixture_budgets(name, net, act):
    """Budgets within 1e-4 relative of the stored *_bud32 wherever that is nonzero (it is stored in f32: 6e-8), references
    within 1 % of *_bud32 of *_ref.  Off-diagonal entries of exact duplicates (rho = 1 in mp, 1 - 1e-16 in fp64) are counted
    and printed, and NOT excluded: the port holds there too (its error there is sqrt(1e-16) of a budget of sqrt(u))."""
    x1, x2 = Z["cmp_%s_x1" % name], Z["cmp_%s_x2" % name]
    w, b, lw = (float(v) for v in Z["cmp_%s_hyp" % name])
    d = x1.shape[1]
    worst_b = worst_r = 0.0
    ndup = 0
    for L in (1, 3, 6):
        for tag, xb in (("sym", None), ("cross", x2)):
            key = "cmp_%s_%s_%s_L%d_%s" % (name, net, act, L, tag)
            fb, fr = Z[key + "_bud32"].astype(np.float64), Z[key + "_ref"]
            n1, n2 = fr.shape[1:]
            i, j = np.divmod(np.arange(n1 * n2), n2)
            ref, bud = KB.reference(net, act, L, w, b, lw, x1, xb, i, j, d, KB.U["f32"])
            other = x1 if xb is None else xb
            ndup += int(((x1[i] == other[j]).all(axis=1) & ((i != j) | (xb is not None))).sum())
            for m in (0, 1):
                got_b, got_r = bud[m].reshape(n1, n2), ref[m].reshape(n1, n2)
                assert np.isfinite(got_b).all() and np.isfinite(got_r).all(), key
                nz = fb[m] != 0
                rb = np.abs(got_b[nz] - fb[m][nz]) / fb[m][nz]
                worst_b = max(worst_b, float(rb.max()))
                assert rb.max() <= 1e-4, (key, m, float(rb.max()))
                assert (got_b[~nz] <= 1e-30).all(), (key, m)
                rr = np.abs(got_r - fr[m])
                assert (rr <= 0.01 * fb[m]).all(), (key, m, float((rr[nz] / fb[m][nz]).max()))
                worst_r = max(worst_r, float((rr[nz] / fb[m][nz]).max()))
    print("\n[budget-port] %-8s %-6s %-4s budget rel dev %.2e  |ref dev| / bud32 %.2e  (%d exact-duplicate entries included)"
          % (name, net, act, worst_b, worst_r, ndup))


# ----------------------------------------------------------------------------- exact inputs
@pytest.mark.parametrize("d", [33, 257, 3072])
def test_exact_inputs_have_an_exact_gram(d):
    """float32 Gram of exact(300, d) summed forward and summed reversed in chunks of 4 (the MFMA's K grouping) equals the
    float64 Gram bit for bit: no summation order can round."""
    x = KB.exact(300, d, "f32")
    assert x.dtype == np.float32 and np.array_equal(x, np.round(x)) and np.abs(x).max() <= 3
    g64 = x.astype(np.float64) @ x.astype(np.float64).T
    fwd = np.zeros((300, 300), np.float32)
    for k in range(d):
        fwd += np.outer(x[:, k], x[:, k])
    rev = np.zeros((300, 300), np.float32)
    for k0 in reversed(range(0, d, 4)):
        part = np.zeros((300, 300), np.float32)
        for k in reversed(range(k0, min(k0 + 4, d))):
            part += np.outer(x[:, k], x[:, k])
        rev += part
    assert fwd.dtype == np.float32 and rev.dtype == np.float32
    assert np.array_equal(fwd.astype(np.float64), g64) and np.array_equal(rev.astype(np.float64), g64)
    assert np.abs(g64).max() <= 9 * d < 2 ** 24


def test_generators_are_seeded_and_separated():
    for gen, d in ((KB.gauss, 40), (KB.exact, 33)):
        a, b = gen(300, d, "f32"), gen(300, d, "f32")
        assert np.array_equal(a, b) and not np.array_equal(a, gen(300, d, "f32", seed=1))
        assert gen(64, d, "f64").dtype == np.float64
    x = KB.exact(64, 33, "f32")
    x[5] = 2 * x[9]
    with pytest.raises(AssertionError):
        KB.assert_separated(x)
    with pytest.raises(AssertionError):
        KB.assert_separated(x[:6], x[9:10] * -3)
    x[5] = 0
    with pytest.raises(AssertionError):
        KB.assert_separated(x)


# ----------------------------------------------------------------------------- entry selection
@pytest.mark.parametrize("n1,n2,sym", [(300, 300, True), (260, 132, False), (4000, 4000, True), (4400, 4400, True),
                                       (2100, 2050, False)])
def test_selection_covers_every_tile(n1, n2, sym):
    i, j = KB.select_entries(n1, n2, sym)
    assert i.min() >= 0 and i.max() < n1 and j.min() >= 0 and j.max() < n2
    assert KB.tiles_covered(i, j, n1, n2, sym)
    if n1 * n2 <= KB.FULL_LIMIT:
        assert len(i) == (n1 * (n1 + 1) // 2 if sym else n1 * n2)
        return
    if sym:
        assert (j // KB.TILE <= i // KB.TILE).all()
    tiles = {}
    for a, c in zip(i, j):
        tiles.setdefault((a // KB.TILE, c // KB.TILE), []).append((a % KB.TILE, c % KB.TILE))
    t1 = (n1 + KB.TILE - 1) // KB.TILE
    assert len(tiles) == (t1 * (t1 + 1) // 2 if sym else t1 * ((n2 + KB.TILE - 1) // KB.TILE))
    for (tr, tc), ent in tiles.items():
        h, wd = min(KB.TILE, n1 - tr * KB.TILE), min(KB.TILE, n2 - tc * KB.TILE)
        assert len(ent) >= 64
        assert {(0, 0), (0, wd - 1), (h - 1, 0), (h - 1, wd - 1)} <= set(ent)
        rows = {r for r, _ in ent}
        assert h <= 64 or {63, 64} <= rows, (tr, tc)
    i2, j2 = KB.select_entries(n1, n2, sym)
    assert np.array_equal(i, i2) and np.array_equal(j, j2)


# ----------------------------------------------------------------------------- the port against mpmath on the large inputs
@pytest.mark.parametrize("net,act,L", NETS)
def test_port_against_mpmath_sample(net, act, L):
    """64 entries (two of them diagonal) of exact(1300, 257) at the GPU file's hyper-parameters: the port's reference against
    mlp_entry / resnet_entry at 40 digits on the EXACT rational K0 = <x_i, x_j> / 257.  Within 1 % of the f32 budget, and within
    the f64 budget (u = 2^-53, d_terms = 2) -- which is why the GPU file may allow fp64 results twice that budget and no more."""
    mp, g = _gen()
    w, b, lw = HYP
    n, d = 1300, 257
    x = KB.exact(n, d, "f32")
    rng = np.random.default_rng(5)
    i = np.concatenate([rng.integers(n, size=62), [17, 1299]])
    j = np.concatenate([rng.integers(n, size=62), [17, 1299]])
    sw = j > i
    i, j = np.where(sw, j, i), np.where(sw, i, j)
    ref, b32 = KB.reference(net, act, L, w, b, lw, x, None, i, j, 2, KB.U["f32"])
    _, b64 = KB.reference(net, act, L, w, b, lw, x, None, i, j, 2, KB.U["f64"])
    xi = x.astype(np.int64)
    worst32 = worst64 = 0.0
    for e in range(len(i)):
        k0 = mp.mpf(int(xi[i[e]] @ xi[j[e]])) / d
        qi, qj = mp.mpf(int(xi[i[e]] @ xi[i[e]])) / d, mp.mpf(int(xi[j[e]] @ xi[j[e]])) / d
        want = g.ENTRY[net](k0, qi, qj, L, act, w, b, lw)
        for m in (0, 1):
            err = abs(float(mp.mpf(float(ref[m][e])) - want[m]))
            worst32 = max(worst32, err / b32[m][e])
            worst64 = max(worst64, err / b64[m][e])
    print("\n[budget-port] mp sample %-6s %-4s L=%d: |port - mp| / f32 budget %.2e, / f64 budget %.3f" % (net, act, L, worst32, worst64))
    assert worst32 <= 0.01
    assert worst64 <= 1.0


def test_fast_erf_allowance_is_the_fixture_tests_term():
    w, lw, L = 1.3, 0.9, 3
    amp = 4 * w * w / np.pi
    assert KB.fast_erf_allowance(L, w, lw) == lw * lw * (2 / np.pi) * 2.6e-7 * sum(amp ** i for i in range(L))
