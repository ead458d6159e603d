"""Host checks of tests/_grad_probe_rules.py, the reference and yardstick of test_gpu_grad_probes.py (no GPU).

1. In float64 the rules are the existing ones (_multi_rules.dense_tangents, _ntk_rules.tangents) to a few u per entry.
2. They are the ENTRYWISE central differences of the oracle's kernel matrices (not of a loss), one all-zero row included.
3. The yardstick Y = max |rules_T - rules_longdouble| / s exists for every case the GPU file runs: finite everywhere, below 64 u
   on separated inputs.  (The zero-row cases are not separated: under b_std > 0 the zero rows are exact duplicates of each other,
   and the generic formulas cancel there as they do at c = 1; the near-duplicate cases grow like 1 / sqrt(1 - c^2) by design.)
"""
import numpy as np
import pytest

import _grad_probe_rules as G
import _multi_rules as M
import _ntk_rules as NT
from oracle import nngp_oracle as O
from test_gpu_kernel_budget import NETS as BUDGET_NETS

U64 = 2.0 ** -53
DTYPES = [np.float32, np.float64]


def test_cases_are_the_kernel_budget_nets():
    assert G.NETS == BUDGET_NETS and np.finfo(np.longdouble).eps <= 2.0 ** -63


def _x(n, zero_row=None, seed=5):
    x = np.random.default_rng(seed).standard_normal((n, G.D))
    if zero_row is not None:
        x[zero_row] = 0.0
    return x


def _gram(x):
    k0 = x @ x.T / x.shape[1]
    q = np.einsum("ij,ij->i", x, x) / x.shape[1]
    np.fill_diagonal(k0, q)
    return k0, q


def _rel(new, old, i, j):
    n = i.max() + 1
    s = G.scales(old[:, i, j], old[:, np.arange(n), np.arange(n)], i, j)
    return np.abs(new - old[:, i, j]) / s


@pytest.mark.parametrize("net,act,layers", G.NETS, ids=G.NET_IDS)
def test_float64_rules_are_the_existing_rules(net, act, layers):
    x = _x(40)
    k0, q = _gram(x)
    i, j = np.tril_indices(40)
    k, kw, kb = M.dense_tangents(net, x, layers, act, G.W, G.B, G.LW)
    old = np.stack([kw * 2 * G.W, kb * 2 * G.B, k * 2 / G.LW])
    r = _rel(G.entry_tangents(net, act, layers, G.W, G.B, G.LW, k0, q, i, j, np.float64, "nngp"), old, i, j)
    print("nngp: max |new - old| / s = %.1f u" % (r.max() / U64))
    assert r.max() <= 64 * U64
    _, dw, db, dl = NT.tangents(net, x, layers, act, G.W, G.B, G.LW)
    r = _rel(G.entry_tangents(net, act, layers, G.W, G.B, G.LW, k0, q, i, j, np.float64, "ntk"), np.stack([dw, db, dl]), i, j)
    print("ntk:  max |new - old| / s = %.1f u" % (r.max() / U64))
    assert r.max() <= 64 * U64


@pytest.mark.parametrize("get", ["nngp", "ntk"])
@pytest.mark.parametrize("net,act,layers", G.NETS, ids=G.NET_IDS)
def test_rules_are_the_entrywise_central_differences_of_the_oracle_kernel(net, act, layers, get):
    """n = 12 with row 5 all zero (b_std > 0), relative step 1e-5 and 2e-6 as every finite-difference comparison here, per entry
    against max(s_ij, |fd_ij|)."""
    n = 12
    x = _x(n, zero_row=5)
    k0, q = _gram(x)
    kfn = O.mlp_kernel if net == "mlp" else O.dense_resnet_kernel
    hyp = dict(w_std=G.W, b_std=G.B, last_w_std=G.LW)
    fd = []
    for key in ("w_std", "b_std", "last_w_std"):
        step = 1e-5 * abs(hyp[key])
        up, dn = dict(hyp, **{key: hyp[key] + step}), dict(hyp, **{key: hyp[key] - step})
        fd.append((kfn(x, None, layers, act, get=get, **up) - kfn(x, None, layers, act, get=get, **dn)) / (2.0 * step))
    fd = np.stack(fd)
    i, j = np.divmod(np.arange(n * n), n)
    got = G.entry_tangents(net, act, layers, G.W, G.B, G.LW, k0, q, np.maximum(i, j), np.minimum(i, j), np.float64, get)
    s = G.scales(fd[:, i, j], fd[:, np.arange(n), np.arange(n)], i, j)
    err = np.abs(got - fd[:, i, j]) / np.maximum(s, np.abs(fd[:, i, j]))
    print("max err %.3g" % err.max())
    assert np.isfinite(got).all() and err.max() < 2e-6


def test_zero_variance_rows_contribute_nothing_under_zero_bias():
    """b_std == 0 with an all-zero row: finite, d/db_std = 0 everywhere, and nothing in the row's entries (ReLU and erf)."""
    x = _x(12, zero_row=5)
    k0, q = _gram(x)
    i, j = np.tril_indices(12)
    hit = (i == 5) | (j == 5)
    for net, act, layers in G.NETS:
        for get in ("nngp", "ntk"):
            for T in (np.float32, np.float64, np.longdouble):
                t = G.entry_tangents(net, act, layers, G.W, 0.0, G.LW, k0.astype(T), q.astype(T), i, j, T, get)
                assert t.dtype == T and np.isfinite(t).all()
                assert not t[1].any() and not t[:, hit].any()
                assert t[0][~hit].all() and t[2][~hit].all()


@pytest.mark.parametrize("get", ["nngp", "ntk"])
@pytest.mark.parametrize("T", DTYPES, ids=["f32", "f64"])
def test_yardstick_of_every_probe_case(T, get):
    u = G.U[T]
    for cid, kind, n, gap, b_std, (i, j), nets in G.probe_sets():
        for net, act, layers in nets:
            k0, q = G.inputs(kind, n, T)
            ref, s, y, extra = G.reference(net, act, layers, b_std, k0, q, i, j, T, get)
            print("%-12s %s-%s%d Y/u = %s" % (cid, net, act, layers, np.round(y / u, 1)))
            assert np.isfinite(ref.astype(np.float64)).all() and np.isfinite(y).all() and (s >= 0).all()
            if kind == "sep":
                assert y.max() < 64 * u, (cid, net, act, y / u)
            # the extra allowance: only between exactly duplicate rows (the zero rows under b_std > 0), only ReLU Theta, ~ sqrt(u) s
            dup = G.duplicate_mask(k0, q, i, j, b_std)
            assert dup.any() == (kind == "zero" and b_std > 0) and not extra[:, ~dup].any()
            if dup.any():
                assert dup.sum() == 3 and extra[:, dup].all() == (act == "relu" and get == "ntk")
                assert (extra[:, dup] <= 8 * (layers + 1) * np.sqrt(u) * s[:, dup]).all(), extra[:, dup] / s[:, dup] / np.sqrt(u)


@pytest.mark.parametrize("get", ["nngp", "ntk"])
@pytest.mark.parametrize("T", DTYPES, ids=["f32", "f64"])
def test_yardstick_of_the_near_duplicate_cases(T, get):
    """Finite at every gap; it carries the growth of the ReLU tangent of Theta towards c = 1, which is the point of it."""
    p = G.DUP_PAIRS
    assert len(p) == 32 and len(np.unique(np.concatenate([p, p + 1]))) == 64 and (p + 1 < G.DUP_N).all()
    assert sum((p + 1) % G.GT == 0 for p in p) >= 2                 # pairs that straddle a tile edge
    for gap in G.DUP_GAPS[T]:
        k0, q = G.inputs("dup", G.DUP_N, T, gap)
        c0 = k0[p + 1, p].astype(np.float64) / np.sqrt(q[p].astype(np.float64) * q[p + 1].astype(np.float64))
        assert np.allclose(1.0 - c0, gap, rtol=0.05 if T == np.float64 else 0.2), (gap, 1.0 - c0)
        for net, act, layers in G.NETS:
            _, _, y, extra = G.reference(net, act, layers, G.B, k0, q, p + 1, p, T, get)
            assert not extra.any()
            print("gap %g %s-%s%d Y/u = %s" % (gap, net, act, layers, np.round(y / G.U[T], 1)))
            assert np.isfinite(y).all()


@pytest.mark.parametrize("get", ["nngp", "ntk"])
@pytest.mark.parametrize("T", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("net,act,layers", G.NETS, ids=G.NET_IDS)
@pytest.mark.parametrize("n", G.DENSE_N)
def test_yardstick_of_the_dense_seed_cases(n, net, act, layers, T, get):
    _, bound, y = G.dense_reference(net, act, layers, G.B, n, T, get)
    assert np.isfinite(bound.astype(np.float64)).all()
    print("n %d %s-%s%d Y/u = %s" % (n, net, act, layers, np.round(y / G.U[T], 1)))
    assert np.isfinite(y).all() and y.max() < 64 * G.U[T]


def test_geometry_selection_covers_what_it_names():
    i, j = G.geometry_entries(200)
    assert len(i) <= 600 and (j <= i).all() and len(np.unique(i * 200 + j)) == len(i)
    have = set(zip(i.tolist(), j.tolist()))
    nt = 4
    for tr in range(nt):
        for tc in range(tr + 1):
            r0, c0, r1, c1 = tr * 64, tc * 64, min(tr * 64 + 63, 199), min(tc * 64 + 63, 199)
            for e in ((r0, c0), (r1, c0), (r1, c1)) + (((r0, c1),) if tr != tc else ()):
                assert e in have, e
            for r in (31, 32):
                if r0 + r < 200:
                    assert any((r0 + r, c) in have for c in range(c0, c1 + 1))
            assert sum(1 for a, b in have if r0 <= a <= r1 and c0 <= b <= c1) >= 8
    assert all((d, d) in have and (199, d) in have for d in range(200))
    zi, zj = G.zero_row_entries(65)
    zs = set(zip(zi.tolist(), zj.tolist()))
    assert all((max(r, c), min(r, c)) in zs for r in G.ZERO_ROWS for c in range(65))
