"""Host checks of tests/_input_probe_rules.py, the reference of test_gpu_input_probes.py: the long-double rules against the fp64
rules of tests/_input_grad_rules.py and against central differences of the oracle's kernels; exact inputs; seeds that cover every
pair once; the acceptance rule accepts the rules evaluated in T and rejects eight damaged variants; and every case of the GPU
file keeps 16 max(Y, 4u) within the kernel tolerance of its dtype (the cases are the GPU file's own lists)."""
import numpy as np
import pytest

import _input_grad_rules as R
import _input_probe_rules as P

L = np.longdouble
DTYPES = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]
FORM_IDS = ["%s-%s-%s" % f for f in P.FORMS]


def _hyp(layers, act, b=P.B):
    return dict(num_hiddens=layers, act=act, w_std=P.W, b_std=b, last_w_std=P.LW)


# ----------------------------------------------------------------------------------------------------------- the rules
@pytest.mark.parametrize("layers", [0, 1, 2, 3])
@pytest.mark.parametrize("kind,act,get", P.FORMS, ids=FORM_IDS)
def test_long_double_rules_equal_the_fp64_rules(kind, act, get, layers):
    """Within 400 u_64 of the scale max|.| per factor: the two texts order a few operations differently ((1 - s)(1 + s) against
    1 - s^2) and the fp64 one rounds at every step."""
    x1, x2 = P.stored_rows("a1")[:40], P.stored_rows("a2")[:50]
    f = P.factors(kind, act, get, layers, P.B, x1, x2, L)
    f1, f2, dd = R.factors(kind, x1, x2, get, **_hyp(layers, act))
    for got, want in ((f.f1, f1), (f.f2r, f2), (f.ddiag, dd)):
        assert np.abs(got - want.astype(L)).max() <= 400 * P.U[np.float64] * max(np.abs(want).max(), 1e-300)
    g = P.factors(kind, act, get, layers, P.B, x2, x1, L)             # the column side is the row side of the transposed pair
    assert np.abs(f.f2c - g.f2r.T).max() <= 64 * 2.0 ** -64 * max(np.abs(f.f2c).max(), 1e-300)
    assert np.abs(f.f1 - g.f1.T).max() <= 64 * 2.0 ** -64 * np.abs(f.f1).max()


@pytest.mark.parametrize("kind,act,get", P.FORMS, ids=FORM_IDS)
def test_rules_are_the_slopes_of_the_oracle_kernels(kind, act, get):
    """Central differences of oracle.mlp_kernel / dense_resnet_kernel in one input row, h = 1e-5 along a random direction: the
    row side moves x1[r] (every K[r, :]), the column side moves x2[j] (every K[:, j]).  The differences are good to h^2 |K'''| +
    u |K| / h ~ 1e-10; held to 1e-7 of the largest slope."""
    x1, x2 = np.array(P.stored_rows("s")[:6]), np.array(P.stored_rows("s")[10:17])
    f = P.factors(kind, act, get, 2, P.B, x1, x2, L)
    kfn = R.KERNELS[kind]
    h, d = 1e-5, x1.shape[1]
    v = np.random.default_rng(5).standard_normal(d)
    for r in range(len(x1)):
        up, dn = x1.copy(), x1.copy()
        up[r] += h * v
        dn[r] -= h * v
        fd = (np.asarray(kfn(up, x2, get=get, **_hyp(2, act)))[r] - np.asarray(kfn(dn, x2, get=get, **_hyp(2, act)))[r]) / (2 * h)
        want = ((f.f1[r][:, None] * x2 + 2 * f.f2r[r][:, None] * x1[r][None, :]) / d) @ v
        assert np.abs(fd - want.astype(np.float64)).max() <= 1e-7 * np.abs(want).max()
    for j in range(len(x2)):
        up, dn = x2.copy(), x2.copy()
        up[j] += h * v
        dn[j] -= h * v
        fd = (np.asarray(kfn(x1, up, get=get, **_hyp(2, act)))[:, j] - np.asarray(kfn(x1, dn, get=get, **_hyp(2, act)))[:, j]) / (2 * h)
        want = ((f.f1[:, j][:, None] * x1 + 2 * f.f2c[:, j][:, None] * x2[j][None, :]) / d) @ v
        assert np.abs(fd - want.astype(np.float64)).max() <= 1e-7 * np.abs(want).max()
    xs = np.vstack([x1, x2])
    kd = lambda z: np.diag(np.asarray(kfn(z, None, get=get, **_hyp(2, act))))   # noqa: E731
    fd = (kd(xs + h * v) - kd(xs - h * v)) / (2 * h)
    dd = P.factors(kind, act, get, 2, P.B, xs, xs, L).ddiag
    want = (2 * dd[:, None] * xs / d) @ v
    assert np.abs(fd - want.astype(np.float64)).max() <= 1e-7 * np.abs(want).max()


def test_guards_follow_the_device_conventions():
    """Duplicate rows: c = 1 at every activation (D_A = D_1 = D_2 = 0, phi_1 = 0); anti-parallel rows under b_std = 0: c = -1 at
    the first; a zero-variance row: no variance-side term and c = 0.  Nothing else in the hard inputs sits on a guard."""
    for T in DTYPES:
        x, cases = P.hard_inputs(T)
        for b in (0.0, P.B):
            f = P.factors("mlp", "relu", "ntk", 2, b, x, x, L)
            want = np.zeros(f.hits.shape, bool)
            want[:, np.arange(len(x)), np.arange(len(x))] = True
            for r, j in cases["dup"]:
                want[:, r, j] = want[:, j, r] = True
            if b == 0.0:
                for r, j in cases["anti"]:
                    want[0, r, j] = want[0, j, r] = True
                want[:, P.ZERO_ROW, :] = want[:, :, P.ZERO_ROW] = False
            assert np.array_equal(f.hits != 0, want)
            assert np.array_equal(np.flatnonzero(f.zero1), [P.ZERO_ROW] if b == 0.0 else [])
            if b == 0.0:
                assert not f.f2r[P.ZERO_ROW].any() and np.isfinite(f.f1).all()
        assert not P.factors("mlp", "erf", "ntk", 2, 0.0, x, x, L).hits.any()


# ---------------------------------------------------------------------------------------------------- inputs and seeds
def test_every_input_set_is_exact():
    for a, b in (("a1", "a2"), ("s", "s")):
        P.exact_gram(P.stored_rows(a), P.stored_rows(b), np.float32)
    for a, b in (("f1", "f2"), ("fs", "fs")):                          # d = 7: the products; u itself takes one rounding
        P.exact_gram(P.stored_rows(a), P.stored_rows(b), np.float32)
    for T in DTYPES:
        x, _ = P.hard_inputs(T)
        P.exact_gram(x, x, T)
        assert np.abs(x[: P.SCALED[0]]).max() <= 4.0
    for name in ("a1", "a2", "s", "f1", "f2", "fs"):
        x = P.stored_rows(name)
        assert np.abs(x).max() <= 4.0 and np.array_equal(x * 64, np.round(x * 64))
        assert len(np.unique(x, axis=0)) == len(x)


def test_reading_columns():
    a1, a2, s = P.stored_rows("a1"), P.stored_rows("a2"), P.stored_rows("s")
    assert (a1[:, 6] == 0).all() and (a1[:, 7] == 1).all() and (a2[:, 6] == 1).all() and (a2[:, 7] == 0).all()
    assert ((s[:, 6] == 0) & (s[:, 7] == 1) | (s[:, 6] == 1) & (s[:, 7] == 0)).all()
    for t0 in range(0, 130, 64):                                        # every 64-row tile of the pass holds both roles
        assert 0 < (s[t0:t0 + 64, 6] == 0).sum() < len(s[t0:t0 + 64])
    assert s[129, 6] != s[128, 6] or s[129, 6] != s[0, 6]


@pytest.mark.parametrize("n1,n2", [(130, 130), (5, 257), (1, 257)])
def test_shift_seeds_cover_every_pair_once(n1, n2):
    count = np.zeros((n1, n2), int)
    for s in P.shift_seeds(n1, n2):
        assert len(set(s.r)) == n1 and set(np.abs(s.g)) <= {0.25, 0.5, 1.0, 2.0, 4.0}
        count[s.r, s.j] += 1
    assert (count == 1).all()


@pytest.mark.parametrize("n", [1, 2, 64, 65, 130, 257])
def test_matching_seeds_cover_every_pair_once(n):
    seeds = P.matching_seeds(n)
    assert len(seeds) == (n - 1 if n % 2 == 0 else n if n > 1 else 0) + 1
    count = np.zeros((n, n), int)
    for s in seeds:
        assert (s.r >= s.j).all()
        off = s.r != s.j
        assert off.all() or not off.any()
        rows = np.concatenate([s.r[off], s.j[off]])
        assert len(set(rows)) == len(rows)
        count[s.r, s.j] += 1
    assert (count == np.tril(np.ones((n, n), int))).all()


def test_packed_seeds_read_each_pair_once():
    for T in DTYPES:
        _, cases = P.hard_inputs(T)
        for name, pairs in cases.items():
            for sym in (False, True):
                both = pairs if sym else pairs + [(j, r) for r, j in pairs]
                seeds = P.pack_pairs(both, sym)
                got = sorted((int(r), int(j)) for s in seeds for r, j in zip(s.r, s.j))
                assert got == sorted((max(p), min(p)) if sym else p for p in both), name


# ------------------------------------------------------------------------------------------------------ acceptance rule
def _simulated(case, fac, x1, x2, sym, two=2, seeds=None):
    seeds = case.seeds if seeds is None else seeds
    return np.stack([P.simulate(fac, x1, x2, s, case.T, sym, two) for s in seeds])


ACCEPT = [("mlp", "relu", "ntk", 2), ("resnet", "erf", "ntk", 2), ("resnet", "relu", "nngp", 2), ("mlp", "erf", "nngp", 1)]


@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("sym", [False, True], ids=["asym", "sym"])
@pytest.mark.parametrize("kind,act,get,layers", ACCEPT)
def test_acceptance_takes_the_rules_evaluated_in_T(kind, act, get, layers, sym, T):
    n = 40
    x1, x2 = (P.stored_rows("s")[:n],) * 2 if sym else (P.stored_rows("a1")[:n], P.stored_rows("a2")[:n])
    seeds = P.matching_seeds(n) if sym else P.shift_seeds(n, n)
    case = P.reference(kind, act, get, layers, P.B, x1, x2, seeds, T, sym)
    ratio, _ = P.hold(case, _simulated(case, case.fac_t, x1, x2, sym))
    assert ratio <= 1.125                                             # the yardstick's own error, and u / 2 <= max(Y, 4u) / 8 of the cast
    exact = _simulated(case, case.fac, x1, x2, sym)
    assert P.hold(case, exact)[0] <= 0.25                             # the long-double factors, rounded once: below 4 u
    if sym:                                                           # the trick's separate components, to the bit in long double
        rd = case.rd
        cross = (rd.side != 2) & (rd.xr[:, 6] != rd.xj[:, 6])
        a, b = np.where(rd.xr[cross, 6] == 0, 6, 7), np.where(rd.xr[cross, 6] == 0, 7, 6)
        f1 = case.fac.f1[rd.fr[cross], rd.fc[cross]]
        assert np.array_equal(case.ref[cross, a], rd.g[cross] * f1 / 8)
        f2 = np.where(rd.side[cross] == 0, case.fac.f2r[rd.fr[cross], rd.fc[cross]], case.fac.f2c[rd.fr[cross], rd.fc[cross]])
        assert np.array_equal(case.ref[cross, b], 2 * rd.g[cross] * f2 / 8)


MUTANTS = [("drop_phi1p", "mlp", "relu", "nngp"), ("swap_p", "mlp", "erf", "nngp"), ("swap_f2", "resnet", "relu", "ntk"),
           ("no_two", "mlp", "erf", "ntk"), ("no_TDA", "mlp", "relu", "ntk"), ("last_early", "resnet", "erf", "nngp"),
           ("no_lw2", "resnet", "relu", "nngp"), ("shift_col", "mlp", "relu", "nngp")]


MUTANT_CASES = [m + (sym,) for m in MUTANTS for sym in (False, True) if sym or m[0] != "swap_f2"]   # (no column side in the other)


@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mut,kind,act,get,sym", MUTANT_CASES, ids=["%s-%s" % (m[0], "sym" if m[4] else "asym") for m in MUTANT_CASES])
def test_acceptance_rejects_damaged_rules(mut, kind, act, get, sym, T):
    """Each damaged variant, evaluated in long double and rounded to T (so nothing but the damage is wrong), fails `hold`."""
    n = 40
    x1, x2 = (P.stored_rows("s")[:n],) * 2 if sym else (P.stored_rows("a1")[:n], P.stored_rows("a2")[:n])
    seeds = P.matching_seeds(n) if sym else P.shift_seeds(n, n)
    case = P.reference(kind, act, get, 2, P.B, x1, x2, seeds, T, sym)
    assert mut in P.MUTATIONS
    P.hold(case, _simulated(case, case.fac, x1, x2, sym))             # (undamaged: accepted)
    if mut == "no_two":
        bad = _simulated(case, case.fac, x1, x2, sym, two=1)
    elif mut == "shift_col":                                          # one pair of one call takes the neighbouring column's factors
        s = seeds[3]
        t = int(np.flatnonzero(s.r - s.j >= 2)[0]) if sym else 2
        j = s.j.copy()
        j[t] = (j[t] + 1) % n
        moved = list(seeds)
        moved[3] = P.Seed(s.r, j, s.g)
        bad = _simulated(case, case.fac, x1, x2, sym, seeds=moved)
    else:
        bad = _simulated(case, P.factors(kind, act, get, 2, P.B, x1, x2, L, mut=mut), x1, x2, sym)
    with pytest.raises(AssertionError):
        P.hold(case, bad)


# ------------------------------------------------------------------------------------------------------------ Y caps
import test_gpu_input_probes as G  # noqa: E402  (its case lists and builders; nothing in it touches the device at import)


@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
def test_every_gpu_case_keeps_its_bound_within_the_kernel_tolerance(T):
    """16 max(Y, 4u) <= tests/_tol.py's kernel tolerance for EVERY case of the GPU file, from the reference alone; and the guard
    hits of section C are exactly the constructed ones."""
    worst = {}
    for tag, build in G.all_cases(T):
        case = build()
        y = case.y if hasattr(case, "y") else case[2]
        assert P.FACTOR * max(y, 4 * P.U[T]) <= P.TOL[T], (tag, y / P.U[T])
        worst[tag.split()[0]] = max(worst.get(tag.split()[0], 0.0), y / P.U[T])
    print("\nlargest Y / u per section, %s: %s" % (np.dtype(T).name, " ".join("%s %.0f" % kv for kv in sorted(worst.items()))))
