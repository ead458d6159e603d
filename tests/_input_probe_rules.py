"""Per-pair probes of the input-gradient kernels (csrc/input_grad.hip, csrc/input_grad_sym.hip, the chain of
csrc/input_tangent.hpp): the rules in a NumPy scalar type of the caller's choice, exact inputs, seeds that read many pairs per
call, and the acceptance rule.  Shared by test_input_probe_host.py and test_gpu_input_probes.py; not a test module.

Rules.  tests/_input_grad_rules.factors restated so that ONE text runs in T = np.float32, np.float64 (the yardstick: what a
careful libm evaluation in the storage type loses) and np.longdouble (the reference), carries the column-side variance tangent
beside the row-side one, and returns per pair F_1 = dF/du, F_2 row side = dF/dv_r, F_2 column side = dF/dv_j, per row
ddiag = dK_rr/dv_r, and the guard hits.  Guards (the device's conventions, csrc/input_tangent.hpp): ReLU where (1 - c)(1 + c) <= 0
has D_A = D_1 = D_2 = 0; a zero-variance ReLU row has c = 0 and no variance-side term.  Two rows that are equal by construction
have c = 1 at EVERY activation and anti-parallel rows under b_std = 0 have c = -1 at the first: the rules set these exactly
(a later layer's c = A / sqrt(q_i q_j) is 1 only to rounding, in any precision).

Inputs are exact by construction: entries are multiples of 2^-6 with |x| <= 4 and d = 8 (near-duplicates: one entry on a finer
grid, chosen so that the sums still fit the storage type), so X X^T / d and |x|^2 / d are exact in T in any summation order: u and
v are known exactly and the chain is the only device arithmetic under test.  `exact_gram` asserts it for the inputs of every case
(`reference`, `dense_reference`).  The ordinary rows are stored (tests/golden/input_probe_rows.npz): random grid rows chosen so
that no pair sits beside a zero crossing of F_1 or F_2, where Y would leave the fp32 kernel tolerance (`select_rows`).

Reading.  gx[r, :] = sum_j G_rj (F_1 x_j + 2 F_2 x_r) / d depends on row r of the seed alone.  Two reserved feature columns
A, B: rows of role "P" have x[A] = 0, x[B] = 1, rows of role "Q" x[A] = 1, x[B] = 0.  Between a P row r and a Q row j, with
g = +-2^k and d = 8, gx[r, A] = g F_1 / d and gx[r, B] = 2 g F_2 / d to the bit.  The asymmetric entry takes x1 all P and x2 all
Q; the symmetric entry mixes the roles, so cross pairs show F_1, F_2 row and F_2 column in separate components of gx[i] and gx[j]
and same-role pairs are compared as vectors.

Seeds.  Asymmetric: one non-zero per row, G[r, (r + shift) mod n2] = g_r; n2 shifts cover every pair.  Symmetric: a perfect
matching per call (round-robin tournament), n - 1 rounds cover every off-diagonal pair; a diagonal seed reads ddiag.

Acceptance, per component e of every probed row:  |device - ref| <= 16 max(Y, 4 u_T) s_e (+ extra_e),
    s_e = |g| (|F_1 x_j[e]| + 2 |F_2 x_r[e]|) / d from the reference,
    Y   = the largest |rules_T - ref| / s_e over the case's readings (from the reference alone),
    16 and 4 u: the project's convention (tests/test_gpu_grad_probes.py),
and 16 max(Y, 4 u) may not exceed the project's kernel tolerance of the dtype (tests/_tol.py: 2e-3 / 1e-8).  Rows without a seed
entry must be exactly 0.  extra: `singular_allowance`, the derived absolute allowance at the pairs that sit ON a ReLU guard."""
import itertools

import numpy as np

L = np.longdouble
U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
TOL = {np.float32: 2e-3, np.float64: 1e-8}       # the project's kernel tolerances (tests/_tol.py)
FACTOR = 16.0
W, B, LW = 1.3, 0.4, 0.9
D = 8
MUTATIONS = ("drop_phi1p", "swap_p", "swap_f2", "no_two", "no_TDA", "last_early", "no_lw2", "shift_col")


def nsets_of(kind, layers):
    return layers if kind == "mlp" else layers + 1


# ------------------------------------------------------------------------------------------------------------ the rules
def _act(T, act, a, qi, qj, force=None, push=None):
    """(phi, D, phi_1, phi_2, D_A, D_1, D_2, hit) at pre-activation a [n1, n2], row variances qi [n1, 1], column variances
    qj [1, n2], all in T.  force: c where it is known by construction (NaN elsewhere).  push: delta, the entries on a guard take
    c = sign(c) (1 - delta) instead (singular_allowance).  hit: int8, sign(c) where the ReLU guard (1 - c)(1 + c) <= 0 holds."""
    pi = T(4) * np.arctan(T(1))
    one, two, zero = T(1), T(2), T(0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if act == "relu":
            sp = np.sqrt(qi * qj)
            ok = sp > 0
            c = np.clip(np.where(ok, a / np.where(ok, sp, one), zero), -one, one)
            if force is not None:
                c = np.where(np.isnan(force) | ~ok, c, force.astype(T))
            hit = np.where(ok & ~((one - c) * (one + c) > 0), np.sign(c), zero).astype(np.int8)
            if push is not None:
                c = np.where(hit != 0, hit.astype(T) * (one - T(push)), c)
            om = (one - c) * (one + c)
            flat = ~(om > 0)
            s1 = np.sqrt(np.maximum(om, zero))
            pm = pi - np.arccos(c)
            phi = sp * (s1 + pm * c) / (two * pi)
            big_d = pm / (two * pi)
            qig, qjg = np.where(qi > 0, qi, one), np.where(qj > 0, qj, one)
            p1 = np.where(qi > 0, s1 * sp / (T(4) * pi * qig), zero)
            p2 = np.where(qj > 0, s1 * sp / (T(4) * pi * qjg), zero)
            inv = np.where(flat, zero, one / (two * pi * np.where(flat, one, s1)))
            d_a = np.where(ok, inv / np.where(ok, sp, one), zero)
            d_1 = np.where(qi > 0, -inv * c / (two * qig), zero)
            d_2 = np.where(qj > 0, -inv * c / (two * qjg), zero)
            return phi, big_d, p1, p2, d_a, d_1, d_2, hit
        if act == "erf":
            ti, tj = one + two * qi, one + two * qj
            p = ti * tj
            sp = np.sqrt(p)
            s = np.clip(two * a / sp, -one, one)
            om = np.maximum((one - s) * (one + s), T(np.finfo(T).tiny))
            den = np.sqrt(om)
            r15 = (p * om) * (sp * den)
            return ((two / pi) * np.arcsin(s), T(4) / (pi * sp * den), -(two / pi) * s / (den * ti), -(two / pi) * s / (den * tj),
                    T(16) * a / (pi * r15), -T(4) * tj / (pi * r15), -T(4) * ti / (pi * r15), np.zeros(np.shape(a), np.int8))
    raise KeyError(act)


def _act_diag(T, act, q):
    """(phi, phi', D, D') on the diagonal as functions of the variance q entering the activation."""
    pi = T(4) * np.arctan(T(1))
    if act == "relu":
        return q / T(2), np.full_like(q, T(0.5)), np.full_like(q, T(0.5)), np.zeros_like(q)
    t1, t2 = T(1) + T(2) * q, T(1) + T(4) * q
    r2 = np.sqrt(t2)
    return (T(2) / pi) * np.arcsin(T(2) * q / t1), (T(4) / pi) / (t1 * r2), (T(4) / pi) / r2, -(T(8) / pi) / (t2 * r2)


def _diag_chain(T, kind, act, q0, nsets, w2, b2):
    """Per row: the (q, p = dq/dq0) entering each activation, and (q', theta') behind the last one."""
    q, qt = q0.copy(), np.ones_like(q0)
    th, tht = np.zeros_like(q0), np.zeros_like(q0)
    if kind == "resnet":
        q, qt = w2 * q + b2, w2 * qt
        th, tht = q.copy(), qt.copy()
    sets = []
    for s in range(nsets):
        if kind == "mlp":
            q, qt = w2 * q + b2, w2 * qt
            th, tht = q + w2 * th, qt + w2 * tht
        sets.append((q, qt))
        o, oq, dd, ddq = _act_diag(T, act, q)
        ot, to, tot = oq * qt, th * dd, tht * dd + th * ddq * qt
        if kind == "resnet" and s != nsets - 1:
            a2, a2t = w2 * o + b2, w2 * ot
            q, qt, th, tht = q + a2, qt + a2t, th + a2 + w2 * to, tht + a2t + w2 * tot
        else:
            q, qt, th, tht = o, ot, to, tot
    return sets, (qt, tht)


class Factors:
    """f1, f2r, f2c [n1, n2], ddiag [n1] in T; hits [nsets, n1, n2] int8 (the sign of c on a ReLU guard); zero1 [n1], zero2 [n2]:
    rows whose variance is 0 at the first activation."""


def in_T(a, T):
    """An exact host value in T; it must be representable."""
    a = np.asarray(a, L)
    out = a.astype(T)
    assert np.array_equal(out.astype(L), a), "the inputs are not exact in %s" % np.dtype(T).name
    return out


def factors(kind, act, get, layers, b_std, x1, x2, T, mut=None, push=None):
    """The rules at every pair (r, j) of x1 [n1, d] x x2 [n2, d] (exact values), arithmetic in T throughout.  u = (x1 . x2) / d
    and v = |x|^2 / d take one rounding in T (none when d = 8).  mut: one of MUTATIONS (a damaged variant for the host test).
    push: per activation a delta or None, for singular_allowance."""
    x1l, x2l = np.asarray(x1, L), np.asarray(x2, L)
    d = x1l.shape[1]
    nsets = nsets_of(kind, layers)
    w2, b2 = T(float(W) * float(W)), T(float(b_std) * float(b_std))
    lw2 = T(1) if mut == "no_lw2" else T(float(LW) * float(LW))
    ntk = {"nngp": False, "ntk": True}[get]
    k = in_T(x1l @ x2l.T, T) / T(d)
    v1 = in_T((x1l * x1l).sum(1), T) / T(d)
    v2 = in_T((x2l * x2l).sum(1), T) / T(d)
    rows, (qt_f, tht_f) = _diag_chain(T, kind, act, v1, nsets, w2, b2)
    cols, _ = _diag_chain(T, kind, act, v2, nsets, w2, b2)
    same = (x1l[:, None, :] == x2l[None, :, :]).all(-1) & ((v1 > 0)[:, None] | (b2 > 0))
    anti = (x1l[:, None, :] == -x2l[None, :, :]).all(-1) & (v1 > 0)[:, None] & (b2 == 0)
    ku, kv, kc = np.ones_like(k), np.zeros_like(k), np.zeros_like(k)
    th, thu, thv, thc = (np.zeros_like(k) for _ in range(4))
    if kind == "resnet":
        k, ku = w2 * k + b2, w2 * ku
        th, thu = k.copy(), ku.copy()
    hits = np.zeros((nsets,) + k.shape, np.int8)
    last_at = nsets - 2 if mut == "last_early" else nsets - 1
    for s in range(nsets):
        a, au, av, ac, tt, tu, tv, tc = k, ku, kv, kc, th, thu, thv, thc
        if kind == "mlp":
            a, au, av, ac = w2 * k + b2, w2 * ku, w2 * kv, w2 * kc
            tt, tu, tv, tc = a + w2 * th, au + w2 * thu, av + w2 * thv, ac + w2 * thc
        (qi, pr), (qj, pc) = rows[s], cols[s]
        pr, pc = pr[:, None], pc[None, :]
        if mut == "swap_p":
            pr, pc = pc + np.zeros_like(k), pr + np.zeros_like(k)
        force = np.where(same, 1.0, np.where(anti & (s == 0), -1.0, np.nan)) if act == "relu" else None
        phi, big_d, p1, p2, d_a, d_1, d_2, hits[s] = _act(T, act, a, qi[:, None], qj[None, :], force, None if push is None else push[s])
        o, ou = phi, big_d * au
        ov = big_d * av + (T(0) if mut == "drop_phi1p" else p1 * pr)
        oc = big_d * ac + p2 * pc
        du, dv, dc = d_a * au, d_a * av + d_1 * pr, d_a * ac + d_2 * pc
        if mut == "no_TDA":
            du = np.zeros_like(du)
        to, tou, tov, toc = tt * big_d, tu * big_d + tt * du, tv * big_d + tt * dv, tc * big_d + tt * dc
        if kind == "resnet" and s != last_at:
            a2, a2u, a2v, a2c = w2 * o + b2, w2 * ou, w2 * ov, w2 * oc
            o, ou, ov, oc = a + a2, au + a2u, av + a2v, ac + a2c
            to, tou, tov, toc = tt + a2 + w2 * to, tu + a2u + w2 * tou, tv + a2v + w2 * tov, tc + a2c + w2 * toc
        k, ku, kv, kc, th, thu, thv, thc = o, ou, ov, oc, to, tou, tov, toc
    f = Factors()
    f.f1 = lw2 * (ku + thu if ntk else ku)
    f.f2r = lw2 * (kv + thv if ntk else kv)
    f.f2c = lw2 * (kc + thc if ntk else kc)
    if mut == "swap_f2":
        f.f2r, f.f2c = f.f2c, f.f2r
    f.ddiag = lw2 * (qt_f + tht_f if ntk else qt_f)
    f.hits = hits
    f.zero1 = np.asarray(rows[0][0] == 0) if nsets else np.zeros(len(v1), bool)
    f.zero2 = np.asarray(cols[0][0] == 0) if nsets else np.zeros(len(v2), bool)
    for a in (f.f1, f.f2r, f.f2c, f.ddiag):
        assert a.dtype == np.dtype(T)
    return f


# ------------------------------------------------------------------------------------------------------------- inputs
def exact_gram(x1, x2, T=np.float32):
    """Asserts that x1 x2^T and the squared row norms, accumulated in T, are the long-double values (so they are exact in T in any
    summation order: every partial sum is a multiple of the same unit below the same bound)."""
    for a, b in ((x1, x2), (x1, x1), (x2, x2)):
        a, b = np.asarray(a), np.asarray(b)
        assert np.array_equal(a.astype(T).astype(np.float64), a) and np.array_equal(b.astype(T).astype(np.float64), b)
        got = (a.astype(T)[:, None, :] * b.astype(T)[None, :, :])
        acc = np.zeros(got.shape[:2], T)
        for e in range(got.shape[2]):
            acc = acc + got[:, :, e]
        rev = np.zeros(got.shape[:2], T)
        for e in reversed(range(got.shape[2])):
            rev = rev + got[:, :, e]
        want = a.astype(L) @ b.astype(L).T
        assert np.array_equal(acc.astype(L), want) and np.array_equal(rev.astype(L), want), "the Gram matrix is not exact in T"
        if a.shape[1] == 8:
            assert np.array_equal((acc / T(8)).astype(L), want / L(8))


def grid_rows(n, seed, role=None, d=D):
    """n rows of d entries, multiples of 2^-6 in [-4, 4]; the last two columns (A = d - 2, B = d - 1) carry the role: "P" (0, 1),
    "Q" (1, 0), "mix" (either, at random) or None (ordinary entries)."""
    x = np.random.default_rng([20261021, n, seed]).integers(-256, 257, size=(n, d)).astype(np.float64) / 64.0
    if role is not None:
        mix = np.random.default_rng([20261021, n, seed, 1]).random(n) < 0.5
        p = mix if role == "mix" else np.full(n, role == "P")
        x[:, d - 2] = np.where(p, 0.0, 1.0)
        x[:, d - 1] = np.where(p, 1.0, 0.0)
    x.setflags(write=False)
    return x


FORMS = [(kind, act, get) for kind in ("mlp", "resnet") for act in ("relu", "erf") for get in ("nngp", "ntk")]
SELECT_Y = 1024.0   # in units of u_32: half of what the fp32 kernel tolerance allows Y, 2e-3 / 16 = 2097 u


def _pairs_ok(xa, xb, sym, layers=2, b_std=B):
    """[na, nb] bool: no factor of the pair loses more than SELECT_Y u to a float32 evaluation, in any form (select_rows)."""
    ok = np.ones((len(xa), len(xb)), bool)
    for kind, act, get in FORMS:
        ref, val = (factors(kind, act, get, layers, b_std, xa, xb, T) for T in (L, np.float32))
        for name in ("f1", "f2r", "f2c") if sym else ("f1", "f2r"):
            a, b = getattr(ref, name), getattr(val, name).astype(L)
            with np.errstate(divide="ignore", invalid="ignore"):
                ok &= ~(np.abs(a - b) > L(SELECT_Y * U[np.float32]) * np.abs(a))
    return ok


def select_rows(n, seed, role, against=None, d=D, pool=96):
    """n grid rows in which no pair (against None: among themselves; else: with every row of `against`) sits beside a zero
    crossing of F_1 or F_2: F_2 changes sign inside the range of ordinary correlations (erf near u = -b2 / w2, ReLU NTK near
    c = 0.7), and a reading that isolates it has the scale |F_2|, so among 10^4 random pairs the closest one to the crossing
    would alone put Y above what the fp32 kernel tolerance allows.  Greedy over pools of random grid rows; the criterion is the
    reference's own (float32 rules against long double, _pairs_ok).  This is how tests/golden/input_probe_rows.npz was made
    (make_golden); the host test re-checks the Y caps on the stored rows."""
    sym = against is None
    rows, t = np.zeros((0, d)), 0
    while len(rows) < n:
        cand = np.array(grid_rows(pool, 1000 * seed + t, role, d))
        t += 1
        if sym:
            good = (_pairs_ok(cand, rows, True).all(1) & _pairs_ok(rows, cand, True).all(0)) if len(rows) else np.ones(pool, bool)
            among = _pairs_ok(cand, cand, True)
            among = among & among.T
        else:
            good = _pairs_ok(against, cand, False).all(0)
        taken = []
        for c in np.flatnonzero(good):
            if sym and not all(among[c, k] for k in taken):
                continue
            taken.append(c)
            rows = np.vstack([rows, cand[c:c + 1]])
            if len(rows) == n:
                break
    return rows


GOLDEN = "golden/input_probe_rows.npz"


def make_golden(path):
    """The stored input sets (numerators over 64, int16)."""
    out = {}
    out["a1"] = np.array(grid_rows(130, 1, "P"))
    out["a2"] = select_rows(257, 2, "Q", against=out["a1"])          # A, D: x2 (its first 130 rows: n2 = 130)
    out["s"] = select_rows(257, 3, "mix")                            # B, D: x (its first 130 rows: n = 130)
    out["f1"] = np.array(grid_rows(66, 4, "P", d=7))
    out["f2"] = select_rows(66, 5, "Q", against=out["f1"], d=7)      # F: d = 7
    out["fs"] = select_rows(66, 6, "mix", d=7)
    np.savez_compressed(path, **{k: np.round(v * 64).astype(np.int16) for k, v in out.items()})


def stored_rows(name):
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), GOLDEN)) as z:
        x = z[name].astype(np.float64) / 64.0
    x.setflags(write=False)
    return x


# x_j = x_r + 2^-k e_0.  The Gram matrix stays exact in T up to k = 8 (f32) and k = 23 (f64); the gaps used are the smallest at
# which 16 Y stays within the kernel tolerance over ten pairs and every form: 1 - c ~ 2e-4 in f32 (at k = 7, 8 Y reaches 3000 u
# against the 2097 u allowed) and ~ 1e-11 in f64 (k = 20: 1.2e7 u against 5.6e6 u), and in f64 two wider ones beside it, so
# that 1 - c runs over 2e-3, 7e-4, 2e-4 (f32) and 1e-5, 1e-8, 1e-11 (f64).  The host test holds both conditions.
NEAR_K = {np.float32: (4, 5, 6), np.float64: (8, 13, 18)}
NEAR_PAIRS = 10                                            # per gap: Y is a largest rounding error, a handful of pairs is a lottery
ORDINARY = (0, 1, 63, 64, 65, 127)                         # rows of the hard inputs that stay ordinary grid rows
ANTI, DUP = ((44, 45), (46, 110)), ((50, 60), (51, 120))
ZERO_ROW = 90
SCALED = tuple(range(100, 107))                            # rows 2^s b_s, s = -6, -4, ..., 6
HARD_N = 130


def near_pairs(t):
    """The (r, j) of gap number t: four partners in r's own 64-row tile, five in the next, one in the ragged last tile (t < 2)."""
    r = [2 + 10 * t + p for p in range(NEAR_PAIRS)]
    j = [32 + 4 * t + p for p in range(4)] + [66 + 5 * t + p for p in range(5)] + [(128, 129, 126)[t]]
    return list(zip(r, j))


def hard_inputs(T):
    """(x [130, 8], {case: [(r, j)]}) of section C: near-duplicates at NEAR_K[T], anti-parallel rows, exactly duplicate rows, an
    all-zero row, rows scaled by 2^-6 ... 2^6.  Every case lists its pairs once, r < j."""
    x = np.array(grid_rows(HARD_N, 7))
    rng = np.random.default_rng(20261022)
    cases = {}
    for t, k in enumerate(NEAR_K[T]):
        cases["near%d" % k] = near_pairs(t)
        for r, j in cases["near%d" % k]:
            x[r] = rng.integers(-32, 33, size=D) / 64.0      # short rows: the gap in c is 2^-2k sin^2 / (2 |x|^2)
            x[j] = x[r]
            x[j, 0] += 2.0 ** -k
    for r, j in ANTI:
        x[j] = -x[r]
    for r, j in DUP:
        x[j] = x[r]
    x[ZERO_ROW] = 0.0
    for t, r in enumerate(SCALED):
        x[r] = rng.integers(-3, 4, size=D) * 2.0 ** (2 * t - 6)
        x[r, t % D] = 2.0 ** (2 * t - 6)                     # never all zero
    cases["anti"], cases["dup"] = list(ANTI), list(DUP)
    cases["zero"] = [tuple(sorted((ZERO_ROW, j))) for j in ORDINARY + (129, DUP[0][0], SCALED[0], SCALED[-1])]
    cases["scaled"] = [(a, b) for a, b in itertools.combinations(SCALED, 2)] + [
        tuple(sorted((a, b))) for a in SCALED for b in ORDINARY[::2]]
    x.setflags(write=False)
    return x, cases


# -------------------------------------------------------------------------------------------------------------- seeds
class Seed:
    """One call's seed: entries G[r[t], j[t]] = g[t].  Asymmetric entry: every r at most once.  Symmetric entry: r >= j, every
    row at most once over r and j together (a matching, or diagonal entries r == j)."""

    def __init__(self, r, j, g):
        self.r, self.j, self.g = np.asarray(r, np.int64), np.asarray(j, np.int64), np.asarray(g, np.float64)


def seed_values(count, key):
    """+-2^k, k in -2 .. 2."""
    rng = np.random.default_rng([count, key])
    return np.where(rng.random(count) < 0.5, -1.0, 1.0) * 2.0 ** rng.integers(-2, 3, size=count)


def shift_seeds(n1, n2, shifts=None):
    """G[r, (r + shift) mod n2] = g_r: with every shift in range(n2), every pair exactly once."""
    r = np.arange(n1)
    return [Seed(r, (r + s) % n2, seed_values(n1, s)) for s in (range(n2) if shifts is None else shifts)]


def round_robin(n):
    """The rounds of a round-robin tournament over n rows (the circle method): n - 1 rounds of n / 2 pairs (n even), n rounds with
    one bye each (n odd).  Every unordered pair occurs exactly once."""
    m = n + (n % 2)
    out = []
    for t in range(m - 1):
        pairs = [(m - 1, t)] + [((t + k) % (m - 1), (t - k) % (m - 1)) for k in range(1, m // 2)]
        out.append([(max(a, b), min(a, b)) for a, b in pairs if max(a, b) < n])
    return out


def matching_seeds(n):
    """The n - 1 (n) rounds, lower-triangle entries, then the diagonal seed."""
    out = []
    for t, pairs in enumerate(round_robin(n)):
        if pairs:
            i, j = np.array(pairs).T
            out.append(Seed(i, j, seed_values(len(i), t)))
    out.append(Seed(np.arange(n), np.arange(n), seed_values(n, n + 7)))
    return out


def pack_pairs(pairs, sym):
    """Seeds that read the given pairs, each once: greedily, a row at most once per seed (sym: over both sides; entries i > j)."""
    seeds, left, t = [], [tuple(p) for p in pairs], 0
    while left:
        used, take, rest = set(), [], []
        for a, b in left:
            keys = (a, b) if sym else (a,)
            if used.isdisjoint(keys):
                used.update(keys)
                take.append((max(a, b), min(a, b)) if sym else (a, b))
            else:
                rest.append((a, b))
        r, j = np.array(take).T
        seeds.append(Seed(r, j, seed_values(len(r), 100 + t)))
        left, t = rest, t + 1
    return seeds


def dense_matrix(seed, n1, n2, T, sym=False):
    """The seed as the matrix the entry takes; sym: the strict upper triangle is NaN (the lower triangle is what is read)."""
    g = np.zeros((n1, n2), T)
    g[seed.r, seed.j] = seed.g.astype(T)
    if sym:
        assert (seed.r >= seed.j).all()
        g[np.triu_indices(n1, 1)] = np.nan
    return g


# ----------------------------------------------------------------------------------------------------------- readings
class Readings:
    """What the seeds of a case make the entry return: per reading t, gx[seed[t], row[t], :] = g (F_1 xj + 2 F_2 xr) / d."""


def readings(seeds, x1, x2, sym):
    """Index arrays: seed, row (the row of gx), fr / fc (the factor entry), side (0: F_2 row side, 1: F_2 column side, 2: the
    diagonal, F_1 = 0 and F_2 = ddiag / 2), xr (the row's own inputs), xj (the partner's), g."""
    sd, row, fr, fc, side, xr, xj, g = ([] for _ in range(8))
    for t, s in enumerate(seeds):
        if sym:
            assert len(set(s.r[s.r != s.j]) | set(s.j[s.r != s.j])) == 2 * int((s.r != s.j).sum())
        else:
            assert len(set(s.r)) == len(s.r)
        dg = (s.r == s.j) if sym else np.zeros(len(s.r), bool)
        parts = [(s.r, np.where(dg, 2, 0), s.r, s.j)]
        if sym:
            parts.append((s.j[~dg], np.ones(int((~dg).sum()), np.int64), s.j[~dg], s.r[~dg]))
        for p, (rw, sde, own, partner) in enumerate(parts):
            keep = slice(None) if p == 0 else ~dg
            sd.append(np.full(len(rw), t)); row.append(rw); side.append(sde)
            fr.append(s.r[keep]); fc.append(s.j[keep]); g.append(s.g[keep])
            xr.append(np.asarray(x1)[own]); xj.append(np.asarray(x2)[partner])
    rd = Readings()
    rd.seed, rd.row, rd.fr, rd.fc, rd.side, rd.g = (np.concatenate(a) for a in (sd, row, fr, fc, side, g))
    rd.xr, rd.xj = np.concatenate(xr).astype(L), np.concatenate(xj).astype(L)
    rd.nseeds, rd.n1, rd.d = len(seeds), len(x1), np.asarray(x1).shape[1]
    return rd


def components(rd, fac, two=2):
    """(value [P, d], scale [P, d]) in long double from the factors of `fac` (any T)."""
    f1 = np.where(rd.side == 2, L(0), fac.f1.astype(L)[rd.fr, rd.fc])
    f2 = np.select([rd.side == 0, rd.side == 1], [fac.f2r.astype(L)[rd.fr, rd.fc], fac.f2c.astype(L)[rd.fr, rd.fc]],
                   fac.ddiag.astype(L)[rd.fr] / L(2))
    a, b = f1[:, None] * rd.xj, L(two) * f2[:, None] * rd.xr
    g = rd.g.astype(L)[:, None]
    return g * (a + b) / L(rd.d), np.abs(g) * (np.abs(a) + np.abs(b)) / L(rd.d)


def yardstick(val_t, ref, s):
    """Y: the largest |rules_T - ref| / s over the readings' components (0 where the scale is 0 and the values agree)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(s > 0, np.abs(val_t - ref) / s, np.where(val_t == ref, L(0), L(np.inf)))
    return float(r.max()) if r.size else 0.0


def singular_allowance(kind, act, get, layers, b_std, x1, x2, T, rd, ref_fac):
    """The ABSOLUTE allowance [P, d] at the readings whose pair sits ON a ReLU guard at some activation (exactly duplicate rows,
    anti-parallel rows under b_std = 0); 0 elsewhere and for erf.

    There the maps are not differentiable: phi_1 ~ sqrt(1 - c^2) has an infinite slope in c and D_A, D_1, D_2 ~ 1 / sqrt(1 - c^2)
    are unbounded; the rules and the device's guard take phi_1 = D_A = D_1 = D_2 = 0.  The device forms c~ = A ra_i ra_j from
    rounded tables and its own rounded chain, which is +-1 only to rounding: |c~| = 1 - delta with delta = 0 (the guard), or
    u <= delta <= dmax = (2 nsets + 5) u, the count tests/_kernel_budget.py moves a correlation by (tests/_grad_probe_rules.py:
    duplicate_allowance).  Then phi_1 = sqrt(2 delta) (...) and D_A = 1 / sqrt(2 delta) (...): to first order the deviation of
    F_1, F_2 from the guarded value is linear in (sqrt(delta_l), 1 / sqrt(delta_l)) per activation l, and a x + b / x on
    [sqrt(u), sqrt(dmax)] takes its largest magnitude at an end.  The allowance is taken over the rules in long double run with
    delta_l in {guard, u, dmax} at every activation (3^nsets runs, the approximation's own error carried through the remaining
    layers), and per run it is
        |value - ref|  +  dmax s(run).
    The first term is small, O(sqrt(delta)) s: c is extremal in x_r where |c| = 1, so in gx = g (F_1 x_j + 2 F_2 x_r) / d the
    unbounded parts of F_1 and F_2 cancel (x_j = +-x_r) and only the sqrt(delta) parts stay.  The second is the rounding of that
    cancelling sum: the device adds two terms of the run's own scale s(run) = |g| (|F_1 x_j| + 2 |F_2 x_r|) / d, which at
    delta = u is s / sqrt(2 u) / (2 pi) for the NTK forms, each known to the dmax relative that c~ itself is known to
    (duplicate_allowance counts its cancelling sum the same way)."""
    nsets = nsets_of(kind, layers)
    on_guard = (ref_fac.hits != 0).any(axis=0)[rd.fr, rd.fc] & (rd.side != 2)
    ref, _ = components(rd, ref_fac)
    extra = np.zeros(ref.shape, L)
    if act != "relu" or not on_guard.any():
        return extra
    dmax = (2 * nsets + 5) * U[T]
    for deltas in itertools.product((None, U[T], dmax), repeat=nsets):
        if all(dl is None for dl in deltas):
            continue
        run = factors(kind, act, get, layers, b_std, x1, x2, L, push=[0.0 if dl is None else dl for dl in deltas])
        val, s_run = components(rd, run)
        extra = np.maximum(extra, np.where(on_guard[:, None], np.abs(val - ref) + L(dmax) * s_run, L(0)))
    return extra


class Case:
    """The reference of one case: readings, ref and scale [P, d], Y, extra [P, d], bound factor."""


def reference(kind, act, get, layers, b_std, x1, x2, seeds, T, sym):
    c = Case()
    exact_gram(x1, x2, T)
    c.rd = readings(seeds, x1, x2, sym)
    c.fac = factors(kind, act, get, layers, b_std, x1, x2, L)
    c.fac_t = factors(kind, act, get, layers, b_std, x1, x2, T)
    c.ref, c.s = components(c.rd, c.fac)
    c.val_t, _ = components(c.rd, c.fac_t)
    c.y = yardstick(c.val_t, c.ref, c.s)
    c.yy = max(c.y, 4.0 * U[T])
    c.extra = singular_allowance(kind, act, get, layers, b_std, x1, x2, T, c.rd, c.fac)
    c.T, c.seeds = T, seeds
    return c


def hold(case, gx, tag=""):
    """gx [nseeds, n1, d]: what the entry returned per seed.  Asserts every reading's components within 16 max(Y, 4 u) s + extra,
    every other row exactly 0, 16 max(Y, 4 u) within the kernel tolerance.  Returns (largest (err - extra) / (max(Y, 4u) s),
    largest err / extra where an allowance applies)."""
    rd, T = case.rd, case.T
    gx = np.asarray(gx)
    assert gx.shape == (rd.nseeds, rd.n1, rd.d) and np.isfinite(gx).all(), tag
    assert FACTOR * case.yy <= TOL[T], "%s: 16 max(Y, 4u) = %.3g exceeds the kernel tolerance" % (tag, FACTOR * case.yy)
    probed = np.zeros(gx.shape[:2], bool)
    assert not probed[rd.seed, rd.row].any()
    probed[rd.seed, rd.row] = True
    assert probed.sum() == len(rd.seed), tag + ": a row is read twice in one call"
    assert not gx[~probed].any(), tag + ": a row without a seed entry is not exactly zero"
    err = np.abs(gx[rd.seed, rd.row].astype(L) - case.ref)
    over = np.maximum(err - case.extra, L(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(case.s > 0, over / (L(case.yy) * case.s), np.where(over == 0, L(0), L(np.inf)))
        used = np.where(case.extra > 0, err / case.extra, L(0))
    worst = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else (0, 0)
    assert (over <= FACTOR * L(case.yy) * case.s).all(), "%s: ratio %.3g at seed %d row %d (factor entry %d, %d) component %d" % (
        tag, float(ratio.max()), rd.seed[worst[0]], rd.row[worst[0]], rd.fr[worst[0]], rd.fc[worst[0]], worst[1])
    return (float(ratio.max()) if ratio.size else 0.0), (float(used.max()) if used.size else 0.0)


# ------------------------------------------------------------------------------------- a host model of the two entries
def simulate(fac, x1, x2, seed, T, sym, two=2):
    """gx [n1, d] of one call from the factors `fac`, by the dense formulas of the two entries (not through `readings`):
    asymmetric ((G o F_1) X2 + 2 rowsum(G o F_2) o x1) / d; symmetric (W X + (2 r + G_nn ddiag_n) x_n) / d with the symmetric
    completion of the lower-triangle seed."""
    x1l, x2l = np.asarray(x1, L), np.asarray(x2, L)
    n1, n2 = len(x1l), len(x2l)
    g = np.zeros((n1, n2), L)
    g[seed.r, seed.j] = seed.g
    f1, f2 = fac.f1.astype(L), fac.f2r.astype(L)
    if sym:
        low = np.tril(np.ones((n1, n1), bool), -1)
        f1 = np.where(low, f1, f1.T)                                    # the pass evaluates the lower entry (i, j), i > j
        f2 = np.where(low, f2, fac.f2c.astype(L).T)
        dg = np.diag(g).copy()
        g = g + np.tril(g, -1).T
        np.fill_diagonal(g, 0)
        out = ((g * f1) @ x2l + (L(two) * (g * f2).sum(1) + dg * fac.ddiag.astype(L))[:, None] * x1l) / L(x1l.shape[1])
    else:
        out = ((g * f1) @ x2l + L(two) * (g * f2).sum(1)[:, None] * x1l) / L(x1l.shape[1])
    return out.astype(T)


# ------------------------------------------------------------------------------------------------------- dense seeds
def dense_seed(n1, n2, T, sym):
    g = np.random.default_rng([20261023, n1, n2]).standard_normal((n1, n2))
    if sym:
        g = (g + g.T) / 2.0
    return g.astype(T)


def dense_reference(kind, act, get, layers, b_std, x1, x2, g, T, sym):
    """(ref [n1, d], bound scale [n1, d], Y): gx under a full seed, sum_j |G_rj| s_e(r, j) and the yardstick over ALL pairs (and,
    sym, the diagonal), in long double from the stored seed."""
    exact_gram(x1, x2, T)
    x1l, x2l, gl = np.asarray(x1, L), np.asarray(x2, L), np.asarray(g, L)
    d = x1l.shape[1]
    out = []
    for T_ in (L, T):
        fac = factors(kind, act, get, layers, b_std, x1, x2, T_)
        f1, f2 = fac.f1.astype(L), fac.f2r.astype(L)
        if sym:
            np.fill_diagonal(f1, 0)
            np.fill_diagonal(f2, fac.ddiag.astype(L) / 2)
        a = f1[:, :, None] * x2l[None, :, :]                           # [n1, n2, d]
        b = 2 * f2[:, :, None] * x1l[:, None, :]
        out.append(((a + b) / d, (np.abs(a) + np.abs(b)) / d))
    (val, s), (val_t, _) = out
    y = yardstick(val_t, val, s)
    return (gl[:, :, None] * val).sum(1), (np.abs(gl)[:, :, None] * s).sum(1), y
