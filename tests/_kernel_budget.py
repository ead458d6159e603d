"""Rounding-level error budgets for the dense NNGP / NTK kernel build, in vectorised NumPy fp64 (a helper, not a test module).

The budget is the rule of the mpmath fixture (tests/golden/make_mp_golden.py, `kernel_with_budget`) restated for arrays of
entries, so that matrices of more than one tile can be held to it (the fixture's mp loops take a second per entry):

    reference   the layer recursion of the entry (K0_ij, q_i, q_j);
    push        the same recursion with the correlation rho = K / sqrt(q_i q_j) of EVERY activation moved by
                +-(d_terms + 2 L + 4) u, clamped to [-1, 1]; the larger of the two deviations;
    final       plus (2 L + 4) u (|K_ij| + sqrt(K_ii K_jj)).

d_terms counts the roundings of the input Gram: d for inputs whose products round (the fixture's sets, `gauss`), 2 for the
`exact` inputs below (integer rows: the sum is exact in any order, what is left is the rounded 1 / d and its product), 1 for a
stored K0 that was rounded once (smn_recursion).  u = 2^-24 (f32) or 2^-53 (f64).  Diagonal entries of a symmetric build take
rho = 1 exactly at every layer, as the device's closed-form diagonal does (in fp64, k / sqrt(q q) is 1 - 1e-16 and Kdot of
ReLU would carry the square root of that).

tests/test_kernel_budget_host.py holds this port to the fixture (budgets within 1e-4 relative, references within 1 % of the
f32 budget) and to mpmath at 40 digits on a sample of the large inputs.  Its reference is a rounded fp64 evaluation, so inputs
must stay away from |rho| = 1 off the diagonal, where J and Kdot have square-root sensitivity: both generators assert
1 - |c0| >= 1e-3 for every pair of rows.
"""
import numpy as np

U = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
NPT = {"f64": np.float64, "f32": np.float32}
TILE = 128                   # the build's tile; BM = 64 half tiles split it between local rows 63 and 64
FULL_LIMIT = 4 * 1000 * 1000  # matrices of up to this many entries are checked in full
PI = np.pi


# ----------------------------------------------------------------------------------------------------------- the rule
def _act_map(act, k, qi, qj, push, diag):
    """make_mp_golden.act_map for arrays.  diag: boolean mask (or None) of entries whose rho is 1 exactly.  The recursions
    pass it at every activation of the nominal run (where k = q stays true) and at the first one of a pushed run (behind it
    the pushed diagonal entry has left rho = 1 like any other)."""
    sp = np.sqrt(qi * qj)
    zero = sp == 0
    rho = np.where(zero, 0.0, k / np.where(zero, 1.0, sp))
    if diag is not None:
        rho = np.where(diag & ~zero, 1.0, rho)
    if push:
        rho = rho + np.where(rho >= 0, push, -push)
    rho = np.clip(rho, -1.0, 1.0)
    if push or diag is not None:
        k = np.where(zero, k, rho * sp)
    if act == "relu":
        s = np.sqrt((1.0 - rho) * (1.0 + rho))
        back = PI - np.arctan2(s, rho)          # pi - acos(rho), without the cancellation of arccos at rho -> 1
        return sp * (s + back * rho) / (2 * PI), back / (2 * PI), qi / 2, qj / 2
    pij = (1 + 2 * qi) * (1 + 2 * qj)
    c = np.clip(2 * k / np.sqrt(pij), -1.0, 1.0)
    kd = 4 / (PI * np.sqrt(pij - 4 * k * k))
    return (2 / PI * np.arcsin(c), kd, 2 / PI * np.arcsin(2 * qi / (1 + 2 * qi)), 2 / PI * np.arcsin(2 * qj / (1 + 2 * qj)))


def _mlp(k, qi, qj, L, act, w, b, lw, push=0.0, diag=None):
    """make_mp_golden.mlp_entry: L x [Dense(w, b); act]; Dense(lw, 0)."""
    w2, b2, lw2 = w * w, b * b, lw * lw
    th = np.zeros_like(k)
    for layer in range(L):
        k, qi, qj = w2 * k + b2, w2 * qi + b2, w2 * qj + b2
        th = k + w2 * th
        k, kd, qi, qj = _act_map(act, k, qi, qj, push, diag if layer == 0 or not push else None)
        th = th * kd
    k = lw2 * k
    return k, k + lw2 * th


def _resnet(k, qi, qj, L, act, w, b, lw, push=0.0, diag=None):
    """make_mp_golden.resnet_entry: Dense; L x {(act; Dense) + Identity}; act; Dense(lw, 0)."""
    w2, b2, lw2 = w * w, b * b, lw * lw
    k, qi, qj = w2 * k + b2, w2 * qi + b2, w2 * qj + b2
    th = k
    for layer in range(L):
        kb, kd, qib, qjb = _act_map(act, k, qi, qj, push, diag if layer == 0 or not push else None)
        tb = th * kd
        kb, qib, qjb = w2 * kb + b2, w2 * qib + b2, w2 * qjb + b2
        tb = kb + w2 * tb
        k, qi, qj, th = k + kb, qi + qib, qj + qjb, th + tb
    k, kd, qi, qj = _act_map(act, k, qi, qj, push, diag if L == 0 or not push else None)
    th = th * kd
    k = lw2 * k
    return k, k + lw2 * th


ENTRY = {"mlp": _mlp, "resnet": _resnet}


def row_kernel(net, act, L, w, b, lw, q):
    """(K(x, x), Theta(x, x)) of rows with input variance q: the scale of an entry's row and column."""
    q = np.asarray(q, np.float64)
    with np.errstate(all="ignore"):
        return ENTRY[net](q, q, q, L, act, w, b, lw, 0.0, np.ones(q.shape, bool))


def entry_budget(net, act, L, w, b, lw, k0, qi, qj, d_terms, u, diag=None, dii=None, djj=None):
    """(ref[2], bud[2]): NNGP and NTK references of the entries (k0, qi, qj) and their budgets under the rule of the module
    docstring.  diag marks the entries a symmetric build takes from its closed-form diagonal; dii / djj are row_kernel of
    qi / qj where the caller has them per row already (they are computed per entry otherwise)."""
    k0, qi, qj = (np.asarray(v, np.float64) for v in np.broadcast_arrays(k0, qi, qj))
    f = ENTRY[net]
    hyp = (L, act, w, b, lw)
    if dii is None:
        dii = row_kernel(net, act, L, w, b, lw, qi)
    if djj is None:
        djj = row_kernel(net, act, L, w, b, lw, qj)
    push = (d_terms + 2 * L + 4) * u
    with np.errstate(all="ignore"):
        ref = f(k0, qi, qj, *hyp, 0.0, diag)
        pp = f(k0, qi, qj, *hyp, push, diag)
        pm = f(k0, qi, qj, *hyp, -push, diag)
    bud = []
    for m in (0, 1):
        dev = np.maximum(np.abs(pp[m] - ref[m]), np.abs(pm[m] - ref[m]))
        bud.append(dev + (2 * L + 4) * u * (np.abs(ref[m]) + np.sqrt(np.abs(dii[m] * djj[m]))))
    return ref, bud


def fast_erf_allowance(L, w, lw):
    """The extra ABSOLUTE allowance of the f32 NNGP-only MLP erf build (the correlation-space FAST maps, asin_fast):
    |asin_fast - asin| <= 2.6e-7 over [-1, 1] (nngp_math.hpp) whatever the entry's scale.  Each layer injects
    lw^2 (2 / pi) 2.6e-7 and the layers behind it amplify it by at most w^2 Kdot <= 4 w^2 / pi
    (Kdot = 4 / (pi sqrt((1 + 2q)(1 + 2q') - 4 K^2)) <= 4 / pi)."""
    amp = 4 * w * w / PI
    return lw * lw * (2 / PI) * 2.6e-7 * sum(amp ** i for i in range(L))


# ----------------------------------------------------------------------------------------------------------- inputs
def assert_separated(x1, x2=None, gap=1e-3):
    """Every off-diagonal input correlation c0 = <x_i, x_j> / (|x_i| |x_j|) has 1 - |c0| >= gap (no zero rows either)."""
    a = np.asarray(x1, np.float64)
    b = a if x2 is None else np.asarray(x2, np.float64)
    na, nb = np.sqrt((a * a).sum(1)), np.sqrt((b * b).sum(1))
    assert na.min() > 0 and nb.min() > 0, "zero row"
    for r0 in range(0, a.shape[0], 512):
        c = np.abs(a[r0:r0 + 512] @ b.T) / np.outer(na[r0:r0 + 512], nb)
        if x2 is None:
            c[np.arange(c.shape[0]), r0 + np.arange(c.shape[0])] = 0.0
        assert 1.0 - c.max() >= gap, "input rows %d..: max |c0| = %.6f" % (r0, c.max())


def gauss(n, d, t="f32", seed=0):
    """Standard normal rounded to the dtype; d_terms = d.  Only for d <= 64: the Gram term d u is a worst-case bound."""
    assert d <= 64
    x = np.random.default_rng([20261019, n, d, seed]).standard_normal((n, d)).astype(NPT[t])
    assert_separated(x)
    return x


def exact(n, d, t="f32", seed=0):
    """Integers uniform in -3..3: every product and partial sum of the Gram is an integer of magnitude <= 9 d <= 9 * 3072
    < 2^24, exact in f32 and f64 in any summation order (the MFMA's included).  d_terms = 2: the rounded 1 / d and its
    product.  This makes d = 257 and d = 3072 as tight as d = 5."""
    assert 9 * d < 2 ** 24
    x = np.random.default_rng([20261019, n, d, seed, 7]).integers(-3, 4, size=(n, d)).astype(NPT[t])
    assert_separated(x)
    return x


# ----------------------------------------------------------------------------------------------------------- entries
def select_entries(n1, n2, sym, seed=0, per_tile=64):
    """(i, j) of the entries to check.  Up to FULL_LIMIT entries: all of them (symmetric: the lower triangle with the
    diagonal; the caller checks the mirrored position as well).  Larger: per 128 x 128 tile (symmetric: lower tiles) the
    four corners, one entry in each of local rows 63 and 64 (the seam of the 64-row half tiles) and seeded random entries
    up to at least per_tile -- no tile is left out."""
    if n1 * n2 <= FULL_LIMIT:
        if sym:
            return np.tril_indices(n1)
        i, j = np.divmod(np.arange(n1 * n2), n2)
        return i, j
    rng = np.random.default_rng([n1, n2, int(sym), seed])
    ii, jj = [], []
    for tr in range((n1 + TILE - 1) // TILE):
        for tc in range(tr + 1 if sym else (n2 + TILE - 1) // TILE):
            r0, c0 = tr * TILE, tc * TILE
            h, wd = min(TILE, n1 - r0), min(TILE, n2 - c0)
            lr = [0, 0, h - 1, h - 1] + [r for r in (63, 64) if r < h]
            lc = [0, wd - 1, 0, wd - 1] + [int(rng.integers(wd)) for r in (63, 64) if r < h]
            extra = max(per_tile - len(lr), 0)
            lr = np.concatenate([lr, rng.integers(h, size=extra)])
            lc = np.concatenate([lc, rng.integers(wd, size=extra)])
            ii.append(r0 + lr)
            jj.append(c0 + lc)
    return np.concatenate(ii).astype(np.int64), np.concatenate(jj).astype(np.int64)


def tiles_covered(i, j, n1, n2, sym):
    """True when (i, j) holds an entry of every tile (symmetric: every lower tile)."""
    t1, t2 = (n1 + TILE - 1) // TILE, (n2 + TILE - 1) // TILE
    seen = np.zeros((t1, t2), bool)
    seen[i // TILE, j // TILE] = True
    return bool(seen[np.tril_indices(t1)].all() if sym else seen.all())


def gram_entries(x1, x2, i, j):
    """(k0[i, j], q1, q2) = (<x1_i, x2_j> / d, |x1|^2 / d, |x2|^2 / d) in fp64; x2 = None: the symmetric Gram."""
    a = np.asarray(x1, np.float64)
    b = a if x2 is None else np.asarray(x2, np.float64)
    d = a.shape[1]
    if a.shape[0] * b.shape[0] <= FULL_LIMIT:
        g = (a @ b.T)[i, j]
    else:
        g = np.concatenate([np.einsum("ed,ed->e", a[i[s:s + 65536]], b[j[s:s + 65536]]) for s in range(0, len(i), 65536)])
    return g / d, (a * a).sum(1) / d, (b * b).sum(1) / d


def reference(net, act, L, w, b, lw, x1, x2, i, j, d_terms, u, diag=None):
    """entry_budget of the entries (i, j) of the kernel of x1 against x2.  x2 = None: the symmetric build, whose diagonal
    entries are exact; a cross build that has such entries (a row shard of the symmetric kernel) names them in diag."""
    k0, q1, q2 = gram_entries(x1, x2, i, j)
    d1 = row_kernel(net, act, L, w, b, lw, q1)
    d2 = d1 if x2 is None else row_kernel(net, act, L, w, b, lw, q2)
    if diag is None and x2 is None:
        diag = i == j
    return entry_budget(net, act, L, w, b, lw, k0, q1[i], q2[j], d_terms, u, diag=diag,
                        dii=(d1[0][i], d1[1][i]), djj=(d2[0][j], d2[1][j]))
