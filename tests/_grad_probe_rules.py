"""The forward-mode tangent rules of csrc/grad.hip for single entries, in a NumPy scalar type of the caller's choice (a helper
shared by test_grad_probe_host.py and test_gpu_grad_probes.py; not a test module).

tests/_multi_rules.dense_tangents (NNGP: K, K_w, K_b) and tests/_ntk_rules.tangents (Theta: six states) restated as ONE
implementation that
  * works in T = np.float32, np.float64 or np.longdouble throughout (libm functions, no device-style approximation), so the
    same text gives the reference (longdouble) and the yardstick (what a careful evaluation in the storage type loses);
  * takes the stored (k0 [n,n], q [n]) the device entries take, not x, and returns only the entries (i, j) asked for;
  * carries the zero-variance guards of tests/_cnn_grad_rules.act_d: where a row's variance is 0 the ReLU map is not
    differentiable and the row contributes no variance-side term (and its correlation is defined as 0, as the oracle does);
  * covers MLP and dense ResNet, relu and erf.

Per entry the state is (K, K_w, K_b, Theta, Theta_w, Theta_b) (subscripts d/dw^2, d/db^2) and per side the row's own chain
(q, q_w, q_b); entries with i == j are taken from the row chain behind every activation, as the device's exact diagonal is:
    Dense:       A = w2 K + b2, A_w = K + w2 K_w, A_b = 1 + w2 K_b;  T = A + w2 Theta, T_w = A_w + Theta + w2 Theta_w,
                 T_b = A_b + w2 Theta_b
    activation:  K <- phi(A), K_t = D A_t + phi_1 q_i,t + phi_2 q_j,t, D = phi_A;  D_t = D_A A_t + D_1 q_i,t + D_2 q_j,t;
                 Theta <- T D, Theta_t = T_t D + T D_t
    output:      K~ = lw2 K (NNGP) or lw2 (K + Theta) (NTK);  d/dw_std = 2 w_std d/dw2, d/db_std = 2 b_std d/db2,
                 d/dlast_w_std = 2 K~ / last_w_std
"""
import numpy as np

U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}


def _act(act, T, a, qi, qj, diag, ntk, push=None):
    """phi, D = phi_A, phi_1, phi_2 and (ntk) D_A, D_1, D_2 at pre-activation a with variances qi, qj, all in T.
    push = (mask, delta): ReLU entries whose correlation is taken as 1 - delta (duplicate_allowance)."""
    pi = T(4) * np.arctan(T(1))
    one, two, zero = T(1), T(2), T(0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if act == "relu":
            sp = np.sqrt(qi * qj)
            c = np.where(sp > 0, a / sp, zero)
            c = np.where(diag & (sp > 0), one, c)
            c = np.clip(c, -one, one)
            if push is not None:
                c = np.where(push[0], one - T(push[1]), c)
            s1 = np.sqrt(np.maximum((one - c) * (one + c), zero))
            pm = pi - np.arccos(c)
            phi = sp * (s1 + pm * c) / (two * pi)
            d = pm / (two * pi)
            p1 = np.where(qi > 0, s1 * sp / (T(4) * pi * qi), zero)
            p2 = np.where(qj > 0, s1 * sp / (T(4) * pi * qj), zero)
            if not ntk:
                return phi, d, p1, p2, None, None, None
            inv = np.where(s1 > 0, one / (two * pi * s1), zero)      # flat where (1-c)(1+c) <= 0: D = 1/2 identically
            da = np.where(sp > 0, inv / sp, zero)
            d1 = np.where(qi > 0, -inv * c / (two * qi), zero)
            d2 = np.where(qj > 0, -inv * c / (two * qj), zero)
            return phi, d, p1, p2, da, d1, d2
        if act == "erf":
            ti, tj = one + two * qi, one + two * qj
            p = ti * tj
            sp = np.sqrt(p)
            s = np.clip(two * a / sp, -one, one)
            om = np.maximum((one - s) * (one + s), T(np.finfo(T).tiny))
            den = np.sqrt(om)
            phi = two / pi * np.arcsin(s)
            d = T(4) / (pi * sp * den)
            p1 = -(two / pi) * s / (den * ti)
            p2 = -(two / pi) * s / (den * tj)
            if not ntk:
                return phi, d, p1, p2, None, None, None
            r15 = (p * om) * (sp * den)                               # R^(3/2), R = (1+2q_i)(1+2q_j) - 4 A^2 = p (1-s^2)
            return phi, d, p1, p2, T(16) * a / (pi * r15), -T(4) * tj / (pi * r15), -T(4) * ti / (pi * r15)
    raise KeyError(act)


def _row_act(act, T, q, qw, qb):
    """The row's own chain through an activation: phi(q, q, q) and its total derivative in q, closed forms."""
    if act == "relu":
        return q / T(2), qw / T(2), qb / T(2)          # zero variance: q = 0 stays 0, slope 1/2
    pi = T(4) * np.arctan(T(1))
    dq = (T(4) / pi) / ((T(1) + T(2) * q) * np.sqrt(T(1) + T(4) * q))
    return (T(2) / pi) * np.arcsin(T(2) * q / (T(1) + T(2) * q)), dq * qw, dq * qb


def entry_states(net, act, layers, w_std, b_std, k0, q, i, j, T=np.float64, ntk=False, push=None):
    """(K, K_w, K_b, Theta, Theta_w, Theta_b) behind the last activation (before the last Dense) at the entries (i, j) of the
    kernel over the stored Gram k0 [n,n] and its diagonal q [n]; Theta* are None unless ntk.
    push = (mask, delta, kt): the perturbed run of duplicate_allowance (ReLU, ntk)."""
    i, j = np.asarray(i), np.asarray(j)
    diag = i == j
    q = np.asarray(q).astype(T)
    w2, b2 = T(w_std) * T(w_std), T(b_std) * T(b_std)
    one = T(1)
    k = np.where(diag, q[i], np.asarray(k0)[i, j].astype(T))
    z = np.zeros(k.shape, T)
    ent = [k, z, z, z, z, z]
    ri, rj = [q[i], z, z], [q[j], z, z]

    def dense(ent, ri, rj):
        k, kw, kb, th, tw, tb = ent
        a, aw, ab = w2 * k + b2, k + w2 * kw, one + w2 * kb
        out = [a, aw, ab, None, None, None]
        if ntk:
            out[3:] = a + w2 * th, aw + th + w2 * tw, ab + w2 * tb
        return out, *([w2 * r[0] + b2, r[0] + w2 * r[1], one + w2 * r[2]] for r in (ri, rj))

    def activ(ent, ri, rj):
        a, aw, ab, t, tw, tb = ent
        phi, d, p1, p2, da, d1, d2 = _act(act, T, a, ri[0], rj[0], diag, ntk, None if push is None else push[:2])
        kw = d * aw + p1 * ri[1] + p2 * rj[1]
        kb = d * ab + p1 * ri[2] + p2 * rj[2]
        ro, co = _row_act(act, T, *ri), _row_act(act, T, *rj)
        out = [np.where(diag, ro[0], phi), np.where(diag, ro[1], kw), np.where(diag, ro[2], kb), None, None, None]
        if ntk:
            dw = da * aw + d1 * ri[1] + d2 * rj[1]
            db = da * ab + d1 * ri[2] + d2 * rj[2]
            if push is not None:                                     # the rounding of the cancelling sum behind D_t
                dw = dw + np.where(push[0], T(push[2]) * ri[1] / ri[0], T(0))
                db = db + np.where(push[0], T(push[2]) * ri[2] / ri[0], T(0))
            out[3:] = t * d, tw * d + t * dw, tb * d + t * db
        return out, list(ro), list(co)

    def add(x, y):
        return [None if u is None else u + v for u, v in zip(x, y)]

    if net == "mlp":
        for _ in range(layers):
            ent, ri, rj = dense(ent, ri, rj)
            ent, ri, rj = activ(ent, ri, rj)
    elif net == "resnet":
        ent, ri, rj = dense(ent, ri, rj)
        for _ in range(layers):
            blk = dense(*activ(ent, ri, rj))
            ent, ri, rj = add(ent, blk[0]), add(ri, blk[1]), add(rj, blk[2])
        ent, ri, rj = activ(ent, ri, rj)
    else:
        raise KeyError(net)
    return ent


def entry_tangents(net, act, layers, w_std, b_std, last_w_std, k0, q, i, j, T=np.float64, get="nngp", push=None):
    """[3, len(i)] in T: d K~_ij / d(w_std, b_std, last_w_std) with K~ the NNGP kernel (get="nngp") or Theta (get="ntk")."""
    ntk = {"nngp": False, "ntk": True}[get]
    k, kw, kb, th, tw, tb = entry_states(net, act, layers, w_std, b_std, k0, q, i, j, T, ntk, push)
    if ntk:
        k, kw, kb = k + th, kw + tw, kb + tb
    lw = T(last_w_std)
    lw2 = lw * lw
    return np.stack([lw2 * kw * (T(2) * T(w_std)), lw2 * kb * (T(2) * T(b_std)), T(2) * lw * k])


def duplicate_mask(k0, q, i, j, b_std):
    """Entries off the diagonal whose two rows are exact duplicates as stored, k0_ij == q_i == q_j, with a variance behind the
    first Dense (all-zero rows are duplicates of each other under b_std > 0 and dead under b_std == 0)."""
    i, j = np.asarray(i), np.asarray(j)
    k0, q = np.asarray(k0), np.asarray(q)
    return (i != j) & (k0[i, j] == q[i]) & (q[i] == q[j]) & ((q[i] > 0) | (b_std != 0))


def duplicate_allowance(net, act, layers, w_std, b_std, last_w_std, k0, q, i, j, T, get):
    """The extra ABSOLUTE allowance [3, len(i)] of the ReLU tangent of Theta between exactly duplicate rows off the diagonal; 0
    everywhere else (and for erf, and for the NNGP form, whose first-order terms cancel).

    There c = 1 identically, D = phi_A = 1/2 and D_t = 0 whatever the hyper-parameters, and the rules (like the device's own
    diagonal) take that exactly.  The device tile forms c~ = A ra_i ra_j from the rounded tables and its own rounded chain, which
    is 1 only to rounding (csrc/act_tangent.hpp: "1e-16 in c is 1e-8 in D"; README, the NTK paragraph): c~ = 1 - delta with
    0 <= delta <= dmax = (2 L + 5) u, the count tests/_kernel_budget.py moves every correlation by (d_terms = 1 for a stored
    K0).  Then
        D~   = 1/2 - sqrt(2 delta) / (2 pi) (1 + O(delta)),   phi, phi_1, phi_2 follow the same c~ (their first orders cancel)
        D~_t = sqrt(delta / 2) / (2 pi) q_t / q                the exact value of the generic formula at c~, plus the rounding of
               its cancelling sum  rs1 / (2 pi) [uu A_t - c~ (ra_i^2 q_i,t + ra_j^2 q_j,t) / 2]:  the three terms are q_t / q up to
               dmax relative each, and rs1 = 1 / sqrt(2 delta) <= 1 / sqrt(2 u) (delta >= u or the entry is flat),
               so at most  kt q_t / q,  kt = dmax / (sqrt(2 u) 2 pi).
    The allowance is the larger deviation from the reference of the rules run with c = 1 - dmax at every activation of those
    entries and D_t moved by +kt q_t / q or -kt q_t / q: the approximation's own error carried through the remaining layers,
    as _kernel_budget's pushed runs carry theirs.  It is of the order sqrt(u) s_ij."""
    i, j = np.asarray(i), np.asarray(j)
    out = np.zeros((3, len(i)), np.longdouble)
    mask = duplicate_mask(k0, q, i, j, b_std)
    if act != "relu" or get != "ntk" or not mask.any():
        return out
    nsets = layers if net == "mlp" else layers + 1
    dmax = (2 * nsets + 5) * U[T]
    kt = dmax / (np.sqrt(2.0 * U[T]) * 2.0 * np.pi)
    L = np.longdouble
    ref = entry_tangents(net, act, layers, w_std, b_std, last_w_std, k0, q, i[mask], j[mask], L, get)
    for sign in (1.0, -1.0):
        run = entry_tangents(net, act, layers, w_std, b_std, last_w_std, k0, q, i[mask], j[mask], L, get,
                             push=(np.ones(int(mask.sum()), bool), dmax, sign * kt))
        out[:, mask] = np.maximum(out[:, mask], np.abs(run - ref))
    return out


def scales(ref, ref_diag, i, j):
    """s_ij = max(|ref_ij|, sqrt(|ref_ii ref_jj|)) per term: ref [3, len(i)] at the entries, ref_diag [3, n] on the diagonal."""
    return np.maximum(np.abs(ref), np.sqrt(np.abs(ref_diag[:, i] * ref_diag[:, j])))


def yardstick(val_t, ref, s):
    """Y per term: the largest |rules_T - ref| / s over the entries (0 where the scale is 0: nothing to lose there)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(s > 0, np.abs(val_t.astype(np.longdouble) - ref) / s, np.where(val_t.astype(np.longdouble) == ref, 0.0, np.inf))
    return np.asarray(r.max(axis=1), np.float64)


# ------------------------------------------------------------------------------------------------------------- cases
# What test_gpu_grad_probes.py probes and test_grad_probe_host.py checks the yardstick of: inputs are generated in fp64, the
# Gram and its diagonal rounded ONCE to the storage type (k0_ii = q_i exactly), so the contraction is the only device arithmetic.
NETS = (("mlp", "relu", 3), ("mlp", "erf", 6), ("resnet", "relu", 2), ("resnet", "erf", 1))   # test_gpu_kernel_budget.NETS
NET_IDS = ["%s-%s%d" % n for n in NETS]
W, B, LW = 1.4, 0.3, 0.8
D = 7
GT = 64                              # tile edge of the contraction
ZERO_ROWS = (0, 31, 64)
DUP_N = 200
DUP_PAIRS = np.concatenate([[63, 127, 191], 5 + 6 * np.arange(29)])   # rows p of the 32 pairs (p, p + 1); three straddle a tile edge
DUP_GAPS = {np.float32: (1e-2, 1e-4), np.float64: (1e-2, 1e-4, 1e-6)}


def _round_gram(x, T):
    k0 = x @ x.T / x.shape[1]
    q = np.einsum("ij,ij->i", x, x) / x.shape[1]
    np.fill_diagonal(k0, q)
    k0, q = k0.astype(T), q.astype(T)
    assert np.array_equal(np.diag(k0), q)
    for a in (k0, q):
        a.setflags(write=False)
    return k0, q


_CACHE = {}


def inputs(kind, n, T, gap=None):
    """(k0 [n,n], q [n]) in the storage type T.  kind: "sep" Gaussian rows, no two closer than 1 - |c0| = 1e-3; "zero": the same
    with the rows ZERO_ROWS all zero; "dup": the rows p + 1 of DUP_PAIRS at correlation 1 - gap with row p (same length)."""
    key = (kind, n, T, gap)
    if key in _CACHE:
        return _CACHE[key]
    x = np.random.default_rng([20261020, n]).standard_normal((n, D))
    if kind == "zero":
        x[list(ZERO_ROWS)] = 0.0
    elif kind == "dup":
        c = 1.0 - gap
        for p in DUP_PAIRS:
            v = x[p + 1] - (x[p + 1] @ x[p]) / (x[p] @ x[p]) * x[p]
            x[p + 1] = c * x[p] + np.sqrt((1.0 - c) * (1.0 + c)) * np.linalg.norm(x[p]) * v / np.linalg.norm(v)
    else:
        assert kind == "sep"
    if kind != "dup":
        live = x[np.abs(x).sum(1) > 0]
        nr = np.linalg.norm(live, axis=1)
        cc = np.abs(live @ live.T) / np.outer(nr, nr)
        np.fill_diagonal(cc, 0.0)
        assert 1.0 - cc.max() >= 1e-3
    _CACHE[key] = _round_gram(x, T)
    return _CACHE[key]


def all_lower(n):
    return np.tril_indices(n)


def geometry_entries(n, seed=0, per_tile=16):
    """The fixed selection behind one tile row: per 64 x 64 tile of the lower triangle its corners, local rows 31 / 32 (the
    boundary of the NTK form's two passes), 16 seeded entries; the diagonal, the last row and column."""
    rng = np.random.default_rng([n, seed])
    ii, jj = [np.arange(n), np.full(n, n - 1)], [np.arange(n), np.arange(n)]
    nt = (n + GT - 1) // GT
    for tr in range(nt):
        for tc in range(tr + 1):
            r0, c0 = tr * GT, tc * GT
            h, wd = min(GT, n - r0), min(GT, n - c0)
            lr = [0, 0, h - 1, h - 1] + [r for r in (31, 32) if r < h]
            lc = [0, wd - 1, 0, wd - 1] + [int(rng.integers(wd)) for r in (31, 32) if r < h]
            lr = np.concatenate([lr, rng.integers(h, size=per_tile)]) + r0
            lc = np.concatenate([lc, rng.integers(wd, size=per_tile)]) + c0
            ii.append(np.maximum(lr, lc))        # a diagonal tile: mirrored into the lower triangle
            jj.append(np.minimum(lr, lc))
    e = np.unique(np.stack([np.concatenate(ii), np.concatenate(jj)]).astype(np.int64), axis=1)
    return e[0], e[1]


def zero_row_entries(n):
    """Every lower entry in a row or a column of ZERO_ROWS, and the geometry selection beside them."""
    i, j = np.tril_indices(n)
    hit = np.isin(i, ZERO_ROWS) | np.isin(j, ZERO_ROWS)
    gi, gj = geometry_entries(n)
    e = np.unique(np.stack([np.concatenate([i[hit], gi]), np.concatenate([j[hit], gj])]), axis=1)
    return e[0], e[1]


def probe_sets():
    """[(id, kind, n, gap, b_std, (i, j), nets)]: every entrywise case of the GPU file (dtype and get are its parameters)."""
    mlp_relu = NETS[:1]
    out = [("all65", "sep", 65, None, B, all_lower(65), NETS)]
    out += [("all%d" % n, "sep", n, None, B, all_lower(n), mlp_relu) for n in (1, 63, 64)]
    out.append(("geometry200", "sep", 200, None, B, geometry_entries(200), NETS))
    out.append(("zero65", "zero", 65, None, B, zero_row_entries(65), NETS))
    out.append(("zero65-b0", "zero", 65, None, 0.0, zero_row_entries(65), NETS))
    return out


def reference(net, act, layers, b_std, k0, q, i, j, T, get):
    """(ref [3, E] longdouble, s [3, E], Y [3], extra [3, E]) of the entries (i, j) for inputs stored in T: the rules in longdouble
    on the widened inputs, the scale s_ij = max(|ref_ij|, sqrt(|ref_ii ref_jj|)), the yardstick of evaluating in T and
    duplicate_allowance."""
    n = len(q)
    dg = np.arange(n)
    ref = entry_tangents(net, act, layers, W, b_std, LW, k0, q, i, j, np.longdouble, get)
    ref_d = entry_tangents(net, act, layers, W, b_std, LW, k0, q, dg, dg, np.longdouble, get)
    val = entry_tangents(net, act, layers, W, b_std, LW, k0, q, i, j, T, get)
    s = scales(ref, ref_d, np.asarray(i), np.asarray(j))
    return ref, s, yardstick(val, ref, s), duplicate_allowance(net, act, layers, W, b_std, LW, k0, q, i, j, T, get)


# ------------------------------------------------------------------------------------------------- dense seeds
DENSE_N = (200, 1300)                # several tile rows; 210 tiles (the second-stage reduction's strided loop)
COEF = 0.7


def dense_seed(n, T):
    """(neg_kinv [n,n] symmetric, alpha [n]) stored in T: a random symmetric matrix seed and a random vector seed."""
    key = ("seed", n, T)
    if key not in _CACHE:
        rng = np.random.default_rng([20261020, n, 1])
        g = rng.standard_normal((n, n))
        g = ((g + g.T) / 2.0).astype(T)
        a = rng.standard_normal(n).astype(T)
        for v in (g, a):
            v.setflags(write=False)
        _CACHE[key] = g, a
    return _CACHE[key]


def dense_reference(net, act, layers, b_std, n, T, get, kind="sep", keep=None):
    """(expected [4], bound [3], Y [3]) of the dense-seed call on inputs(kind, n, T) with G = COEF alpha alpha^T + neg_kinv:
    expected[0..2] = sum_ij G_ij ref_ij over all i, j (the lower triangle with m = 2 off the diagonal), expected[3] = tr G,
    bound = sum_ij m_ij |G_ij| s_ij, all in longdouble from the stored values.  keep: the rows (= columns) that take part."""
    k0, q = inputs(kind, n, T)
    nk, al = dense_seed(n, T)
    if keep is not None:
        k0, q, nk, al = k0[np.ix_(keep, keep)], q[keep], nk[np.ix_(keep, keep)], al[keep]
    i, j = np.tril_indices(len(q))
    ref, s, y, _ = reference(net, act, layers, b_std, k0, q, i, j, T, get)
    L = np.longdouble
    g = L(COEF) * al.astype(L)[i] * al.astype(L)[j] + nk.astype(L)[i, j]
    m = np.where(i == j, L(1), L(2))
    expected = np.concatenate([(m * g * ref).sum(axis=1), [g[i == j].sum()]])
    return expected, (m * np.abs(g) * s).sum(axis=1), y
