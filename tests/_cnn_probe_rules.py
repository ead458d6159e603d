"""The forward-mode tangent rules of csrc/cnn_grad.hip for single image pairs, in a NumPy scalar type of the caller's choice (a
helper shared by test_cnn_probe_host.py and test_gpu_cnn_grad_probes.py; not a test module).

tests/_cnn_grad_rules.py (box3, act_d, cnn_tangents) restated as ONE implementation that
  * works in T = np.float32, np.float64 or np.longdouble throughout (libm functions, no device-style approximation), so the
    same text gives the reference (longdouble) and the yardstick (what a careful evaluation in the storage type loses);
  * takes the images x [N, H, W, C] already rounded to the storage type and returns only the pairs (n, m) asked for, a block of
    pairs at a time: the per-pixel maps are [block, H, W], never N^2 of them;
  * takes a pair with n == m from the per-image chain (q, qw, qb), as the device's dexact is;
  * carries the zero-variance guards of _cnn_grad_rules.act_d: where q <= 0 the ReLU map is not differentiable, the pixel
    contributes no variance-side term and its correlation is taken as 0.

Per pair the state is three H x W maps (K, Kw = dK/dw^2, Kb = dK/db^2), per image (q, qw, qb):
    Conv:  Kw <- box(K)/9 + w^2 box(Kw)/9    Kb <- 1 + w^2 box(Kb)/9    K <- w^2 box(K)/9 + b^2      (box: 3x3, zero padded)
    Act:   Kw <- phi_A Kw + phi_qi qw_n + phi_qj qw_m   (Kb likewise);   K <- phi(K, q_n, q_m)
    Flatten + Dense:  lw^2 * mean over the H W pixels
    terms: d/dw_std = 2 w_std d/dw^2,  d/db_std = 2 b_std d/db^2,  d/dlast_w_std = 2 K~ / last_w_std

fault = ... evaluates a deliberately WRONG variant of the rules (FAULTS below): what a slip in cgrad_pair_kernel would compute.
test_cnn_probe_host.py feeds them to the acceptance function of the GPU test, which has to reject every one of them.
"""
import numpy as np

from _grad_probe_rules import U, scales, yardstick  # noqa: F401  (re-exported)

LD = np.longdouble
FACTOR = 16.0
W, B, LW = 1.3, 0.4, 0.9

FAULTS = ("next_layer_table",   # the column image's (q, qw, qb) taken from the next layer (clamped to the last)
          "wrap",               # the pair maps' box sum wraps round instead of zero padding
          "skip_box_kb",        # box(Kb) skipped in layers >= 1
          "mean_slots",         # the mean taken over the 64 NP lane slots instead of the H W pixels
          "carry")              # Kw / Kb start from the previous pair's final maps instead of 0


def box3(a, wrap=False):
    h, w = a.shape[-2:]
    out = np.zeros_like(a)
    if wrap:
        for dh in (-1, 0, 1):
            for dw in (-1, 0, 1):
                out += np.roll(a, (dh, dw), axis=(-2, -1))
        return out
    p = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(1, 1), (1, 1)])
    for dh in range(3):
        for dw in range(3):
            out += p[..., dh:dh + h, dw:dw + w]
    return out


def act_d(k, qi, qj, act, T):
    """(phi, phi_A, phi_qi, phi_qj) per pixel, all in T."""
    pi = T(4) * np.arctan(T(1))
    one, two, zero = T(1), T(2), T(0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if act == "relu":
            sp = np.sqrt(qi * qj)
            c = np.where(sp > 0, k / sp, zero)
            c = np.clip(c, -one, one)
            s1 = np.sqrt(np.maximum((one - c) * (one + c), zero))
            pm = pi - np.arccos(c)
            o = sp * (s1 + pm * c) / (two * pi)
            da = pm / (two * pi) + zero * sp
            d1 = np.where(qi > 0, s1 * sp / (T(4) * pi * qi), zero)    # zero variance: no variance-side term
            d2 = np.where(qj > 0, s1 * sp / (T(4) * pi * qj), zero)
            return o, da, d1, d2
        if act == "erf":
            ti, tj = one + two * qi, one + two * qj
            sp = np.sqrt(ti * tj)
            s = np.clip(two * k / sp, -one, one)
            den = np.sqrt(np.maximum((one - s) * (one + s), T(np.finfo(T).tiny)))
            o = (two / pi) * np.arcsin(s)
            return o, T(4) / (pi * sp * den), -(two / pi) * s / (den * ti), -(two / pi) * s / (den * tj)
    raise KeyError(act)


def image_chain(xs, layers, act, w2, b2, T):
    """The per-image chain of the images xs [I, H, W, C]: per layer the PRE-activation (q, qw, qb), each [I, H, W], and the
    (q, qw, qb) behind the last activation."""
    pi = T(4) * np.arctan(T(1))
    one, two, nine = T(1), T(2), T(9)
    q = np.einsum("nhwc,nhwc->nhw", xs, xs) / T(xs.shape[-1])
    qw, qb = np.zeros_like(q), np.zeros_like(q)
    pre = []
    for _ in range(layers):
        bq = box3(q)
        qw = bq / nine + w2 * box3(qw) / nine
        qb = one + w2 * box3(qb) / nine
        q = w2 * bq / nine + b2
        pre.append((q, qw, qb))
        if act == "relu":
            dq, q = T(0.5), q / two
        else:
            dq = (T(4) / pi) / ((one + two * q) * np.sqrt(one + T(4) * q))
            q = (two / pi) * np.arcsin(two * q / (one + two * q))
        qw, qb = dq * qw, dq * qb
    return pre, (q, qw, qb)


def lane_pixels(hw):
    """Pixels per lane of the form cgrad_launch picks for an image of hw pixels."""
    return 1 if hw <= 64 else 4 if hw <= 256 else 16


def _pair_block(x, layers, act, w2, b2, lw2, n_idx, m_idx, T, fault, init=None):
    """One block of pairs: ([3, P] = lw^2 mean (K, Kw, Kb), the final (Kw, Kb) maps of the off-diagonal pairs)."""
    imgs, inv = np.unique(np.concatenate([n_idx, m_idx]), return_inverse=True)
    xs = np.asarray(x)[imgs].astype(T)
    h, w, c = xs.shape[1:]
    pre, last = image_chain(xs, layers, act, w2, b2, T)
    ni, mi = inv[:len(n_idx)], inv[len(n_idx):]
    out = np.stack([lw2 * a.mean(axis=(1, 2), dtype=T)[ni] for a in last])
    off = np.flatnonzero(n_idx != m_idx)
    if not len(off):
        return out, None
    ni, mi = ni[off], mi[off]
    one, nine = T(1), T(9)
    wrap = fault == "wrap"
    k = np.einsum("phwc,phwc->phw", xs[ni], xs[mi]) / T(c)
    kw, kb = (np.zeros_like(k), np.zeros_like(k)) if init is None else init
    for l in range(layers):
        bk = box3(k, wrap)
        kw = bk / nine + w2 * box3(kw, wrap) / nine
        kb = one + w2 * (kb if fault == "skip_box_kb" and l >= 1 else box3(kb, wrap)) / nine
        k = w2 * bk / nine + b2
        qn, qwn, qbn = (a[ni] for a in pre[l])
        qm, qwm, qbm = (a[mi] for a in pre[min(l + 1, layers - 1) if fault == "next_layer_table" else l])
        o, da, d1, d2 = act_d(k, qn, qm, act, T)
        kw = da * kw + d1 * qwn + d2 * qwm
        kb = da * kb + d1 * qbn + d2 * qbm
        k = o
    if fault == "mean_slots":
        out[:, off] = np.stack([lw2 * (a.sum(axis=(1, 2), dtype=T) / T(64 * lane_pixels(h * w))) for a in (k, kw, kb)])
    else:
        out[:, off] = np.stack([lw2 * a.mean(axis=(1, 2), dtype=T) for a in (k, kw, kb)])
    return out, (kw, kb)


def pair_tangents(x, layers, act, w_std, b_std, last_w_std, n_idx, m_idx, T=np.float64, block=512, fault=None):
    """[3, P] in T: (K, dK/dw^2, dK/db^2) behind Flatten + Dense of the image pairs (n_idx[p], m_idx[p]) of x [N, H, W, C] (already
    rounded to the storage type), `block` pairs at a time."""
    assert fault is None or fault in FAULTS
    n_idx, m_idx = np.asarray(n_idx, np.int64), np.asarray(m_idx, np.int64)
    w2, b2 = T(w_std) * T(w_std), T(b_std) * T(b_std)
    lw2 = T(last_w_std) * T(last_w_std)
    out = np.empty((3, len(n_idx)), T)
    for p0 in range(0, len(n_idx), block):
        sl = slice(p0, min(len(n_idx), p0 + block))
        res, fin = _pair_block(x, layers, act, w2, b2, lw2, n_idx[sl], m_idx[sl], T, fault)
        if fault == "carry" and fin is not None:
            init = tuple(np.roll(a, 1, axis=0) for a in fin)
            for a in init:
                a[0] = 0
            res, _ = _pair_block(x, layers, act, w2, b2, lw2, n_idx[sl], m_idx[sl], T, fault, init)
        out[:, sl] = res
    return out


def pair_terms(x, layers, act, w_std, b_std, last_w_std, n_idx, m_idx, T=np.float64, block=512, fault=None):
    """[3, P] in T: d K~_nm / d(w_std, b_std, last_w_std)."""
    k, kw, kb = pair_tangents(x, layers, act, w_std, b_std, last_w_std, n_idx, m_idx, T, block, fault)
    return np.stack([T(2) * T(w_std) * kw, T(2) * T(b_std) * kb, T(2) / T(last_w_std) * k])


def reference(x, layers, act, b_std, n_idx, m_idx, T, block=512):
    """(ref [3, E] longdouble, s [3, E], Y [3]) of the pairs for images x stored in T: the rules in longdouble on the widened
    images, the scale s_nm = max(|ref_nm|, sqrt(|ref_nn ref_mm|)) per term and the yardstick of evaluating in T."""
    n_idx, m_idx = np.asarray(n_idx, np.int64), np.asarray(m_idx, np.int64)
    assert x.dtype == T
    xl = x.astype(LD)
    ref = pair_terms(xl, layers, act, W, b_std, LW, n_idx, m_idx, LD, block)
    imgs = np.unique(np.concatenate([n_idx, m_idx]))
    ref_d = np.zeros((3, x.shape[0]), LD)
    ref_d[:, imgs] = pair_terms(xl, layers, act, W, b_std, LW, imgs, imgs, LD, block)
    val = pair_terms(x, layers, act, W, b_std, LW, n_idx, m_idx, T, block)
    assert val.dtype == T
    s = scales(ref, ref_d, n_idx, m_idx)
    return ref, s, yardstick(val, ref, s)


def floor(T):
    return 4.0 * U[T]


def check(T, out, g, n_idx, m_idx, ref, s, y, nc=1):
    """The acceptance of one case: out [E, 4] = the four terms of one probe call per pair, g [E] the seed values (in T).  Every
    value finite; terms[3] exactly nc g (rounded once in T) on the diagonal and 0.0 off it; |out / (nc m g) - ref| <= 16 max(Y, 4 u)
    s for every pair and term, m = 2 off the diagonal and 1 on it.  Returns (ratio [3, E] = error / (max(Y, 4u) s), problems: a list
    of strings, empty when the case holds)."""
    n_idx, m_idx = np.asarray(n_idx), np.asarray(m_idx)
    problems = []
    if not np.isfinite(out).all():
        problems.append("not finite")
    dg = n_idx == m_idx
    gc = (g.dtype.type(nc) * g).astype(np.float64)
    if not np.array_equal(out[:, 3], np.where(dg, gc, 0.0)):
        problems.append("terms[3] is not exactly g [n == m]")
    m = np.where(dg, 1.0, 2.0)
    dev = out[:, :3].T.astype(LD) / (LD(nc) * m * g.astype(LD))
    err = np.abs(dev - ref)
    yy = np.maximum(y, floor(T))[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(s > 0, err / (yy * s), np.where(err == 0, 0.0, np.inf)).astype(np.float64)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    for t, e in zip(*np.nonzero(~(ratio <= FACTOR))):
        problems.append("term %d pair (%d, %d): ratio %.3g > %g" % (t, n_idx[e], m_idx[e], ratio[t, e], FACTOR))
    return ratio, problems


def seed_values(T, count, seed=0):
    """Seed values of either sign in [1/2, 3/2), exact in T."""
    rng = np.random.default_rng([count, seed])
    return ((0.5 + rng.random(count)) * np.where(rng.random(count) < 0.5, -1.0, 1.0)).astype(T)


# ------------------------------------------------------------------------------------------------------------- cases
# (h, w, c, layers) per form of cgrad_launch: pixels per lane 1 / 4 / 16, ragged or exact last lane.  Every form sees the depths
# 1, 2, 4 (at one layer the l > 0 shortcut skips the box sums of Kw and Kb) and the channel counts 1, 2, 3.
FORM_SHAPES = {
    (1, "ragged"): [(1, 1, 3, 4), (5, 7, 2, 1), (6, 6, 1, 2)],                      # 1x1: one live lane
    (1, "exact"): [(8, 8, 1, 4), (1, 64, 2, 2), (64, 1, 3, 1)],
    (4, "ragged"): [(9, 8, 2, 1), (12, 12, 1, 4), (3, 50, 3, 2)],                  # 3x50: the row stride does not divide 64
    (4, "exact"): [(16, 16, 1, 2), (4, 64, 2, 4), (16, 16, 3, 1)],
    (16, "ragged"): [(17, 16, 2, 1), (20, 20, 3, 2), (31, 33, 1, 4), (1, 1024, 1, 2)],   # 1x1024: the largest padded map
    (16, "exact"): [(32, 32, 3, 4), (16, 64, 1, 1), (1024, 1, 2, 2)],              # W = 1 is an exact form
}
SHAPES = [s for v in FORM_SHAPES.values() for s in v]
B0_SHAPES = [(6, 6, 1, 2), (8, 8, 1, 2), (12, 12, 1, 2), (20, 20, 1, 2), (32, 32, 1, 2)]   # b_std == 0 on the zero-border set
ACTS = ("relu", "erf")


def form_of(h, w):
    npl = lane_pixels(h * w)
    return npl, "exact" if h * w == 64 * npl and 64 % w == 0 else "ragged"


def shape_id(s):
    return "%dx%dx%d-L%d" % s


_CACHE = {}


def five_images(h, w, c, T):
    """[5, h, w, c] in T (generated in fp64, rounded once): 0-2 random, 3 a copy of 1 (an exact duplicate off the diagonal), 4 zero
    outside a central block (rows h//4 .. h - h//4, columns likewise: a border of h//4 and w//4 pixels)."""
    key = ("five", h, w, c, T)
    if key not in _CACHE:
        x = np.random.default_rng([20261020, h, w, c]).standard_normal((5, h, w, c))
        x[3] = x[1]
        keep = np.zeros((h, w, 1), bool)
        keep[h // 4:h - h // 4, w // 4:w - w // 4] = True
        x[4] = np.where(keep, x[4], 0.0)
        x = x.astype(T)
        x.setflags(write=False)
        _CACHE[key] = x
    return _CACHE[key]


def many_images(n, h, w, c, T):
    key = ("many", n, h, w, c, T)
    if key not in _CACHE:
        x = np.random.default_rng([20261020, n, h, w, c]).standard_normal((n, h, w, c)).astype(T)
        x.setflags(write=False)
        _CACHE[key] = x
    return _CACHE[key]


ALL15 = np.tril_indices(5)


def tri_pair(pr):
    """Pair number pr of the lower triangle, row by row: pr = n (n + 1) / 2 + m."""
    n = int((np.sqrt(8.0 * pr + 1.0) - 1.0) / 2.0)
    while (n + 1) * (n + 2) // 2 <= pr:
        n += 1
    while n * (n + 1) // 2 > pr:
        n -= 1
    return n, pr - n * (n + 1) // 2


WALK_N = 160                       # 12 880 pairs: more than the 4 x 2048 waves of the largest plain grid
WALK_STEP = 4 * 2048               # wave number v walks the pairs v, v + WALK_STEP


def walk_pairs():
    """48 pairs of n = 160: the corners, the first and the second pair of six waves (one of them the last wave that has a second
    pair), two runs of eight consecutive pair numbers (the waves of two neighbouring workgroups, the second run in the waves'
    second round) and diagonal entries."""
    n = WALK_N
    npairs = n * (n + 1) // 2
    prs = [0, n * (n - 1) // 2, npairs - 1, 1]                                    # (0,0), (n-1,0), (n-1,n-1), (1,0)
    for v in (2, 3, 77, 1000, 4095, npairs - 1 - WALK_STEP - 5):
        prs += [v, v + WALK_STEP]
    prs += list(range(4001, 4009)) + list(range(WALK_STEP + 4001, WALK_STEP + 4009))
    out = [tri_pair(p) for p in prs]
    out += [(d, d) for d in (2, 63, 64, 65, 100, 127, 128, 158)]
    for e in [(159, 158), (100, 37), (64, 63), (128, 0), (33, 32), (90, 89), (159, 80), (5, 3)]:
        out.append(e)
    seen, uniq = set(), []
    for e in out:
        if e not in seen:
            seen.add(e)
            uniq.append(e)
    assert len(uniq) == 48, len(uniq)
    a = np.array(uniq, np.int64)
    return a[:, 0], a[:, 1]


TILED_N = 1531


def tiled_pairs():
    """32 pairs of n = 1531 (the tiled pair order: tiles of tile_bn x 32 pairs, ragged last tiles, half-empty diagonal tiles)."""
    n = TILED_N
    e = [(0, 0), (n - 1, 0), (n - 1, n - 1), (1, 0), (31, 31), (32, 31), (32, 32), (33, 0), (63, 32), (64, 63),
         (1530, 1529), (1530, 1504), (1530, 1503), (1504, 1504), (1519, 1000), (1520, 1000), (1527, 31), (1528, 32),
         (1000, 999), (1000, 1000), (1001, 992), (1001, 991), (765, 3), (766, 383), (255, 254), (256, 255), (256, 0),
         (511, 96), (512, 95), (1279, 1279), (1280, 640), (1407, 1406)]
    assert len(set(e)) == 32
    a = np.array(e, np.int64)
    return a[:, 0], a[:, 1]


DENSE_N = 160
DENSE_SHAPES = [(6, 6, 1, 2), (12, 12, 1, 2)]
COEF = 0.7


def dense_seed(n, T, c=1):
    """(neg_kinv [n, n] symmetric, alpha [n, c]) stored in T."""
    key = ("seed", n, T, c)
    if key not in _CACHE:
        rng = np.random.default_rng([20261020, n, 1])
        g = rng.standard_normal((n, n))
        g = ((g + g.T) / 2.0).astype(T)
        a = rng.standard_normal((n, c)).astype(T)
        for v in (g, a):
            v.setflags(write=False)
        _CACHE[key] = g, a
    return _CACHE[key]


def dense_reference(h, w, c, layers, act, n, T):
    """(expected [4], bound [3], Y [3]) of the dense-seed call on many_images with G = COEF alpha alpha^T + neg_kinv: expected[0..2]
    = sum over the lower triangle of m G ref, expected[3] = tr G, bound = sum m |G| s, all in longdouble from the stored values."""
    key = ("dense", h, w, c, layers, act, n, T)
    if key not in _CACHE:
        x = many_images(n, h, w, c, T)
        nk, al = dense_seed(n, T)
        i, j = np.tril_indices(n)
        ref, s, y = reference(x, layers, act, B, i, j, T, block=1024)
        g = LD(COEF) * al.astype(LD)[i, 0] * al.astype(LD)[j, 0] + nk.astype(LD)[i, j]
        m = np.where(i == j, LD(1), LD(2))
        expected = np.concatenate([(m * g * ref).sum(axis=1), [g[i == j].sum()]])
        _CACHE[key] = expected, (m * np.abs(g) * s).sum(axis=1), y
    return _CACHE[key]
