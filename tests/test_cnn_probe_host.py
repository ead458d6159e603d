"""Host checks of tests/_cnn_probe_rules.py, the reference, yardstick and acceptance of test_gpu_cnn_grad_probes.py (no GPU).

1. In float64 the rules are the existing ones (_cnn_grad_rules.cnn_tangents) within 4 u of s per pair.
2. In longdouble they are the ENTRYWISE central differences of oracle.nngp_oracle.cnn_kernel in w_std, b_std and last_w_std: the
   diagonal, the duplicate pair and the zero-border image included.
3. The yardstick Y = max |rules_T - rules_longdouble| / s exists for every case the GPU file runs and is printed per case.
4. The acceptance function the GPU test applies (_cnn_probe_rules.check) REJECTS the output of deliberately damaged rules -- the
   slips a pair kernel can make without moving a dense fp64 contraction by 1e-9 -- and accepts the undamaged rules evaluated in the
   storage type: the allowance 16 max(Y, 4u) s is tight enough to see each of them.
"""
import numpy as np
import pytest

import _cnn_grad_rules as R
import _cnn_probe_rules as P
from oracle import nngp_oracle as O

LD = np.longdouble
DTYPES = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]
HOST_SHAPES = [(1, 1, 3, 4), (5, 7, 2, 1), (6, 6, 1, 2), (8, 8, 1, 4), (12, 12, 1, 4), (3, 50, 3, 2), (20, 20, 3, 2)]


def test_longdouble_is_wider_than_double():
    assert np.finfo(LD).eps <= 2.0 ** -63


def test_the_case_grid_reaches_every_form_with_every_depth_and_channel_count():
    assert set(P.FORM_SHAPES) == {(n, r) for n in (1, 4, 16) for r in ("ragged", "exact")}
    for form, shapes in P.FORM_SHAPES.items():
        assert all(P.form_of(h, w) == form for h, w, _, _ in shapes), form
        assert {c for _, _, c, _ in shapes} >= {1, 2, 3} and {l for _, _, _, l in shapes} >= {1, 2, 4}, form
    for want in [(1, 1), (5, 7), (6, 6), (8, 8), (1, 64), (64, 1), (9, 8), (12, 12), (3, 50), (16, 16), (4, 64), (17, 16), (20, 20),
                 (31, 33), (1, 1024), (32, 32), (16, 64), (1024, 1)]:
        assert any((h, w) == want for h, w, _, _ in P.SHAPES), want
    i, j = P.walk_pairs()
    assert len(i) == 48 and (j <= i).all() and i.max() == P.WALK_N - 1
    pr = i * (i + 1) // 2 + j
    assert sum(int(p + P.WALK_STEP) in set(pr.tolist()) for p in pr) >= 12      # a wave's first and second pair, both probed
    i, j = P.tiled_pairs()
    assert len(i) == 32 and (j <= i).all() and i.max() == P.TILED_N - 1


@pytest.mark.parametrize("act", P.ACTS)
@pytest.mark.parametrize("h,w,c,layers", HOST_SHAPES, ids=[P.shape_id(s) for s in HOST_SHAPES])
def test_float64_rules_are_the_existing_rules(h, w, c, layers, act):
    x = P.five_images(h, w, c, np.float64)
    i, j = np.divmod(np.arange(25), 5)
    old = np.stack(R.cnn_tangents(x, layers, act, P.W, P.B, P.LW))                     # (K, Kw, Kb) [3, 5, 5]
    new = P.pair_tangents(x, layers, act, P.W, P.B, P.LW, np.maximum(i, j), np.minimum(i, j), np.float64, block=7)
    d = np.arange(5)
    s = P.scales(old[:, i, j], old[:, d, d], i, j)
    r = np.abs(new - old[:, i, j]) / s
    print("max |new - old| / s = %.2f u" % (r.max() / P.U[np.float64]))
    assert new.dtype == np.float64 and r.max() <= 4 * P.U[np.float64]


@pytest.mark.parametrize("act", P.ACTS)
@pytest.mark.parametrize("h,w,c,layers", HOST_SHAPES, ids=[P.shape_id(s) for s in HOST_SHAPES])
def test_longdouble_rules_are_the_entrywise_central_differences_of_the_oracle_kernel(h, w, c, layers, act):
    """All 25 entries of the five images (the diagonal, the duplicate pair (3, 1), the zero-border image 4), relative step 1e-5
    and 2e-6 as every finite-difference comparison here, per entry against max(s_nm, |fd_nm|)."""
    x = P.five_images(h, w, c, np.float64)
    hyp = dict(w_std=P.W, b_std=P.B, last_w_std=P.LW)
    fd = []
    for key in ("w_std", "b_std", "last_w_std"):
        step = 1e-5 * abs(hyp[key])
        up, dn = dict(hyp, **{key: hyp[key] + step}), dict(hyp, **{key: hyp[key] - step})
        fd.append((O.cnn_kernel(x, None, layers, act, **up) - O.cnn_kernel(x, None, layers, act, **dn)) / (2.0 * step))
    fd = np.stack(fd)
    i, j = np.divmod(np.arange(25), 5)
    got = P.pair_terms(x.astype(LD), layers, act, P.W, P.B, P.LW, np.maximum(i, j), np.minimum(i, j), LD)
    d = np.arange(5)
    s = P.scales(fd[:, i, j], fd[:, d, d], i, j)
    err = np.abs(got - fd[:, i, j]) / np.maximum(s, np.abs(fd[:, i, j]))
    print("max err %.3g" % err.max())
    assert got.dtype == LD and np.isfinite(got.astype(np.float64)).all() and err.max() < 2e-6


@pytest.mark.parametrize("act", P.ACTS)
def test_zero_variance_pixels_under_zero_bias(act):
    """b_std == 0 on the zero-border set: finite in every type, d/db_std = 0, and the other two terms alive."""
    for h, w, c, layers in P.B0_SHAPES:
        for T in (np.float32, np.float64, LD):
            x = P.five_images(h, w, c, np.float64).astype(T)
            t = P.pair_terms(x, layers, act, P.W, 0.0, P.LW, *P.ALL15, T)
            assert t.dtype == T and np.isfinite(t.astype(np.float64)).all() and not t[1].any() and t[0].all() and t[2].all()


@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("act", P.ACTS)
def test_yardstick_of_every_probe_case(act, T):
    """Y / u per case and term (w_std, b_std, last_w_std) for the 15 pairs of the five images: finite, and of the order of a few
    u -- the duplicate pair and the zero-border image included."""
    u = P.U[T]
    for h, w, c, layers in P.SHAPES:
        ref, s, y = P.reference(P.five_images(h, w, c, T), layers, act, P.B, *P.ALL15, T)
        print("%-16s %-4s %s  Y/u = %s" % (P.shape_id((h, w, c, layers)), act, np.dtype(T).name, np.round(y / u, 1)))
        assert np.isfinite(ref.astype(np.float64)).all() and (s > 0).all() and np.isfinite(y).all() and y.max() < 64 * u
    for h, w, c, layers in P.B0_SHAPES:
        ref, s, y = P.reference(P.five_images(h, w, c, T), layers, act, 0.0, *P.ALL15, T)
        print("%-16s %-4s %s  Y/u = %s  (b_std == 0)" % (P.shape_id((h, w, c, layers)), act, np.dtype(T).name, np.round(y / u, 1)))
        assert np.isfinite(y).all() and y.max() < 64 * u and not ref[1].any() and not s[1].any()


def _synth(T, terms, g, i, j, m_off=2.0, m_diag=1.0):
    """What a device whose per-pair tangents are `terms` [3, E] would return: m g dK~ (rounded to T, as gm * s[k] is) and g [n == m]."""
    m = np.where(i == j, m_diag, m_off)
    out = np.empty((len(i), 4))
    out[:, :3] = (LD(1) * m * g.astype(LD) * terms.astype(LD)).T.astype(T)
    out[:, 3] = np.where(i == j, g, 0).astype(np.float64)
    return out


DAMAGE_SHAPES = [(6, 6, 1, 2), (12, 12, 1, 4), (17, 16, 2, 2)]       # ragged forms of 1, 4 and 16 pixels per lane, >= 2 layers


@pytest.mark.parametrize("T", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("act", P.ACTS)
@pytest.mark.parametrize("h,w,c,layers", DAMAGE_SHAPES, ids=[P.shape_id(s) for s in DAMAGE_SHAPES])
def test_the_acceptance_rejects_damaged_rules(h, w, c, layers, act, T):
    x = P.five_images(h, w, c, T)
    i, j = P.ALL15
    ref, s, y = P.reference(x, layers, act, P.B, i, j, T)
    g = P.seed_values(T, len(i))
    # the undamaged rules, evaluated in the storage type, pass: by the definition of Y with a ratio <= 1 (+ the rounding of m g dK)
    ratio, problems = P.check(T, _synth(T, P.pair_terms(x, layers, act, P.W, P.B, P.LW, i, j, T), g, i, j), g, i, j, ref, s, y)
    assert not problems and ratio.max() <= 1.5, (problems, ratio.max())
    xl = x.astype(LD)
    good = P.pair_terms(xl, layers, act, P.W, P.B, P.LW, i, j, LD)
    damaged = {"m = 1 off the diagonal": _synth(T, good, g, i, j, m_off=1.0),
               "m = 2 on the diagonal": _synth(T, good, g, i, j, m_diag=2.0)}
    with np.errstate(all="ignore"):         # a damaged erf chain may leave [-1, 1] for good: inf or NaN, rejected as such
        for fault in P.FAULTS:
            damaged[fault] = _synth(T, P.pair_terms(xl, layers, act, P.W, P.B, P.LW, i, j, LD, fault=fault), g, i, j)
    for name, out in damaged.items():
        ratio, problems = P.check(T, out, g, i, j, ref, s, y)
        hit = np.unique(np.nonzero(~(ratio <= P.FACTOR))[1])
        print("%-24s rejected at %2d of 15 pairs, largest ratio %.3g" % (name, len(hit), ratio.max()))
        assert problems and len(hit) >= 1, name
        # nothing but the diagonal (m = 2 there) or nothing on it (every other damage lives in the pair maps)
        assert (i[hit] == j[hit]).all() if name == "m = 2 on the diagonal" else (i[hit] != j[hit]).all(), (name, hit)
    # and a terms[3] that is off by one rounding is rejected too
    out = _synth(T, good, g, i, j)
    out[0, 3] = np.nextafter(T(out[0, 3]), T(4))
    assert P.check(T, out, g, i, j, ref, s, y)[1]
