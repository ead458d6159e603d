"""Host tests of tests/_factor_rules.py (no GPU): every rule stays within its derived bound on LAPACK's own results for every
case test_gpu_factor.py runs, every rule flags the damage it is there for, and the preconditions of the GPU cases hold
(LAPACK's info for the failing pivots and the NaNs, the row sample, the size at which trail_kernel is first taken)."""
import math

import numpy as np
import pytest

import _factor_rules as R

DTYPES = [np.float32, np.float64]
SAMPLED = [s for s in R.SHAPES_A if sum(s) > R.SAMPLE_ABOVE]


# ----------------------------------------------------------------------------- the rules on LAPACK
SCHEDULE_SHAPES = sorted({(s[2], dt) for s in R.SCHEDULES for dt in s[3] if s[2] not in R.SHAPES_A}, key=str)


@pytest.mark.parametrize("n,m,dtype", [(n, m, dt) for n, m in R.SHAPES_A for dt in DTYPES] + [(n, m, dt) for (n, m), dt in SCHEDULE_SHAPES])
def test_lapack_is_within_the_derived_bound(dtype, n, m):
    a, f, rho = R.reference(n, m, dtype)
    assert set(rho) == ({"factor", "rows", "schur"} if m else {"factor"})
    assert R.within(rho, n), rho
    assert R.logdet_ok(R.logdet_self(f[:n, :n])[0], f[:n, :n])
    assert R.upper_intact(a, f)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", sorted(R.SHIFT_KINDS))
@pytest.mark.parametrize("n_shift", R.SHIFT_COUNTS)
@pytest.mark.parametrize("n,m", R.SHIFT_SHAPES)
def test_lapack_is_within_the_derived_bound_on_the_shifted_cases(dtype, kind, n_shift, n, m):
    ns = n if n_shift is None else n_shift
    a, a_sh, f, rho = R.shift_reference(n, m, ns, kind, dtype)
    assert R.within(rho, n), rho
    idx = np.arange(n + m)
    assert np.array_equal(a_sh[idx[ns:], idx[ns:]], a[idx[ns:], idx[ns:]])          # nothing beyond n_shift moved
    assert ns == 0 or np.all(a_sh[idx[:ns], idx[:ns]] > a[idx[:ns], idx[:ns]])
    i, j = np.tril_indices(n + m, -1)
    assert np.array_equal(a_sh[i, j], a[i, j])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("n,nrhs", R.TRSM_SHAPES)
def test_lapack_trsm_is_within_the_derived_bound(dtype, trans, n, nrhs):
    l, b, x, rho = R.trsm_reference(n, nrhs, trans, dtype)
    assert rho <= n + 1
    # the other op(L) is not a solution
    assert R.rho_trsm(l, b, x, 1 - trans) > R.REF_FACTOR * max(rho, 1.0) or n == 1


def test_zero_denominators():
    z = np.zeros((2, 2))
    assert R._ratio_max(z, z) == 0.0
    assert R._ratio_max(np.array([[0.0, 1e-300]]), np.zeros((1, 2))) == math.inf
    assert R._ratio_max(np.array([[np.nan]]), np.ones((1, 1))) == math.inf
    # a zero appended row against anything: rho 0, not NaN
    a = np.eye(3, dtype=np.float32); a[2, :2] = 0.0
    f, info = R.lapack_factor(a, 2)
    assert info == 0 and R.residuals(a, f, 2) == {"factor": 0.0, "rows": 0.0, "schur": 0.0}


# ----------------------------------------------------------------------------- sampling
@pytest.mark.parametrize("n_total", [1, 2500, 2501, 2560, 4480, 4481, 5888, 8192, 6144 + 128])
def test_row_sample_hits_every_group_of_16(n_total):
    rows = R.sample_rows(n_total)
    assert rows.size >= n_total / 16 and rows.max() < n_total and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.unique(rows // 16), np.arange((n_total + 15) // 16))    # no 16-row group is left out
    if n_total <= R.SAMPLE_ABOVE:
        assert rows.size == n_total
    else:
        full = rows[: n_total // 16]
        assert np.array_equal(full % 16, (full // 16) % 16)                          # the offset rotates with the group
        assert set(full[:16 * 8] % 128) >= set(range(0, 128, 17))                    # and so walks through a tile's block rows


@pytest.mark.parametrize("n,m", SAMPLED)
def test_sampled_rho_is_the_full_rho_of_the_sampled_rows(n, m):
    a, f, rho = R.reference(n, m, np.float32)
    l = np.tril(f[:n, :n]).astype(np.float64)
    rows = R.sample_rows(n + m)[::37]
    worst = 0.0
    for r in rows[rows < n]:
        num = np.abs(a[r, :r + 1].astype(np.float64) - l[r] @ l[:r + 1].T)
        worst = max(worst, float((num / (2.0 ** -24 * (np.abs(l[r]) @ np.abs(l[:r + 1]).T))).max()))
    assert 0.0 < worst <= rho["factor"]


# ----------------------------------------------------------------------------- damage
def _damage_sites(f, n, m):
    """(i, j, k) of the dropped product: the last evaluated row of the factor, a column in the middle, the largest product."""
    rows = R.sample_rows(n + m)
    i = int(rows[rows < n][-1])
    j = i // 2
    return i, j, int(np.argmax(np.abs(f[i, :j].astype(np.float64) * f[j, :j])))


@pytest.mark.parametrize("n,m,dtype", [(n, m, dt) for n, m in R.SHAPES_A if n >= 16 for dt in DTYPES] + [(n, m, dt) for (n, m), dt in SCHEDULE_SHAPES])
def test_one_dropped_product_is_flagged(dtype, n, m):
    a, f, rho = R.reference(n, m, dtype)                                              # (LAPACK's rho, or the chain's where that is the reference)
    i, j, k = _damage_sites(f, n, m)
    bad = R.residuals(a, R.drop_product(f, i, j, k), n)
    assert bad["factor"] > R.REF_FACTOR * rho["factor"], (bad, rho)
    assert not R.within(bad, n, rho)
    if dtype == np.float64:
        assert not R.within(bad, n)                                                  # fp64: far outside the derived bound too
    if m:
        # the same in an appended row (W = B L^-T) and, through it, in the Schur block
        r = n + int((R.sample_rows(n + m)[R.sample_rows(n + m) >= n] - n)[-1])
        g = np.array(f); g[r, j] = g[r, j] + g[r, k] * g[j, k] / g[j, j]
        bad = R.residuals(a, g, n)
        assert bad["rows"] > R.REF_FACTOR * rho["rows"] and bad["schur"] > R.REF_FACTOR * rho["schur"], (bad, rho)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m", [(391, 37), (1152, 0), (1024, 128), (4480, 0)])
def test_a_block_row_without_its_last_k_step_is_flagged(dtype, n, m):
    a, f, rho = R.reference(n, m, dtype)
    r0 = (n // 16 - 1) * 16                                                          # the last whole 16-row block row
    bad = R.residuals(a, R.drop_last_kstep(f, r0, 128), n)
    assert bad["factor"] > R.REF_FACTOR * rho["factor"], (bad, rho)
    if m >= 16:
        bad = R.residuals(a, R.drop_last_kstep(f, n + (m // 16 - 1) * 16, 128), n)
        assert bad["rows"] > R.REF_FACTOR * rho["rows"], (bad, rho)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,p", [(129, 1), (391, 3), (1152, 0), (1152, 8), (4480, 17)])
def test_a_lost_sub_panel_share_of_logdet_is_flagged(dtype, n, p):
    _, f, _ = R.reference(n, 0, dtype)
    lh = f[:n, :n]
    assert not R.logdet_ok(R.logdet_without_subpanel(lh, p), lh)
    # ... as is a logdet accumulated in fp32, or one ulp-of-fp32 off
    good = R.logdet_self(lh)[0]
    assert R.logdet_ok(good, lh) and not R.logdet_ok(float(np.float32(good)) + 1e-6 * abs(good), lh)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", sorted(R.SHIFT_KINDS))
@pytest.mark.parametrize("n,m", R.SHIFT_SHAPES)
def test_a_misplaced_shift_is_flagged(dtype, kind, n, m):
    jitter, ridge = R.SHIFT_KINDS[kind]
    for ns in (1, 127, 300):
        a, a_sh, f, rho = R.shift_reference(n, m, ns, kind, dtype)
        # shifted over all n_factor entries (count, trace and division), as a kernel that ignored n_shift would
        f_bad, info = R.lapack_factor(R.shifted(a, n, jitter, ridge), n)
        bad = R.residuals(a_sh, f_bad, n, diag_allow=1.0)
        assert info == 0 and not R.within(bad, n, rho), (ns, bad)
        if ridge:
            # the right entries, but the trace taken (and divided) over all n_factor entries
            f_bad, info = R.lapack_factor(R.shifted(a, ns, jitter, ridge, trace_over=n), n)
            bad = R.residuals(a_sh, f_bad, n, diag_allow=1.0)
            assert info == 0 and not R.within(bad, n, rho), (ns, bad)
        # the shift also reached the diagonal of the Schur block (or, the same thing in the padded copy, the identity padding
        # behind n_factor): rho_schur is taken against the unshifted C
        f_bad, info = R.lapack_factor(R.shifted(a, ns, jitter, ridge, also=np.arange(n, n + m)), n)
        bad = R.residuals(a_sh, f_bad, n, diag_allow=1.0)
        assert info == 0 and bad["schur"] > R.REF_FACTOR * rho["schur"] and bad["schur"] > n + 1, (ns, bad)
        # and the allowance on the diagonal forgives one rounding of a_ii, not a shift
        assert R.within(R.residuals(a_sh, f, n, diag_allow=1.0), n, rho)


def test_n_shift_zero_changes_nothing():
    a = R.shift_matrix(391, 37, 0, np.float32)
    assert np.array_equal(R.shifted(a, 0, 0.5, 0.25), a)


def test_info_off_by_one_is_flagged():
    assert R.info_ok(129, math.nan, 129)
    assert not R.info_ok(128, math.nan, 129) and not R.info_ok(130, math.nan, 129) and not R.info_ok(0, math.nan, 129)
    assert not R.info_ok(129, 0.0, 129)


# ----------------------------------------------------------------------------- the emulated chain
@pytest.mark.parametrize("n,m,dtype", sorted(R.CHAIN_SHAPES, key=str))
def test_chain_emulation_is_within_the_derived_bound_and_above_lapack(n, m, dtype):
    a, f, rho = R.reference(n, m, dtype)
    rows = R.chain_rows(n + m)
    assert rows.size >= R.CHAIN_ROWS and rows[-1] == R.sample_rows(n + m)[-1] and set(rows) <= set(R.sample_rows(n + m))
    assert R.within(rho, n), rho
    assert rho["factor"] > R.residuals(a, f, n, rows=rows)["factor"]                 # the same rows of LAPACK's factor: the order costs
    g = R.emulate_chain(a, f, n, rows)
    others = np.setdiff1d(np.arange(n + m), rows)
    assert np.array_equal(g[others], f[others]) and R.upper_intact(a, g)            # only the emulated rows were recomputed
    # ... and to fp32 accuracy it is the same factor
    assert np.abs(np.tril(g).astype(np.float64) - np.tril(f)).max() <= 1e-3 * np.abs(np.tril(f)).max()


def test_chain_emulation_is_the_plain_loop():
    """On a small matrix: every row emulated = the textbook jik Cholesky with the chain c <- fl(c - l_ik l_jk)."""
    a = R.matrix(37, 5, np.float32)
    f, _ = R.lapack_factor(a, 37)
    g = R.emulate_chain(a, f, 37, np.arange(42))
    want = np.array(a)
    for i in range(42):
        for j in range(min(i, 36) + 1):
            c = a[i, j]
            for k in range(j):
                c = np.float32(c - np.float32(want[i, k] * want[j, k]))
            want[i, j] = np.sqrt(c) if i == j else np.float32(c / want[j, j])
        for j in range(37, i + 1):
            c = a[i, j]
            for k in range(37):
                c = np.float32(c - np.float32(want[i, k] * want[j, k]))
            want[i, j] = c
    assert np.array_equal(np.tril(g), np.tril(want)) and R.upper_intact(a, g)
    assert R.within(R.residuals(a, g, 37), 37)


# ----------------------------------------------------------------------------- preconditions of the GPU cases
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p,n,m", R.PIVOT_CASES + [R.PIVOT_LOOKAHEAD])
def test_failing_pivot_cases_fail_where_they_should(dtype, p, n, m):
    a = R.pivot_matrix(p, n, m, dtype)
    assert R.lapack_factor(a, n)[1] == p
    if p > 1:                                                                        # and the minor before it is fine
        f, info = R.lapack_factor(np.ascontiguousarray(a[:p - 1, :p - 1]), p - 1)
        assert info == 0 and R.within(R.residuals(a[:p - 1, :p - 1], f, p - 1), p - 1)
    # far from rounding: the pivot is half the largest diagonal entry of the SPD matrix below zero, or lower
    a64 = a.astype(np.float64)
    a64 = np.tril(a64) + np.tril(a64, -1).T
    piv = a64[p - 1, p - 1] - (a64[p - 1, :p - 1] @ np.linalg.solve(a64[:p - 1, :p - 1], a64[:p - 1, p - 1]) if p > 1 else 0.0)
    assert piv <= -0.499 * np.delete(a64.diagonal(), p - 1).max()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("i,j,n,m", R.NAN_CASES)
def test_nan_cases_fail_at_the_row_of_the_nan(dtype, i, j, n, m):
    assert j < i < n
    a = R.nan_matrix(i, j, n, m, dtype)
    assert R.lapack_first_bad_pivot(a, n) == i + 1
    assert R.lapack_first_bad_pivot(a[:i, :i].copy(), i) == 0                     # every pivot before it is a number


def test_nan_placements():
    (i0, j0, _, _), (i1, j1, _, _) = R.NAN_CASES
    assert i0 // 128 == j0 // 128                                                    # inside one sub-panel
    assert j1 < 1024 <= i1                                                           # across the default super-panel edge


def test_trail_kernel_threshold():
    n = R.trail_kernel_min_n()
    assert n == 5888 and n > R.SAMPLE_ABOVE and ("trail_kernel", (n, 0)) in [(s[0], s[2]) for s in R.SCHEDULES]
    tn, tm = (2048 - 256) // 128, (n - 256) // 128
    assert tn * (tn + 1) // 2 + (tm - tn) * tn > 512 >= tn * (tn + 1) // 2 + (tm - 1 - tn) * tn
