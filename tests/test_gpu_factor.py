"""GPU tests of smn_cholesky / smn_trsm through the C ABI against the componentwise backward-error rules of
tests/_factor_rules.py: every case asserts rho <= n_factor + 1 (derived, any summation order) and rho <= 8 x the same rule on
LAPACK's result in the same precision on the same matrix, the log-determinant against the stored diagonal, exact info, and
that nothing strictly above the diagonal was written.  (For four large shapes and the shifted cases the reference is not
LAPACK but a NumPy emulation of the library's summation order: _factor_rules.py CHAIN_SHAPES gives the reason and figures.)

One case per route of cholesky.hip (launch_update, launch_panel, cholesky_t; heads.hip smn_cholesky for the padded copy); the
comment beside each names the condition that selects it at that size, for 256 CUs and the default knobs (super-panel
S = 1024, outer panel W = 256, no look-ahead under n_total = 8192).

Tile forms of launch_update by the number nt of 128 x 128 tiles of a launch: nt <= 256 (kQuarterTileMax) 64 x 64 tiles,
nt <= 384 (kHalfTileMax) 64-row tiles, above full tiles, with the XCD map from nt >= 512 unless the shape is a trapezoid.

With SMN_FACTOR_RECORD=<file> in the environment every measured pair (rho_gpu, rho_ref) is appended to that file
(profiles/r14_factor_residuals.txt was written that way)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _factor_rules as R  # noqa: E402

DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


@pytest.fixture(scope="module")
def schedule_ctx(L):
    """Contexts created under environment switches (read once, by smn_ctx_create), one per schedule and module run."""
    made = {}

    def get(name):
        if name not in made:
            env = {s[0]: s[1] for s in R.SCHEDULES}[name]
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                made[name] = L.Context(0)
            finally:
                for k, v in old.items():
                    if v is None:
                        del os.environ[k]
                    else:
                        os.environ[k] = v
        return made[name]

    yield get
    made.clear()


def factor(L, c, a, n_factor, n_shift=0, jitter=0.0, ridge=0.0):
    """smn_cholesky on an upload of `a`; returning at all is SMN_OK (Context.call raises otherwise)."""
    n_total = a.shape[0]
    ad = c.to_device(a)
    info, logdet = C.c_int(-7), C.c_double(-7.0)
    c.call("smn_cholesky", L.dtype_code(a.dtype.type), ad.ptr, n_total, n_factor, n_total, n_shift, jitter, ridge, C.byref(info),
           C.byref(logdet))
    return info.value, logdet.value, ad.numpy()


def record(case, dtype, got, ref, refname="lapack"):
    line = "%-44s %-8s ref=%-6s " % (case, np.dtype(dtype).name, refname) + "  ".join(
        "%s gpu %.3g ref %.3g" % (k, got[k], ref[k]) for k in ("factor", "rows", "schur", "trsm") if k in got)
    print(line)
    path = os.environ.get("SMN_FACTOR_RECORD")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def check(case, a_upload, a_rule, got, info, logdet, n_factor, ref, diag_allow=0.0, refname="lapack"):
    """The assertions every good factorisation gets.  a_upload: what went to the device (its strict upper triangle must come
    back); a_rule: the matrix the factor must reproduce (the same, or the host-shifted one); ref: the reference residuals --
    LAPACK's, or those of the emulated chain where _factor_rules.py names it the reference and says why."""
    assert got.dtype == a_upload.dtype
    rho = R.residuals(a_rule, got, n_factor, diag_allow)
    record(case, got.dtype, rho, ref, refname)
    assert info == 0, case
    for k, v in rho.items():
        assert v <= n_factor + 1, (case, k, v)
        assert v <= R.REF_FACTOR * ref[k], (case, k, v, ref[k])
    lh = got[:n_factor, :n_factor]
    assert abs(logdet - R.logdet_self(lh)[0]) <= R.logdet_bound(lh), (case, logdet, R.logdet_self(lh)[0], R.logdet_bound(lh))
    assert R.upper_intact(a_upload, got), case


# ----------------------------------------------------------------------------- A: one shape per route, default context
ROUTES = [
    # padded copy (smn_cholesky: n_total or n_factor no multiple of 128 -> workspace copy with identity padding), one sub-panel:
    (1, 0),        # 128 x 128 copy, 127 identity columns; cholesky_t: one launch_panel, no update at all
    (16, 0),       # the same; the factor is exactly one 16-column leaf of panelr_kernel
    (17, 3),       # one column into the second leaf; 3 appended rows padded to a tile: panel grid of 1 group, then the far update
                   # (`!sb` branch of cholesky_t) K = 128 on the one Schur tile: nt = 1 <= kQuarterTileMax
    (127, 0),      # one identity column
    (129, 1),      # padded to 256 + 128: second sub-panel -> the strip update (js > j0) K = 128 over 2 tile rows, far update K = 256
    # in place (all of: n_total % 128 == 0, n_factor % 128 == 0, 16-byte aligned):
    (128, 0),      # one launch_panel, nothing else
    (256, 128),    # strip update K = 128 (js = 128 > j0 = 0), tiles_m = 2; j1 == s_end: no near update; far update K = 256
    (384, 0),      # first near update: j1 = 256 < s_end = 384, K = W = 256, a 1 x 1 trapezoid (turned into the triangle)
    (640, 128),    # near updates behind outer panels 0 and 1 (trapezoids of 3 x 5 and 1 x 3 tiles), far update K = 640
    # ragged in both dimensions (padded copy):
    (391, 37),     # 512 + 128
    (1025, 0),     # 1152: ONE column in the second super-panel (s_end = 1024 < n_factor): far update K = 1024, panel of an identity block
    (1300, 77),    # 1408 + 128: far K = 1024, then strip / near / far (K = 384) inside the second super-panel, appended rows throughout
    (2305, 0),     # 2432: three super-panels, far updates of 11 and 3 tile rows
    # far update with K = S = 1024 in one launch (`!sb`: n_total < chain_min_n), in place:
    (1152, 0),
    (1024, 128),   # ... on the Schur tile
    # 35 tile rows, row-sampled.  launch_panel: fp32 below = n_total - 128 = 4352 > kPanelSmallRows -> 128-row workgroups for the
    # first two sub-panels, 16-row ones (kPanelSmallXR) from the third on; fp64: grid = 4352 / 16 = 272 > num_cu -> passes = 2
    # (multi-pass panels).  launch_update: far update behind super-panel 0 is 27 tile rows = 378 tiles -> half tiles
    # (kQuarterTileMax < nt <= kHalfTileMax), every other update <= 256 tiles -> quarter tiles.
    (4480, 0),
    # 40 tile rows, row-sampled: the far update behind super-panel 0 is 32 tile rows = 528 tiles: the smallest n with nt >= 512,
    # i.e. full 128 x 128 tiles in the XCD patch order (u.use_map); behind super-panel 1 24 rows = 300 tiles (half tiles).
    # (Full tiles WITHOUT the map, 384 < nt < 512, are the K = 2048 far update of the trail_kernel case below: 30 rows = 465 tiles.)
    (5120, 0),
]


def test_route_list_is_the_rules_list():
    assert ROUTES == R.SHAPES_A


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m", ROUTES)
def test_factor_routes(L, ctx, dtype, n, m):
    a, _, ref = R.reference(n, m, dtype)
    info, logdet, got = factor(L, ctx, a, n)
    check("A (%d,%d)" % (n, m), a, a, got, info, logdet, n, ref, refname="chain" if (n, m, dtype) in R.CHAIN_SHAPES else "lapack")


# ----------------------------------------------------------------------------- B: schedule switches at small n
# lookahead512 (1664,128): SMN_CHAIN_MIN_N=1 -> sb = stream_bulk, so W = kOuterWide = 512; SMN_SUPER=512 -> S = 512: a super-panel is
#   one outer panel with strips of K = 128, 256, 384 and no near update; behind it F0 (the next 512 columns, trapezoid, K = 512) on
#   the chain and F1 (the rest, triangle) on the CU-masked bulk stream; F1 has <= kF0FirstTiles tiles, so F0 is launched first and
#   F1 waits for it (f0_first); F0 of the next super-panel waits for F1 (ev_b).  The last F1 is the Schur tile alone.
# lookahead512_wide (1664,128): SMN_SUPER_WIDE_ROWS=1024 -> width(0) = kSuperWide = 2048 since n_total - 0 >= 1024: at this size the
#   one wide super-panel swallows all of n_factor -- outer panels of 512 with NEAR updates of K = 512 (trapezoids) under the
#   look-ahead, no F0, F1 = the Schur tile on the bulk stream.
# lookahead_width_change (2432,128): the same switches where the width does change between super-panels: width(0) = 2048, then
#   n_total - 2048 = 512 < 1024 -> width(2048) = 512: F0 is [2048, 2432) with K = 2048, F1 the Schur tile.
# super256 (640,0): S = W = 256: j1 == s_end always, no near update; a far update of K = 256 behind every outer panel.
# trail_kernel (5888,0), fp32: SMN_SUPER=2048, look-ahead off (SMN_CHAIN_CUS=0; n_total < 8192 as well).  The first near update
#   (tag 1, trapezoid so no map, K = 256 <= kPersistMaxK) has tiles_n = 14, tiles_m = 44: nt = 105 + 30 * 14 = 525 > 2 * 256 -> trail_kernel;
#   at n = 5760 nt = 511.  R.trail_kernel_min_n derives it (test_factor_host.py).  Row-sampled.
# panel_leaf0 (1152,128): ctx->panel_leaf false -> launch_panel_x launches panel_kernel (micro-panels in LDS) for every sub-panel.
@pytest.mark.parametrize("name,n,m,dtype", [(s[0], s[2][0], s[2][1], dt) for s in R.SCHEDULES for dt in s[3]])
def test_factor_schedules(L, schedule_ctx, name, n, m, dtype):
    a, _, ref = R.reference(n, m, dtype)
    info, logdet, got = factor(L, schedule_ctx(name), a, n)
    check("B %s (%d,%d)" % (name, n, m), a, a, got, info, logdet, n, ref, refname="chain" if (n, m, dtype) in R.CHAIN_SHAPES else "lapack")


# ----------------------------------------------------------------------------- D: failing pivots, NaN
def _good_then_bad_then_good(L, c, bad, n, m, dtype, want_info, case):
    good = R.reference(n, m, dtype)[0]
    before = factor(L, c, good, n)
    info, logdet, got = factor(L, c, bad, n)               # returned: SMN_OK
    print("%s %s: info %d (want %d) logdet %r" % (case, np.dtype(dtype).name, info, want_info, logdet))
    assert info == want_info, case
    assert math.isnan(logdet), case
    assert R.info_ok(info, logdet, want_info)
    assert R.upper_intact(bad, got), case
    after = factor(L, c, good, n)
    assert before[0] == 0 and after[0] == 0 and before[1] == after[1], case
    assert np.array_equal(before[2], after[2]), case       # the same bits as before the failure


# p (1-based) in (n_factor, m): 1 first pivot; 16 | 17 the last column of a 16-column leaf and the first of the next; 128 | 129 the
# same at a sub-panel edge; 257 the first column of the second outer panel; 391 the last column of a ragged matrix -- all seven
# through the padded copy ((300,0), (391,0)) --; 1025 the first column of the second super-panel, in place, with appended rows
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p,n,m", R.PIVOT_CASES)
def test_failing_pivot(L, ctx, dtype, p, n, m):
    _good_then_bad_then_good(L, ctx, R.pivot_matrix(p, n, m, dtype), n, m, dtype, p, "D pivot %d in (%d,%d)" % (p, n, m))


@pytest.mark.parametrize("dtype", DTYPES)
def test_failing_pivot_under_the_lookahead(L, schedule_ctx, dtype):
    p, n, m = R.PIVOT_LOOKAHEAD                            # first column of the second super-panel: F0 and F1 have run once
    _good_then_bad_then_good(L, schedule_ctx("lookahead512"), R.pivot_matrix(p, n, m, dtype), n, m, dtype, p,
                             "D pivot %d in (%d,%d), look-ahead" % (p, n, m))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("i,j,n,m", R.NAN_CASES)
def test_nan_in_the_lower_triangle(L, ctx, dtype, i, j, n, m):
    """A NaN at (i, j), i > j, reaches row i of the factor and nothing above it: the first pivot that is not a number is i."""
    _good_then_bad_then_good(L, ctx, R.nan_matrix(i, j, n, m, dtype), n, m, dtype, i + 1, "D NaN at (%d,%d) in (%d,%d)" % (i, j, n, m))


# ----------------------------------------------------------------------------- E: shifts
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", sorted(R.SHIFT_KINDS))
@pytest.mark.parametrize("n_shift", R.SHIFT_COUNTS)
@pytest.mark.parametrize("n,m", R.SHIFT_SHAPES)            # padded copy | in place; both with appended rows and > 256 shifted entries
def test_shifts(L, ctx, dtype, kind, n_shift, n, m):
    """The reference matrix is the upload shifted on the host in fp64 and rounded once; the library's own addition may round
    a_ii once more (+1 on the diagonal ratios).  rho_schur is taken against the unshifted C, so a shift that reached the Schur
    diagonal (or the identity padding) fails it; the diagonal from n_shift on is 100 times larger, so a trace over more than
    n_shift entries fails rho_factor.  On these matrices (a diagonal 100 times the off-diagonal part) the reference is the
    emulated chain, not LAPACK: _factor_rules.py, "the library's summation order"."""
    ns = n if n_shift is None else n_shift
    jitter, ridge = R.SHIFT_KINDS[kind]
    a, a_sh, _, ref = R.shift_reference(n, m, ns, kind, dtype)
    info, logdet, got = factor(L, ctx, a, n, ns, jitter, ridge)
    check("E (%d,%d) n_shift %d %s" % (n, m, ns, kind), a, a_sh, got, info, logdet, n, ref, diag_allow=1.0 if ns else 0.0,
          refname="chain")
    if ns == 0:                                            # nothing may change: the bits of the call without any shift
        plain = factor(L, ctx, a, n)
        assert plain[1] == logdet and np.array_equal(plain[2], got)


# ----------------------------------------------------------------------------- F: smn_trsm
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("n,nrhs", R.TRSM_SHAPES)
def test_trsm(L, ctx, dtype, trans, n, nrhs):
    l, b, _, ref = R.trsm_reference(n, nrhs, trans, dtype)
    ld, bd = ctx.to_device(l), ctx.to_device(b)
    ctx.call("smn_trsm", L.dtype_code(dtype), ld.ptr, n, n, bd.ptr, nrhs, nrhs, trans)
    x = bd.numpy()
    rho = R.rho_trsm(l, b, x, trans)
    record("F trsm (%d,%d) trans %d" % (n, nrhs, trans), dtype, {"trsm": rho}, {"trsm": ref})
    assert x.dtype == dtype and rho <= n + 1 and rho <= R.REF_FACTOR * ref, (rho, ref)
    assert np.array_equal(ld.numpy(), l)                   # L is an input
