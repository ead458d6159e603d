"""The conv-NNGP pair kernels past one pass per wave, at their map-size limits and on variance-zero pixels.

smn_kernel_cnn (csrc/cnn.hip) and smn_kernel_conv_resnet (csrc/cnn_resnet.hip) give one wave one image pair and cap the launch
at _conv_pairs.GRID_WAVES waves: beyond that a wave walks several pairs and carries its LDS maps, zero rings, dummy slots,
factor-table offsets and register stencil from pair to pair.  Every multi-pass build here is held to

  1. the fp64 oracle (oracle/nngp_oracle.py) on the input rounded to the test dtype, `relerr` < RTOL: the whole matrix while
     the oracle's state n1 n2 H W stays within _conv_pairs.ORACLE_FULL_STATE, else a sampled block that holds a pair of every
     pass, and the diagonal of the sampled rows against the symmetric oracle call;
  2. the same matrix assembled from cross calls of at most GRID_WAVES pairs each (one pair per wave): BIT-IDENTICAL off the
     diagonal -- a pair's arithmetic does not depend on the wave or the pass that computes it.  (The diagonal of the
     symmetric build is diag[n] of the per-image pass: oracle only.);
  3. exact symmetry of the FILL_FULL result;
  4. on a few cases, FILL_LOWER into a NaN-prefilled buffer with ldk > n: the strict upper triangle and the padding stay NaN,
     the lower triangle has the FILL_FULL bits.

Image i is scaled by 1 + i / n, so a misplaced or swapped pair moves an entry far beyond the tolerance.  No tolerance is
introduced here: RTOL is the parity tests'."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _conv_pairs as P  # noqa: E402
from _tol import relerr  # noqa: E402
from oracle import nngp_oracle as O  # noqa: E402

RTOL = {np.float32: 2e-3, np.float64: 1e-8}      # tests/test_gpu_parity.py
DTYPES = [np.float64, np.float32]
DT = {"f32": np.float32, "f64": np.float64}
ORACLE = {"smn_kernel_cnn": O.cnn_kernel, "smn_kernel_conv_resnet": O.conv_resnet_kernel}


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


# ----------------------------------------------------------------------------- plumbing
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def oracle(entry, x1, x2, depth, act, hyp=P.HYP):
    x2 = None if x2 is None else np.asarray(x2, np.float64)
    return ORACLE[entry](np.asarray(x1, np.float64), x2, depth, act, *hyp)


class Images:
    """n images on the device; rows(r0, r1) is the pointer of images r0 .. r1 - 1."""

    def __init__(self, ctx, x):
        self.x, self.dev = x, ctx.to_device(x)
        self.n, self.shape = x.shape[0], x.shape[1:]
        self.image_bytes = int(np.prod(self.shape)) * x.dtype.itemsize

    def rows(self, r0=0):
        return C.c_void_p(self.dev.ptr.value + r0 * self.image_bytes)


def build(L, ctx, entry, act, depth, a, r0=0, r1=None, b=None, fill=None, ldk=None, hyp=P.HYP):
    """K(a[r0:r1], b) (b None: symmetric) into a NaN-prefilled [rows, ldk] buffer, returned whole."""
    r1 = a.n if r1 is None else r1
    n1, n2 = r1 - r0, (r1 - r0) if b is None else b.n
    ldk = n2 if ldk is None else ldk
    dtype = a.x.dtype
    out = ctx.to_device(np.full((n1, ldk), np.nan, dtype))
    H, W, Ch = a.shape
    ctx.call(entry, L.dtype_code(dtype), L.ACT[act], depth, *hyp, a.rows(r0), n1, b.rows() if b is not None else None,
             0 if b is None else n2, H, W, Ch, L.FILL_FULL if fill is None else fill, out.ptr, ldk)
    return out.raw_numpy()


def assert_oracle(what, got, ref, dtype):
    dtype = np.dtype(dtype).type
    err = relerr(got, ref)
    print("%s %s: relerr %.3g (RTOL %g)" % (what, np.dtype(dtype).name, err, RTOL[dtype]))
    assert err < RTOL[dtype], (what, err)
    return err


def check_multi_pass(L, ctx, entry, shape, depth, act, dtype, n, min_passes=3, lower=False):
    """Checks 1-4 of the module docstring on the symmetric build of n scaled images."""
    what = "%s %s depth %d %s n=%d" % (entry, shape, depth, act, n)
    assert P.passes(P.npairs(n)) >= min_passes, "the premise: a wave walks several pairs"
    x = P.scaled_images((n,) + shape, dtype, seed=n + sum(shape))
    img = Images(ctx, x)
    k = build(L, ctx, entry, act, depth, img)
    assert k.shape == (n, n) and np.isfinite(k).all(), what
    # 3. symmetry
    assert np.array_equal(k, k.T), what
    # 1. oracle
    rows, cols = P.sample_rows_cols(n)
    assert P.sampled_passes(rows, cols, True) == set(range(P.passes(P.npairs(n))))
    if n * n * shape[0] * shape[1] <= P.ORACLE_FULL_STATE:
        assert_oracle(what + " full", k, oracle(entry, x, None, depth, act), dtype)
    else:
        assert_oracle(what + " sampled", k[np.ix_(rows, cols)], oracle(entry, x[rows], x[cols], depth, act), dtype)
        assert_oracle(what + " sampled diagonal", k[rows, rows], np.diag(oracle(entry, x[rows], None, depth, act)), dtype)
    # 2. the single-pass assembly
    single = np.empty_like(k)
    for r0, r1 in P.row_chunks(n, n):
        assert (r1 - r0) * n <= P.GRID_WAVES
        single[r0:r1] = build(L, ctx, entry, act, depth, img, r0, r1, b=img)
    off = ~np.eye(n, dtype=bool)
    bad = np.argwhere((bits(k) != bits(single)) & off)
    assert bad.size == 0, "%s: %d off-diagonal entries differ from the single-pass cross calls, first at %s (pass %d): %r vs %r" % (
        what, len(bad), tuple(bad[0]), P.pass_of(int(bad[0][0]), int(bad[0][1]), True), k[tuple(bad[0])], single[tuple(bad[0])])
    # 4. FILL_LOWER, ldk > n
    if lower:
        ldk = P.aligned_ld(n, dtype)
        kl = build(L, ctx, entry, act, depth, img, fill=L.FILL_LOWER, ldk=ldk)
        assert kl.shape == (n, ldk) and ldk > n
        assert np.isnan(kl[:, n:]).all(), what + ": padding columns written"
        assert np.isnan(kl[:, :n][np.triu_indices(n, 1)]).all(), what + ": strict upper triangle written under FILL_LOWER"
        low = np.tril_indices(n)
        assert np.array_equal(bits(kl[:, :n][low]), bits(k[low])), what + ": FILL_LOWER differs from FILL_FULL"


# ----------------------------------------------------------------------------- A. smn_kernel_conv_resnet past one pass
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ["relu", "erf"])
@pytest.mark.parametrize("shape,block", P.RESNET_SYM)
def test_resnet_symmetric_multi_pass(L, ctx, dtype, act, shape, block):
    """n = 222: 24,753 pairs, 4 passes of resnet_pair_kernel's grid-stride loop.  (16, 8, 2): 128 pixels, the fp32 load batch of
    8 x 64 pixels is ragged (clamped pixels)."""
    check_multi_pass(L, ctx, "smn_kernel_conv_resnet", shape, block, act, dtype, P.N_SYM,
                     lower=(shape == (8, 8, 1) and act == "relu"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_resnet_cross_multi_pass(L, ctx, dtype):
    """150 x 111 = 16,650 pairs, 3 passes; n2 = 111 shares no factor with the 8192-wave stride (the pr / n2, pr % n2 decode)."""
    shape, block, n1, n2 = P.RESNET_CROSS
    entry, what = "smn_kernel_conv_resnet", "smn_kernel_conv_resnet cross %dx%d" % (n1, n2)
    assert P.passes(P.npairs(n1, False, n2)) >= 3 and np.gcd(n2, P.GRID_WAVES) == 1
    x1 = P.scaled_images((n1,) + shape, dtype, 1)
    x2 = P.scaled_images((n2,) + shape, dtype, 2)[::-1].copy()
    a, b = Images(ctx, x1), Images(ctx, x2)
    k = build(L, ctx, entry, "relu", block, a, b=b)
    assert k.shape == (n1, n2) and np.isfinite(k).all()
    assert n1 * n2 * shape[0] * shape[1] <= P.ORACLE_FULL_STATE
    assert_oracle(what, k, oracle(entry, x1, x2, block, "relu"), dtype)
    single = np.empty_like(k)
    for r0, r1 in P.row_chunks(n1, n2):
        single[r0:r1] = build(L, ctx, entry, "relu", block, a, r0, r1, b=b)
    bad = np.argwhere(bits(k) != bits(single))
    assert bad.size == 0, "%s: %d entries differ from the single-pass calls, first at %s" % (what, len(bad), tuple(bad[0]) if len(bad) else None)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,min_passes", P.RESNET_32)
def test_resnet_32x32x3_multi_pass(L, ctx, dtype, n, min_passes):
    """The workload's own image shape, maps shrinking 32 -> 16 -> 8 -> 4 inside the loop.  n = 130 (8,515 pairs) is the smallest
    build with a second pass; n = 181 (16,471 pairs) has three."""
    check_multi_pass(L, ctx, "smn_kernel_conv_resnet", (32, 32, 3), 1, "relu", dtype, n, min_passes=min_passes)


# ----------------------------------------------------------------------------- B. smn_kernel_cnn: every form past one pass
def _case_id(shape, dt, form):
    return "%dx%dx%d-%s-%s" % (shape + (dt, "".join(ch if ch.isalnum() else "_" for ch in form).strip("_")))


CNN_CASES = [pytest.param(shape, DT[dt], layers, id=_case_id(shape, dt, form))
             for shape, dts, layers, form in P.CNN_FORMS for dt in dts]


@pytest.mark.parametrize("act", ["relu", "erf"])
@pytest.mark.parametrize("shape,dtype,layers", CNN_CASES)
def test_cnn_forms_multi_pass(L, ctx, act, shape, dtype, layers):
    """n = 222, plain pair order (24,753 pairs is below the tiled order's threshold for every form): 4 passes of PairWalk::next
    in every form of launch_pairs; the id names the kernel the case reaches (checked in tests/test_conv_pairs_host.py)."""
    check_multi_pass(L, ctx, "smn_kernel_cnn", shape, layers, act, dtype, P.N_SYM,
                     lower=(act == "relu" and shape in ((8, 8, 2), (32, 32, 3))))


# ----------------------------------------------------------------------------- C. conv-ResNet depth, shapes and limits
def _small_pair(shape, dtype, seed, n2=3):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape).astype(dtype), rng.standard_normal((n2,) + shape[1:]).astype(dtype)


def _sym_and_cross(L, ctx, entry, depth, act, x, x2, what, hyp=P.HYP):
    """Symmetric and cross builds against the oracle; returns the symmetric matrix."""
    dtype = x.dtype
    a, b = Images(ctx, x), Images(ctx, x2)
    k = build(L, ctx, entry, act, depth, a, hyp=hyp)
    assert_oracle(what + " symmetric", k, oracle(entry, x, None, depth, act, hyp), dtype)
    assert np.array_equal(k, k.T)
    kc = build(L, ctx, entry, act, depth, a, b=b, hyp=hyp)
    assert_oracle(what + " cross", kc, oracle(entry, x, x2, depth, act, hyp), dtype)
    return k, kc


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ["relu", "erf"])
@pytest.mark.parametrize("block", [4, 5, 6])
def test_resnet_deep_blocks(L, ctx, dtype, act, block):
    """block_size up to the documented maximum of 6 (kMaxOps); entries grow to 1e2 .. 1e3, relerr is relative."""
    x, x2 = _small_pair((4, 8, 8, 2), dtype, block)
    _sym_and_cross(L, ctx, "smn_kernel_conv_resnet", block, act, x, x2, "resnet block %d %s" % (block, act))


def _conv_diag(L, ctx, x, block, act, hyp=P.HYP):
    xd = ctx.to_device(x)
    d = ctx.to_device(np.full(x.shape[0], np.nan, x.dtype))
    ctx.call("smn_kernel_conv_diag", L.dtype_code(x.dtype), 1, L.ACT[act], block, *hyp, xd.ptr, *x.shape, d.ptr)
    return d.raw_numpy()


# widths whose float reciprocal is inexact (40, 48, 56, 328 and their halves) and the largest maps the on-chip limit of
# resnet_t accepts (12 (H + 2)(W + 2) sizeof(T) <= 160 KiB of dynamic LDS)
LIMIT_SHAPES = [((3, 40, 40, 1), np.float32, 84672), ((3, 56, 56, 1), np.float32, 161472), ((3, 48, 32, 2), np.float64, 163200),
                ((3, 32, 48, 2), np.float64, 163200), ((3, 8, 328, 1), np.float32, 158400)]


@pytest.mark.parametrize("act", ["relu", "erf"])
@pytest.mark.parametrize("shape,dtype,lds", LIMIT_SHAPES)
def test_resnet_inexact_widths_and_largest_maps(L, ctx, act, shape, dtype, lds):
    assert 12 * (shape[1] + 2) * (shape[2] + 2) * np.dtype(dtype).itemsize == lds <= 160 * 1024
    x, x2 = _small_pair(shape, dtype, shape[2])
    k, _ = _sym_and_cross(L, ctx, "smn_kernel_conv_resnet", 1, act, x, x2, "resnet %s %s" % (shape, act))
    # smn_kernel_conv_diag(kind = 1): the oracle's diagonal, and the symmetric build's bit for bit
    d = _conv_diag(L, ctx, x, 1, act)
    ref = np.array([oracle("smn_kernel_conv_resnet", x[i:i + 1], None, 1, act)[0, 0] for i in range(shape[0])])
    assert_oracle("conv_diag %s %s" % (shape, act), d, ref, dtype)
    assert np.array_equal(bits(d), bits(np.diag(k).copy()))


def _small_call_still_right(L, ctx, dtype):
    x, x2 = _small_pair((3, 8, 8, 2), dtype, 5)
    _sym_and_cross(L, ctx, "smn_kernel_conv_resnet", 1, "relu", x, x2, "small call after a refusal")


@pytest.mark.parametrize("shape,dtype", [((2, 40, 40, 1), np.float64), ((2, 56, 56, 1), np.float64), ((2, 64, 64, 1), np.float32)])
def test_resnet_refuses_maps_beyond_the_on_chip_limit(L, ctx, shape, dtype):
    assert 12 * (shape[1] + 2) * (shape[2] + 2) * np.dtype(dtype).itemsize > 160 * 1024
    x, x2 = _small_pair(shape, dtype, 0, n2=2)
    a, b = Images(ctx, x), Images(ctx, x2)
    n = shape[0]
    for other in (None, b):
        out = ctx.to_device(np.full((n, n), np.nan, dtype))
        with pytest.raises(L.SmnError) as e:
            ctx.call("smn_kernel_conv_resnet", L.dtype_code(dtype), L.ACT["relu"], 1, *P.HYP, a.rows(), n,
                     other.rows() if other else None, n if other else 0, *shape[1:], L.FILL_FULL, out.ptr, n)
        assert e.value.code == L.ENOTSUP, str(e.value)
        assert np.isnan(out.raw_numpy()).all(), "a refused call wrote its output"
    _small_call_still_right(L, ctx, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_diag_refuses_maps_beyond_its_limit(L, ctx, dtype):
    shape = (2, 96, 96, 1)
    assert (3 * (shape[1] + 2) * (shape[2] + 2) + 256) * 8 > 160 * 1024
    xd = ctx.to_device(np.ones(shape, dtype))
    d = ctx.to_device(np.full(shape[0], np.nan, dtype))
    with pytest.raises(L.SmnError) as e:
        ctx.call("smn_kernel_conv_diag", L.dtype_code(dtype), 1, L.ACT["relu"], 1, *P.HYP, xd.ptr, *shape, d.ptr)
    assert e.value.code == L.ENOTSUP, str(e.value)
    assert np.isnan(d.raw_numpy()).all(), "a refused call wrote its output"
    x = _small_pair((3, 8, 8, 2), dtype, 5)[0]
    ref = np.diag(oracle("smn_kernel_conv_resnet", x, None, 1, "relu"))
    assert_oracle("conv_diag after a refusal", _conv_diag(L, ctx, x, 1, "relu"), ref, dtype)
    _small_call_still_right(L, ctx, dtype)


# ----------------------------------------------------------------------------- D. variance-zero pixels, scale mix
def _zero_region_images(shape, dtype):
    """Image 0 all zero, 1 with its top 6 rows zero, 2 with its right 6 columns zero, 3 with a zero centre of half the
    height and width (8 x 8 of 16 x 16), 4 dense."""
    n, H, W, _ = shape
    assert n == 5
    x = np.random.default_rng(H + W).standard_normal(shape)
    x[0] = 0.0
    x[1, :6] = 0.0
    x[2, :, W - 6:] = 0.0
    x[3, H // 4: H // 4 + H // 2, W // 4: W // 4 + W // 2] = 0.0
    return x.astype(dtype)


ZERO_CASES = [("smn_kernel_conv_resnet", (5, 16, 16, 2), 2, np.float64), ("smn_kernel_conv_resnet", (5, 16, 16, 2), 2, np.float32),
              ("smn_kernel_cnn", (5, 16, 16, 2), 3, np.float64), ("smn_kernel_cnn", (5, 16, 16, 2), 3, np.float32),
              ("smn_kernel_cnn", (5, 32, 32, 3), 3, np.float64)]      # the register-stencil kernel


@pytest.mark.parametrize("act", ["relu", "erf"])
@pytest.mark.parametrize("entry,shape,depth,dtype", ZERO_CASES)
def test_zero_regions_without_bias(L, ctx, act, entry, shape, depth, dtype):
    """b_std = 0 over zero regions: pixels with variance 0 in the per-image tables (ReLU: r = 0) and in the pair maps.  Finite
    everywhere, within RTOL of the oracle, and exactly 0 in the all-zero image's row, column and diagonal."""
    hyp = (1.2, 0.0, 0.9)
    x = _zero_region_images(shape, dtype)
    x2 = np.ascontiguousarray(x[[3, 0, 4]] * dtype(0.7))
    ref = oracle(entry, x, None, depth, act, hyp)
    assert np.isfinite(ref).all() and not ref[0].any() and not ref[:, 0].any() and (ref[1:, 1:] != 0).all()
    k, kc = _sym_and_cross(L, ctx, entry, depth, act, x, x2, "%s %s %s zero regions" % (entry, shape, act), hyp)
    assert np.isfinite(k).all() and np.isfinite(kc).all()
    assert not k[0].any() and not k[:, 0].any(), "the all-zero image's row and column"
    assert not kc[0].any() and not kc[:, 1].any(), "the all-zero image in the cross build"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("entry,shape,depth", [("smn_kernel_conv_resnet", (7, 8, 8, 2), 2), ("smn_kernel_cnn", (7, 12, 12, 2), 3)])
def test_relu_homogeneity_under_a_wide_scale_mix(L, ctx, dtype, entry, shape, depth):
    """ReLU networks without bias are positively homogeneous: K(a x_i, c x_j) = a c K(x_i, x_j).  Images scaled from 1e-3 to
    1e3 give K from 1e-7 to 5e6; relerr's floor would hide the small entries, so the NORMALISED matrix K_ij / sqrt(Kref_ii
    Kref_jj) (oracle entries all >= 0.34) is compared under RTOL: an absolute error leaking in from the fast reciprocal and
    rsqrt paths shows on the small images."""
    hyp = (1.2, 0.0, 0.9)
    x = np.random.default_rng(7).standard_normal(shape)
    x = (x * np.geomspace(1e-3, 1e3, 7).reshape(7, 1, 1, 1)).astype(dtype)
    ref = oracle(entry, x, None, depth, "relu", hyp)
    s = np.sqrt(np.diag(ref))
    norm_ref = ref / np.outer(s, s)
    assert norm_ref.min() > 0.3 and ref.max() / ref.min() > 1e11
    a = Images(ctx, x)
    k = build(L, ctx, entry, "relu", depth, a, hyp=hyp).astype(np.float64)
    assert_oracle("%s scale mix symmetric (normalised)" % entry, k / np.outer(s, s), norm_ref, dtype)
    sel = [6, 0, 3]
    b = Images(ctx, np.ascontiguousarray(x[sel]))
    kc = build(L, ctx, entry, "relu", depth, a, b=b, hyp=hyp).astype(np.float64)
    assert_oracle("%s scale mix cross (normalised)" % entry, kc / np.outer(s, s[sel]), norm_ref[:, sel], dtype)
