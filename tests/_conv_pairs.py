"""What the multi-pass tests of the conv-NNGP pair kernels share (tests/test_gpu_conv_pairs.py; checked on the CPU by
tests/test_conv_pairs_host.py).

smn_kernel_cnn and smn_kernel_conv_resnet give one wave one image pair and cap the launch at 2048 workgroups of 4 waves, so
from GRID_WAVES + 1 pairs on a wave walks several pairs ("passes") and carries its LDS maps, rings, dummy slots and registers
from one pair to the next.  This module knows the plain pair order of those kernels: which pass visits a pair, a sample of
rows and columns that touches every pass, and the single-pass cross calls a symmetric matrix can be assembled from."""
import math

import numpy as np

# The launch cap of both builders: `if (blocks > 256 * 8) blocks = 256 * 8;` in cnn_t (csrc/cnn.hip) and in resnet_t
# (csrc/cnn_resnet.hip), 4 waves per workgroup, one pair per wave and pass.
GRID_WAVES = 256 * 8 * 4
assert GRID_WAVES == 8192

MAX_SAMPLE = 16                 # rows and columns of a sampled oracle block
ORACLE_FULL_STATE = 4 << 20     # n1 n2 H W elements of oracle state up to which the whole matrix is compared

HYP = (1.2, 0.3, 0.9)           # w_std, b_std, last_w_std


def npairs(n, sym=True, n2=None):
    return n * (n + 1) // 2 if sym else n * n2


def passes(num_pairs):
    """Pairs the busiest wave walks in the plain order."""
    return -(-num_pairs // GRID_WAVES)


def pair_number(n, m, sym, n2=None):
    """Lower-triangle numbering pr = n (n + 1) / 2 + m (m <= n) of the symmetric build, pr = n * n2 + m of a cross build."""
    if sym:
        n, m = max(n, m), min(n, m)
        return n * (n + 1) // 2 + m
    return n * n2 + m


def pass_of(n, m, sym, n2=None):
    return pair_number(n, m, sym, n2) // GRID_WAVES


def decode(pr, sym, n2=None):
    """(n, m) of pair number pr."""
    if sym:
        n = (math.isqrt(8 * pr + 1) - 1) // 2
        return n, pr - n * (n + 1) // 2
    return pr // n2, pr % n2


def sample_rows_cols(n, sym=True, n2=None, seed=0):
    """At most MAX_SAMPLE rows and MAX_SAMPLE columns (sorted, unique): 0, 1 and the last index of each side, the row and the
    column of one pair out of the middle of EVERY pass, and random further ones.  In the symmetric case the sampled block
    [rows] x [cols] holds pair (max, min) for every (row, col) in it."""
    m_last = (n if sym else n2) - 1
    rows, cols = {0, min(1, n - 1), n - 1}, {0, min(1, m_last), m_last}
    total = npairs(n, sym, n2)
    for p in range(passes(total)):
        r, c = decode(min(p * GRID_WAVES + GRID_WAVES // 2, total - 1), sym, n2)
        rows.add(r)
        cols.add(c)
    assert len(rows) <= MAX_SAMPLE and len(cols) <= MAX_SAMPLE, "more passes than a sample can hold"
    rng = np.random.default_rng(seed)
    for chosen, extent in ((rows, n), (cols, m_last + 1)):
        for i in rng.permutation(extent):
            if len(chosen) >= min(MAX_SAMPLE, extent):
                break
            chosen.add(int(i))
    return np.array(sorted(rows)), np.array(sorted(cols))


def sampled_passes(rows, cols, sym, n2=None):
    """The passes the pairs of the sampled block belong to."""
    return {pass_of(int(r), int(c), sym, n2) for r in rows for c in cols}


def row_chunks(n, n2):
    """[r0, r1) ranges that cover the n rows once, each with (r1 - r0) * n2 <= GRID_WAVES: a cross call of x[r0:r1] against
    n2 images in which every wave handles one pair."""
    step = GRID_WAVES // n2
    assert step >= 1, "one row is more than a pass"
    return [(r0, min(r0 + step, n)) for r0 in range(0, n, step)]


def scaled_images(shape, dtype, seed):
    """Gaussian images, image i scaled by 1 + i / n: two swapped or misplaced pairs differ far beyond any tolerance."""
    n = shape[0]
    x = np.random.default_rng(seed).standard_normal(shape)
    x *= (1.0 + np.arange(n) / n).reshape((n,) + (1,) * (len(shape) - 1))
    return x.astype(dtype)


def aligned_ld(cols, dtype, extra=1):
    """A leading dimension above `cols` whose rows are a multiple of 16 bytes."""
    al = 16 // np.dtype(dtype).itemsize
    return (cols + extra + al - 1) // al * al


# ------------------------------------------------------------------------------------------------ the cases
# (entry, (H, W, C), depth, n, n2 or None, min passes): every multi-pass build of tests/test_gpu_conv_pairs.py, so the host test
# can check the premise of each.  n = 222: 24,753 pairs, 4 passes.  150 x 111: 16,650 pairs, 3 passes, 111 odd against the
# 8192-wave stride.  181: 16,471 pairs, 3 passes.  n = 130 (8,515 pairs) is the smallest symmetric build with a second pass.
RESNET_SYM = [((8, 8, 1), 1), ((16, 8, 2), 2)]
RESNET_CROSS = ((8, 8, 3), 1, 150, 111)
RESNET_32 = [(130, 2), (181, 3)]
# smn_kernel_cnn: (H, W, C), dtypes, layers, the form of launch_pairs (csrc/cnn.hip) the case is meant to reach
CNN_FORMS = [
    ((32, 32, 1), ("f64",), 2, "conv_pair44_kernel<C=1>"),
    ((32, 32, 3), ("f64",), 2, "conv_pair44_kernel<C=3>"),
    ((32, 32, 2), ("f64",), 2, "conv_pair32_kernel"),
    ((32, 32, 3), ("f32",), 2, "conv_pair_kernel<16,exact>"),
    ((16, 64, 1), ("f64",), 2, "conv_pair_kernel<16,exact> fp64 KB=4"),
    ((16, 16, 2), ("f32", "f64"), 2, "conv_pair_kernel<4,exact>"),
    ((8, 8, 2), ("f32", "f64"), 2, "conv_pair_kernel<4,ragged>"),
    ((28, 28, 1), ("f32", "f64"), 2, "conv_pair_kernel<16,ragged>"),
    ((40, 40, 1), ("f32", "f64"), 2, "conv_pair_kernel<64,ragged>"),
    ((64, 64, 1), ("f32", "f64"), 1, "conv_pair_kernel<64,exact>"),
]
N_SYM = 222


def cnn_form(shape, dtype_name):
    """The dispatch of launch_pairs (csrc/cnn.hip) restated: which pair kernel an image shape and dtype reach."""
    h, w, c = shape
    if h == 32 and w == 32 and dtype_name == "f64":
        return "conv_pair44_kernel<C=%d>" % c if c in (1, 3) else "conv_pair32_kernel"
    hw = h * w
    for np_ in (4, 16, 64):
        if hw <= 64 * np_:
            exact = hw == 64 * np_ and 64 % w == 0
            return "conv_pair_kernel<%d,%s>" % (np_, "exact" if exact else "ragged")
    return None


def multi_pass_builds():
    """(label, n, sym, n2, min passes) of every multi-pass build."""
    out = [("resnet %s" % (s,), N_SYM, True, None, 3) for s, _ in RESNET_SYM]
    out.append(("resnet cross %s" % (RESNET_CROSS[0],), RESNET_CROSS[2], False, RESNET_CROSS[3], 3))
    out += [("resnet (32, 32, 3) n=%d" % n, n, True, None, p) for n, p in RESNET_32]
    out += [("cnn %s" % (s,), N_SYM, True, None, 3) for s, _, _, _ in CNN_FORMS]
    return out
