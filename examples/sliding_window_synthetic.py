#!/usr/bin/env python3
"""A sliding window over a stream on one fitted posterior: `FittedPosterior.remove` + `append` on the reference's offline
regression dataset.

    python examples/sliding_window_synthetic.py [syn-t|syn-normal] [--window 120] [--step 10]

The training points are read as a stream.  The model is fitted on the first `--window` of them; every step drops the `--step`
oldest points with `post.remove(range(k))` and takes in the next `--step` with `post.append(x, y)` -- O(N^2 k) each, nothing is
refitted, the state keeps its allocation (`post.max_points`, `post.nbytes` never move) and the ridge frozen when it was made
(`post.ridge`).  Printed for the Gaussian (`gp`) and the Student-t (`tp`) likelihood: the test NLL after every step, and the
time of the loop beside the same loop done by refitting (`model.posterior()` on the window's points every step; the refit
recomputes the relative ridge on each window, the moving state keeps the first).  At this size every call is a handful of
launches and removing the OLDEST points is the removal's worst case (the whole factor is re-triangularised), so the loop by
refitting is the faster one here: the example shows the surface; what a removal costs beside a refit at N = 4096 and 16384 is in
profiles/r23_fit_remove.txt.  Under `tp` every test_nll recomputes the Student-t quadratic form over the window in fp64 (see
FittedPosterior.append); the timed loops leave it out."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from examples.regression_synthetic import dataset                     # noqa: E402
from smnngp import nt_kernels                                         # noqa: E402
from smnngp.spax.kernels import NNGPKernel                            # noqa: E402
from smnngp.spax.likelihoods import GaussianLikelihood, StudentTLikelihood  # noqa: E402
from smnngp.spax.models import SPR                                    # noqa: E402


def make_model(method, x, y, ym, ys):
    kernel = NNGPKernel(lambda w, b, l: nt_kernels.get_mlp_kernel(2, act="relu", w_std=w, b_std=b, last_w_std=l), 1.0, 1.0, 1.0)
    likelihood = GaussianLikelihood() if method == "gp" else StudentTLikelihood(2.0, 2.0)
    return SPR(kernel, likelihood, x, y, ym, ys, eps=1e-2)


def run_window(method, data, window, step, steps, nll=True):
    """The moving state: [test NLL per step] (empty when nll is False: the timed form) and the loop time."""
    (x, y), (xte, yte), (ym, ys) = data
    out = []
    with make_model(method, x[:window], y[:window], ym, ys).posterior(capacity=64) as post:
        room, nbytes = post.max_points, post.nbytes
        t0 = time.perf_counter()
        for s in range(steps):
            at = window + s * step
            post.remove(range(step)).append(x[at:at + step], y[at:at + step])
            if nll:
                out.append(post.test_nll(xte, yte))
        post.ctx.synchronize()
        loop_ms = (time.perf_counter() - t0) * 1e3
        assert post.num_data == window and (post.max_points, post.nbytes) == (room, nbytes)
    return out, loop_ms


def run_refit(method, data, window, step, steps, nll=True):
    (x, y), (xte, yte), (ym, ys) = data
    out = []
    t0 = time.perf_counter()
    for s in range(steps):
        lo = (s + 1) * step
        with make_model(method, x[lo:lo + window], y[lo:lo + window], ym, ys).posterior(capacity=64) as post:   # the refit
            if nll:
                out.append(post.test_nll(xte, yte))
            post.ctx.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    argv = list(sys.argv[1:])

    def option(name, default):
        if name in argv:
            i = argv.index(name)
            value = int(argv[i + 1])
            del argv[i:i + 2]
            return value
        return default

    window, step = option("--window", 120), max(1, option("--step", 10))
    name = argv[0] if argv else "syn-t"
    (xtr, ytr), _, test, norm = dataset(name)
    window = min(window, len(ytr) - step)
    steps = (len(ytr) - window) // step
    data = ((xtr, ytr), test, norm)
    print("%s: a window of %d points moved over %d by %d steps of %d" % (name, window, len(ytr), steps, step))
    for method in ("gp", "tp"):
        run_window(method, data, window, step, min(steps, 2))                         # warm-up: workspaces, code objects
        nll_win, _ = run_window(method, data, window, step, steps)
        nll_fit, _ = run_refit(method, data, window, step, steps)
        _, ms_win = run_window(method, data, window, step, steps, nll=False)
        _, ms_fit = run_refit(method, data, window, step, steps, nll=False)
        for s, (a, b) in enumerate(zip(nll_win, nll_fit)):
            print("%s  step %2d  points [%3d, %3d)  test NLL: moving state %.6f   refit %.6f" % (method, s + 1, (s + 1) * step,
                                                                                                (s + 1) * step + window, a, b))
        print("%s  loop of %d steps by remove + append %8.2f ms   by refitting %8.2f ms" % (method, steps, ms_win, ms_fit))


if __name__ == "__main__":
    main()
