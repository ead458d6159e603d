#!/usr/bin/env python3
"""Timing of the multi-output entries (profiles/r11_multi_output.txt): this tree's library and, with --parent-lib, a build of
the parent commit's, loaded side by side in ONE process and alternated.
    python scratch/multi_output_probe.py --out FILE [--parent-lib PATH/libsmnngp.so] [--sizes 2048,16384] [--c3]
Host clock around calls that end in a synchronisation; 2 warm-up calls, min / median of `reps`."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import smnngp._lib as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--sizes", default="2048,16384")
ap.add_argument("--c3", action="store_true")
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()


class Lib:
    """A context on one build of the library, through raw ctypes (the same host code for both builds)."""

    def __init__(self, path):
        self.lib = C.CDLL(path)
        self.h = C.c_void_p()
        assert self.lib.smn_ctx_create(0, C.byref(self.h)) == 0

    def call(self, name, *a):
        fn = getattr(self.lib, name)
        fn.argtypes, fn.restype = L.PROTOTYPES[name], C.c_int
        rc = fn(self.h, *a)
        assert rc == 0, (name, rc)

    def to_device(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        self.call("smn_malloc", max(a.nbytes, 16), C.byref(p))
        self.call("smn_memcpy_h2d", p, a.ctypes.data_as(C.c_void_p), a.nbytes)
        return p

    def sync(self):
        self.call("smn_synchronize")


new = Lib(L.LIB_PATH)
par = Lib(args.parent_lib) if args.parent_lib else None
both = [lib for lib in (new, par) if lib is not None]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def clock(lib, fn, reps, before=None):
    ts = []
    for i in range(reps + 2):
        if before:
            before()
        lib.sync()
        t0 = time.perf_counter()
        fn()
        lib.sync()
        ts.append(1e3 * (time.perf_counter() - t0))
    ts = ts[2:]
    return min(ts), float(np.median(ts))


quad, logdet, lp, info, terms = C.c_double(), C.c_double(), C.c_double(), C.c_int(), (C.c_double * 4)()
if not args.c3:
    for n in [int(s) for s in args.sizes.split(",")]:
        d, layers = 3072, 4
        rng = np.random.default_rng(0)
        xh = rng.standard_normal((n, d)).astype(np.float32)
        yh = (np.eye(10)[rng.integers(0, 10, n)] - 0.1).astype(np.float32)
        dev = {}
        for lib in both:
            dev[lib] = dict(x=lib.to_device(xh), y10=lib.to_device(yh), cols=[lib.to_device(yh[:, k]) for k in range(10)])

        def single(lib, k=3):
            v = dev[lib]
            lib.call("smn_spr_loss_grad", L.F32, L.NET_MLP, L.ACT["relu"], layers, 1.3, 0.2, 1.0, v["x"], n, d, d, v["cols"][k],
                     1e-3, 4.0, 1.0, C.byref(quad), C.byref(logdet), C.byref(info), terms)

        def multi(yd, c):
            new.call("smn_spr_loss_grad_multi", L.F32, L.NET_MLP, L.ACT["relu"], layers, 1.3, 0.2, 1.0, dev[new]["x"], n, d, d, yd, c,
                     1e-3, 4.0, 1.0, C.byref(quad), None, C.byref(logdet), C.byref(info), terms)

        def ten():
            for k in range(10):
                single(new, k)

        say("N = %d, d = %d, %d-layer ReLU MLP, fp32, Student-t df = 4, eps = 1e-3 (ms: min / median of %d)" % (n, d, layers, args.reps))
        for rnd in range(2):                                   # alternated: parent, this tree, again
            if par:
                say("  parent smn_spr_loss_grad (single output)   %9.3f / %9.3f   info %d" % (*clock(par, lambda: single(par), args.reps), info.value))
            say("  smn_spr_loss_grad (single output)          %9.3f / %9.3f   info %d" % (*clock(new, lambda: single(new), args.reps), info.value))
            say("  smn_spr_loss_grad_multi C = 1              %9.3f / %9.3f   info %d" % (*clock(new, lambda: multi(dev[new]["cols"][3], 1), args.reps), info.value))
            say("  smn_spr_loss_grad_multi C = 10             %9.3f / %9.3f   info %d" % (*clock(new, lambda: multi(dev[new]["y10"], 10), args.reps), info.value))
        say("  ten smn_spr_loss_grad calls                %9.3f / %9.3f" % clock(new, ten, 3))
        for lib in both:
            for p in [dev[lib]["x"], dev[lib]["y10"]] + dev[lib]["cols"]:
                lib.call("smn_free", p)
else:
    n, h, w, c, layers = 10000, 32, 32, 3, 4
    rng = np.random.default_rng(0)
    xh = rng.standard_normal((n, h, w, c))
    xh /= np.sqrt((xh ** 2).mean(axis=(1, 2, 3), keepdims=True))
    yh = np.eye(10)[rng.integers(0, 10, n)] - 0.1
    dev = {}
    for lib in both:
        k = C.c_void_p()
        lib.call("smn_malloc", 8 * n * n, C.byref(k))
        dev[lib] = dict(x=lib.to_device(xh), y10=lib.to_device(yh), y1=lib.to_device(yh[:, 3]), k=k)

    def build(lib):
        v = dev[lib]
        lib.call("smn_kernel_cnn", L.F64, L.ACT["relu"], layers, 1.3, 0.2, 1.0, v["x"], n, None, 0, h, w, c, L.FILL_LOWER, v["k"], n)

    def lml(lib):
        v = dev[lib]
        lib.call("smn_lml", L.F64, v["k"], n, n, v["y1"], 1e-4, 4.0, 1.0, C.byref(lp), C.byref(quad), C.byref(logdet), C.byref(info))

    def lml_multi(yd, cc):
        new.call("smn_lml_multi", L.F64, dev[new]["k"], n, n, yd, cc, 1e-4, 4.0, 1.0, C.byref(lp), C.byref(quad), None,
                 C.byref(logdet), C.byref(info))

    say("C3 shape: N = %d images %dx%dx%d, %d-layer ReLU get_cnn_kernel, fp64, Student-t df = 4, eps = 1e-4" % (n, h, w, c, layers))
    say("(ms: min / median of 3; the head's window starts behind a fresh build, which is timed on its own)")
    say("  smn_kernel_cnn (lower triangle)            %9.3f / %9.3f" % clock(new, lambda: build(new), 2))
    for rnd in range(2):
        if par:
            say("  parent smn_lml (single output)             %9.3f / %9.3f   info %d" % (*clock(par, lambda: lml(par), 3, lambda: build(par)), info.value))
        say("  smn_lml (single output)                    %9.3f / %9.3f   info %d" % (*clock(new, lambda: lml(new), 3, lambda: build(new)), info.value))
        say("  smn_lml_multi C = 1                        %9.3f / %9.3f   info %d" % (*clock(new, lambda: lml_multi(dev[new]["y1"], 1), 3, lambda: build(new)), info.value))
        say("  smn_lml_multi C = 10                       %9.3f / %9.3f   info %d  logpdf %.6f" % (*clock(new, lambda: lml_multi(dev[new]["y10"], 10), 3, lambda: build(new)), info.value, lp.value))
    say("  ten single-output problems cost 10 x (build + smn_lml); the joint problem costs build + smn_lml_multi C = 10")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a") as f:
    f.write("\n".join(lines) + "\n\n")
