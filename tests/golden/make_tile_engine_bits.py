"""Records tests/golden/tile_engine_bits.json: what the MFMA tile engine (csrc/gemm_nt.hpp) computes, bit for bit, on seeded
inputs, at the smallest shapes that reach each of its forms.  tests/test_gpu_tile_engine_bits.py imports the cases and the
runners from here and compares against the recorded file, so the inputs of the recording and of the test cannot drift apart.

The fixture is recorded ONCE on the GPU from the build whose bits are the reference (the commit before a change of the
engine that promises identical bits) and not re-recorded by the change itself:

    python tests/golden/make_tile_engine_bits.py            -> tests/golden/tile_engine_bits.json
    python tests/golden/make_tile_engine_bits.py OUT.json   -> OUT.json (to compare two builds by hand)

Per case the file holds SHA-256 digests of the raw output bytes (little-endian, the dtype of the call) and, for matrix
outputs, four seeded rows for diagnosis: per row the digest of its stored part and eight seeded entries as hex bit patterns.
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "tile_engine_bits.json")

# (name, kind, arguments).  Super-panel S = 1024; the tile forms by launch size are listed in tests/test_gpu_factor.py.
CASES = [
    ("a_chol_f32_1024", "chol", dict(dtype="f32", n_total=1024, n_factor=1024)),     # quarter tiles and strips
    ("b_chol_f32_4480", "chol", dict(dtype="f32", n_total=4480, n_factor=4480)),     # 64x128 tiles (27 tile rows, 378 tiles)
    ("c_chol_f32_4992", "chol", dict(dtype="f32", n_total=4992, n_factor=4992)),     # 128x128, linear order (31 rows, 496 tiles)
    ("d_chol_f32_5248", "chol", dict(dtype="f32", n_total=5248, n_factor=5248)),     # 128x128 with the XCD map (33 tile rows)
    ("e_chol_f32_8320_8192", "chol", dict(dtype="f32", n_total=8320, n_factor=8192)),  # look-ahead schedule + an appended tile row
    ("f_chol_f64_2176", "chol", dict(dtype="f64", n_total=2176, n_factor=2176)),     # f64 engine, small
    ("g_chol_f64_5248", "chol", dict(dtype="f64", n_total=5248, n_factor=5248)),     # f64 engine with the XCD map
    ("h_gram_f32_384_96", "gram", dict(dtype="f32", n=384, d=96)),                   # build_kernel, plain loop (< 8 K-steps)
    ("i_gram_f32_384_1024", "gram", dict(dtype="f32", n=384, d=1024)),               # build_kernel, pipelined loop
    ("j_spr_loss_f32_2500_64", "loss", dict(dtype="f32", n=2500, d=64, layers=4, act="relu")),   # end-to-end scalars
]
NP = {"f32": np.float32, "f64": np.float64}
SAMPLE_ROWS, SAMPLE_COLS = 4, 8


def _seed(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def spd_matrix(name, n, dtype):
    """Seeded, symmetric, strictly diagonally dominant; the off-diagonal entries are sums of two uniform draws (no small
    integers, all mantissa bits in use), so a changed summation order changes result bits."""
    rng = np.random.default_rng(_seed(name))
    u = rng.random((n, n), dtype=dtype)
    u -= dtype(0.5)
    a = u + u.T
    del u
    np.fill_diagonal(a, 0)
    dom = np.abs(a).sum(axis=1, dtype=np.float64)
    a[np.arange(n), np.arange(n)] = (dom + 1.0 + rng.random(n)).astype(dtype)
    return a


def _hex(v):
    return np.asarray(v).tobytes().hex()


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def matrix_record(name, m, lower):
    """Digest of a matrix output (its lower triangle when `lower`) and the seeded rows."""
    n = m.shape[0]
    if lower:
        m = np.tril(m)
    rng = np.random.default_rng(_seed(name) ^ 0x5eed)
    rows = []
    for r in sorted(int(v) for v in rng.choice(n, size=SAMPLE_ROWS, replace=False)):
        width = r + 1 if lower else m.shape[1]
        cols = sorted(int(v) for v in rng.choice(width, size=min(SAMPLE_COLS, width), replace=False))
        rows.append({"row": r, "sha256": _sha(m[r, :width]), "cols": cols, "bits": [_hex(m[r, c]) for c in cols]})
    return {"sha256": _sha(m), "rows": rows}


def run_chol(L, ctx, name, dtype, n_total, n_factor):
    dt = NP[dtype]
    a = ctx.to_device(spd_matrix(name, n_total, dt))
    info, logdet = C.c_int(-7), C.c_double(-7.0)
    ctx.call("smn_cholesky", L.dtype_code(dt), a.ptr, n_total, n_factor, n_total, 0, 0.0, 0.0, C.byref(info), C.byref(logdet))
    out = {"factor": matrix_record(name, a.numpy(), lower=True), "logdet": _hex(np.float64(logdet.value)), "info": int(info.value)}
    del a
    return out


def run_gram(L, ctx, name, dtype, n, d):
    dt = NP[dtype]
    rng = np.random.default_rng(_seed(name))
    x = ctx.to_device(rng.standard_normal((n, d)).astype(dt))
    k0 = ctx.to_device(np.zeros((n, n), dt))
    q = ctx.to_device(np.zeros((n,), dt))
    ctx.call("smn_gram", L.dtype_code(dt), x.ptr, n, d, None, 0, 0, d, k0.ptr, n, q.ptr, None)
    return {"k0": matrix_record(name, k0.numpy(), lower=False), "q": _sha(q.numpy())}


def run_loss(L, ctx, name, dtype, n, d, layers, act):
    """The call bench.py times (same seed and draw order as `bench.py --n 2500 --d 64`: x, then y)."""
    dt = NP[dtype]
    rng = np.random.default_rng(0)
    x = ctx.to_device(rng.standard_normal((n, d)).astype(dt))
    y = ctx.to_device(rng.standard_normal(n).astype(dt))
    lp, quad, logdet, info = C.c_double(), C.c_double(), C.c_double(), C.c_int()
    ctx.call("smn_spr_loss", L.dtype_code(dt), L.NET_MLP, L.ACT[act], layers, 1.0, 1e-8, 1.0, x.ptr, n, d, d, y.ptr, 1e-3, 0.0, 1.0,
             C.byref(lp), C.byref(quad), C.byref(logdet), C.byref(info))
    return {"logpdf": _hex(np.float64(lp.value)), "quad": _hex(np.float64(quad.value)), "logdet": _hex(np.float64(logdet.value)),
            "info": int(info.value)}


RUNNERS = {"chol": run_chol, "gram": run_gram, "loss": run_loss}


def run_case(L, ctx, name):
    kind, kw = next((k, a) for n, k, a in CASES if n == name)
    return RUNNERS[kind](L, ctx, name, **kw)


def main():
    sys.path.insert(0, ROOT)
    from smnngp import _lib as L
    ctx = L.default_context()
    out = {"format": 1, "cases": {}}
    for name, _, _ in CASES:
        out["cases"][name] = run_case(L, ctx, name)
        print(name, json.dumps(out["cases"][name])[:160], flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
