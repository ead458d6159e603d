"""The MFMA tile engine (csrc/gemm_nt.hpp) computes the same bits as the build tests/golden/tile_engine_bits.json was recorded
from: the order in which a wave ISSUES its MFMAs is free, the order in which one accumulator element sums over k is not.

Cases, inputs and runners live in tests/golden/make_tile_engine_bits.py (the script that recorded the fixture), so the test
and the recording cannot drift apart.  Expected values are SHA-256 digests of the raw output bytes; four seeded rows per
matrix (row digest + eight entries as bit patterns) say where a mismatch sits.  No tolerance anywhere: equality of bits."""
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load_recorder():
    spec = importlib.util.spec_from_file_location("make_tile_engine_bits", os.path.join(GOLDEN, "make_tile_engine_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _load_recorder()


@pytest.fixture(scope="module")
def L():
    from smnngp import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


@pytest.fixture(scope="module")
def expected():
    with open(REC.FIXTURE) as f:
        data = json.load(f)
    assert data["format"] == 1 and sorted(data["cases"]) == sorted(n for n, _, _ in REC.CASES)
    return data["cases"]


def _diagnose(path, got, want):
    """Every leaf that differs, as 'path: got != want' lines; for hex bit patterns of one float also the two values."""
    out = []
    if isinstance(want, dict):
        for k in want:
            out += _diagnose("%s.%s" % (path, k), got.get(k), want[k])
    elif isinstance(want, list):
        if not isinstance(got, list) or len(got) != len(want):
            out.append("%s: %r != %r" % (path, got, want))
        else:
            for i, (g, w) in enumerate(zip(got, want)):
                out += _diagnose("%s[%d]" % (path, i), g, w)
    elif got != want:
        note = ""
        if isinstance(want, str) and isinstance(got, str) and len(want) == len(got) and len(want) in (8, 16):
            dt = np.float32 if len(want) == 8 else np.float64
            note = "  (%r != %r)" % tuple(float(np.frombuffer(bytes.fromhex(h), dt)[0]) for h in (got, want))
        out.append("%s: %s != %s%s" % (path, got, want, note))
    return out


@pytest.mark.parametrize("name", [n for n, _, _ in REC.CASES])
def test_same_bits_as_recorded(L, ctx, expected, name):
    got = REC.run_case(L, ctx, name)
    want = expected[name]
    assert sorted(got) == sorted(want), name
    diff = _diagnose(name, got, want)
    assert not diff, "\n".join(diff[:40])
