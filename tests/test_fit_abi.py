"""CPU-side checks of the fitted-state entries (smn_fit_*, csrc/fit.hip): the library exports the six symbols, each rejects a
NULL context or a NULL state with SMN_EINVAL before it touches a device, and the ctypes signatures have the header's argument
counts.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smnngp.h")
SYMBOLS = ("smn_fit_create", "smn_fit_create_from_kernel", "smn_fit_predict", "smn_fit_apply", "smn_fit_info", "smn_fit_destroy")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from smnngp import _lib
    return _lib


def test_library_exports_the_six_fit_entries(lib):
    raw = C.CDLL(lib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(raw, name), "libsmnngp.so does not export %s" % name
        assert name in lib.PROTOTYPES


def test_signatures_match_the_header(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"typedef\s+struct\s+smn_fit\s+smn_fit\s*;", src)
    want = {"smn_fit_create": 21, "smn_fit_create_from_kernel": 14, "smn_fit_predict": 8, "smn_fit_apply": 11, "smn_fit_info": 5,
            "smn_fit_destroy": 1}
    for name in SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
        assert m, name
        n = len(m.group(1).split(","))
        assert n == want[name] == len(lib.PROTOTYPES[name]), (name, n, len(lib.PROTOTYPES[name]))
    # no per-call dtype: it is fixed when the state is made
    for name in ("smn_fit_predict", "smn_fit_apply"):
        assert "dtype" not in re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)


def test_null_context_and_null_state_are_refused_without_a_device(lib):
    raw = lib._lib
    out = C.c_void_p()
    some = C.c_void_p(64)                                          # never dereferenced: the NULL argument is checked first
    assert raw.smn_fit_create(None, lib.F64, lib.NET_MLP, lib.ACT["relu"], 1, 1.0, 1.0, 1.0, some, 4, 4, 4, some, 1, 1e-3, 0.0, 8,
                              C.byref(out), None, None, None) == lib.EINVAL
    assert raw.smn_fit_create_from_kernel(None, lib.F64, some, 4, 4, some, 1, 1e-3, 0.0, 8, C.byref(out), None, None,
                                          None) == lib.EINVAL
    assert not out.value
    assert raw.smn_fit_predict(None, some, 1, 4, some, None, None, 0) == lib.EINVAL
    assert raw.smn_fit_apply(None, some, 1, 4, some, None, 0, some, some, None, 0) == lib.EINVAL
    n = C.c_int64(-1)
    assert raw.smn_fit_info(None, C.byref(n), None, None, None) == lib.EINVAL and n.value == -1
    assert raw.smn_fit_destroy(None) == lib.EINVAL
