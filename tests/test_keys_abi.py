"""CPU tests of the host side of the keys computed on the device (docs/SPEC.md 3.0k): the ABI surface and every refusal that needs
no device.  What the kernels compute is tests/test_gpu_keys.py's; their registers are tests/test_isa_keys.py's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"p25fe_keys_create", "p25fe_keys_destroy", "p25fe_keys_dev", "p25fe_keys_stream", "p25fe_keys_read"}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from p25rx_amd import _lib
    return _lib


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def test_abi_surface(lib):
    """header, ctypes and the Rust text name the same five functions; none begins with or contains what the older ABI tests pin;
    slot0 is 64-bit everywhere; the ABI version has not moved; the kernels' source is a dependency of the library and of its
    sanitizer build and is not embedded for hipRTC"""
    hdr = open(os.path.join(ROOT, "include", "p25fe.h")).read()
    assert re.search(r"#define P25FE_ABI_VERSION 6\b", hdr) and lib.ABI_VERSION == 6
    assert re.search(r"#define P25FE_KEYS_MAX_CHANNELS 4096\b", hdr) and lib.KEYS_MAX_CHANNELS == 4096
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(p25fe_[a-z0-9_]+)\s*\(", code))
    assert {s for s in declared if s.startswith("p25fe_keys")} == NEW and NEW <= set(lib.SYMBOLS)
    assert "typedef struct p25fe_keys p25fe_keys_t;" in code
    for s in NEW:
        assert not s.startswith(("p25fe_waterfall", "p25fe_scan", "p25fe_afc_", "p25fe_track_")), s
        assert not any(w in s for w in ("cuts", "tune", "nco", "resampl")), s
    rs = open(os.path.join(ROOT, "bindings", "p25fe.rs")).read()
    assert NEW <= set(re.findall(r"pub fn (p25fe_[a-z0-9_]+)\(", rs)) and "pub enum Keys {}" in rs
    L = lib.load()
    for s in NEW:
        assert hasattr(L, s) and getattr(L, s).argtypes is not None, s
    assert len(L.p25fe_keys_create.argtypes) == 10 and L.p25fe_keys_dev.argtypes[4] is C.c_uint64
    m = re.search(r"int p25fe_keys_dev\((.*?)\)", code, re.S)
    assert [a.strip() for a in m.group(1).split(",")] == ["p25fe_keys_t *kp", "const uint64_t *d_rows", "size_t n_rows", "size_t row_stride",
                                                          "uint64_t slot0", "void *stream"]
    m = re.search(r"pub fn p25fe_keys_dev\((.*?)\)", rs, re.S)
    assert [a.split(":")[1].strip() for a in m.group(1).split(",") if a.strip()] == ["*mut Keys", "*const u64", "usize", "usize", "u64",
                                                                                     "*mut c_void"]
    m = re.search(r"int p25fe_keys_create\((.*?)\)", code, re.S)
    assert [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == [
        "sc", "fs_hz", "raster_hz", "half_bw_hz", "on_db", "off_db", "min_slots", "max_rows", "max_keys", "out"]
    m = re.search(r"pub fn p25fe_keys_read\((.*?)\)", rs, re.S)
    assert "*mut WaterfallKey" in m.group(1)
    mk = open(os.path.join(ROOT, "p25rx_amd", "csrc", "Makefile")).read()
    ksrc = re.search(r"^KSRC\s*:=(.*)$", mk, re.M).group(1)
    assert "p25fe_keys.inc" not in ksrc
    for target in (r"\$\(APIO\)", r"\$\(ASAN_LIB\)"):
        deps = re.search(r"^%s:(.*)$" % target, mk, re.M).group(1)
        assert "$(HERE)p25fe_keys.inc" in deps, target
    api = open(os.path.join(ROOT, "p25rx_amd", "csrc", "p25fe_api.hip")).read()
    assert api.index('#include "p25fe_cuts.inc"') < api.index('#include "p25fe_keys.inc"')
    import p25rx_amd
    assert p25rx_amd.Keys.__name__ == "Keys" and hasattr(p25rx_amd.Scanner, "keys_plan")
    for name in ("run_dev", "run_stream", "read", "close"):
        assert callable(getattr(p25rx_amd.Keys, name))


def test_refusals_need_no_device(lib):
    """every refusal of the five calls with no object: nothing here reaches a device.  p25fe_keys_create takes N from the survey
    object, so a null one is looked at first: whatever else is right or wrong, P25FE_ERR_ARG and a null *out"""
    L = lib.load()
    ok = dict(fs=2500000, raster=12500.0, half_bw=4000.0, on=20.0, off=14.0, min_slots=2, max_rows=16, max_keys=16)

    def create(sc=None, null_out=False, **kw):
        a = dict(ok, **kw)
        out = C.c_void_p(12345)
        rc = L.p25fe_keys_create(sc, a["fs"], a["raster"], a["half_bw"], a["on"], a["off"], a["min_slots"], a["max_rows"], a["max_keys"],
                                 None if null_out else C.byref(out))
        return rc, out.value
    assert create() == (lib.ERR_ARG, None)
    assert create(null_out=True)[0] == lib.ERR_ARG
    for kw in (dict(on=14.0, off=20.0), dict(on=float("nan")), dict(off=float("nan")), dict(on=float("inf")), dict(off=float("-inf")),
               dict(min_slots=0), dict(raster=0.0), dict(raster=float("nan")), dict(raster=-1.0), dict(half_bw=-1.0),
               dict(half_bw=float("inf")), dict(fs=0), dict(max_rows=0), dict(max_rows=(1 << 20) + 1), dict(max_keys=0),
               dict(max_keys=(1 << 20) + 1), dict(fs=20000000, raster=1.0)):
        assert create(**kw) == (lib.ERR_ARG, None), kw
    rows = np.zeros((2, 1025), dtype=np.uint64)
    out = np.zeros(4, dtype=lib.WATERFALL_KEY_DTYPE)
    out["reserved"] = -99
    n = C.c_size_t(5)
    for d_rows, n_rows, stride in ((vp(rows), 2, 1025), (None, 2, 1025), (C.c_void_p(rows.ctypes.data + 4), 2, 1025), (vp(rows), 2, 8),
                                   (vp(rows), 0, 1025)):
        assert L.p25fe_keys_dev(None, d_rows, n_rows, stride, 0, None) == lib.ERR_ARG
    assert L.p25fe_keys_stream(None) == lib.ERR_ARG
    assert L.p25fe_keys_read(None, vp(out), 4, C.byref(n)) == lib.ERR_ARG and n.value == 0
    assert L.p25fe_keys_read(None, vp(out), 4, None) == lib.ERR_ARG
    assert L.p25fe_keys_read(None, None, 4, C.byref(n)) == lib.ERR_ARG
    assert (out["reserved"] == -99).all() and not rows.any()
    L.p25fe_keys_destroy(None)                                       # destroying nothing is allowed
