"""p25fe_predecim_fmt_dev / p25fe_channelise_fmt_dev (u8 and s16 input to the two 2.4 Msps stages) at the ABI level: names in the
header, the ctypes binding, the Rust binding and the library; additive, so the ABI version stays 6.  None of this needs a GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"p25fe_predecim_fmt_dev", "p25fe_channelise_fmt_dev"}


@pytest.fixture(scope="module")
def lib():
    from p25rx_amd import _lib
    _lib.load()
    return _lib


def test_library_exports_both_symbols(lib):
    L = lib.load()
    assert NEW <= set(lib.SYMBOLS)
    for s in NEW:
        assert hasattr(L, s), s


def test_header_declares_them_and_still_says_abi_6():
    hdr = open(os.path.join(ROOT, "include", "p25fe.h")).read()
    assert re.search(r"#define P25FE_ABI_VERSION 6\b", hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert NEW <= set(re.findall(r"\b(p25fe_[a-z0-9_]+)\s*\(", code))
    # the cf32 calls keep their signatures
    assert re.search(r"int p25fe_predecim_dev\(p25fe_t \*h, const float \*d_iq, size_t ch_stride,", code)
    assert re.search(r"int p25fe_channelise_dev\(p25fe_t \*h, const float \*d_iq, size_t n_hist,", code)


def test_rust_binding_declares_both():
    rs = open(os.path.join(ROOT, "bindings", "p25fe.rs")).read()
    assert NEW <= set(re.findall(r"pub fn (p25fe_[a-z0-9_]+)\(", rs))
    for name in NEW:
        decl = rs[rs.index("pub fn " + name):]
        decl = decl[:decl.index(";")]
        assert "d_iq: *const c_void, fmt: c_int" in decl and decl.rstrip().endswith("-> c_int"), decl


def test_the_position_is_64_bit_everywhere(lib):
    """the absolute index of the first owned sample: uint64_t in the header, a 64-bit integer in ctypes, u64 in the Rust binding"""
    L = lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "p25fe.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "bindings", "p25fe.rs")).read()
    for name, idx in (("p25fe_predecim_fmt_dev", 6), ("p25fe_channelise_fmt_dev", 5)):
        params = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, hdr).group(1).split(",")
        assert re.fullmatch(r"uint64_t abs_first", params[idx].strip()), params[idx]
        assert getattr(L, name).argtypes[idx] is C.c_uint64
        rp = re.search(r"pub fn %s\(([^)]*)\)" % name, rs).group(1).split(",")
        assert rp[idx].strip() == "abs_first: u64", rp[idx]


def test_null_handle_is_an_argument_error(lib):
    L = lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    for fmt in (lib.FMT_CF32, lib.FMT_U8, lib.FMT_S16, 3, -1):
        assert L.p25fe_predecim_fmt_dev(None, p, fmt, 0, 0, 16, 0, p, 16, None) == lib.ERR_ARG
        assert L.p25fe_channelise_fmt_dev(None, p, fmt, 0, 16, 0, p, 64, None) == lib.ERR_ARG
