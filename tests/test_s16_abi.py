"""P25FE_FMT_S16 (interleaved int16 I/Q) at the ABI level: names, constants, the kernels in the code object and the
per-format variant probe.  None of this needs a GPU."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"p25fe_demod_s16", "p25fe_run_s16", "p25fe_format_variant", "p25fe_probe_format_variant"}


@pytest.fixture(scope="module")
def lib():
    from p25rx_amd import _lib
    _lib.load()
    return _lib


def test_names_and_constants_agree(lib):
    """header, ctypes binding and Rust binding name the same new symbols and the same enum value; the scale is 2^-15"""
    assert lib.FMT_S16 == 2 and lib.FMT_CF32 == 0 and lib.FMT_U8 == 1
    hdr = open(os.path.join(ROOT, "include", "p25fe.h")).read()
    assert re.search(r"P25FE_FMT_S16\s*=\s*2\b", hdr)
    assert re.search(r"#define P25FE_ABI_VERSION 6\b", hdr)               # additive: no ABI bump
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(p25fe_[a-z0-9_]+)\s*\(", code))
    assert NEW <= declared and NEW <= set(lib.SYMBOLS)
    L = lib.load()
    assert all(hasattr(L, s) for s in NEW)
    rs = open(os.path.join(ROOT, "bindings", "p25fe.rs")).read()
    assert NEW <= set(re.findall(r"pub fn (p25fe_[a-z0-9_]+)\(", rs))
    assert "pub const FMT_S16: c_int = 2;" in rs
    m = re.search(r"#define P25FE_S16_SCALE\s+(\S+)", hdr)
    assert m and float.fromhex(m.group(1).rstrip("f")) == 2.0 ** -15 == lib.S16_SCALE
    # what the definition rests on: every int16 times 2^-15 is exact in fp32, and -32768 is -1.0
    v = np.arange(-32768, 32768, dtype=np.int64)
    f = v.astype(np.int16).astype(np.float32) * np.float32(2.0 ** -15)
    assert np.array_equal(f.astype(np.float64) * 32768.0, v.astype(np.float64)) and f[0] == -1.0


def _library_kernels(so):
    """{mangled kernel name: scratch bytes per lane} of the gfx950 code object bundled in the library"""
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", so, fat])
        subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + os.path.join(d, "k.hsaco")],
                              stderr=subprocess.DEVNULL)
        out = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", os.path.join(d, "k.hsaco")]).decode()
    names = re.findall(r"\.name:\s+(\S+)", out)
    scr = [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", out)]
    assert len(names) == len(scr)
    return dict(zip(names, scr))


def test_code_object_holds_the_s16_kernels_without_scratch(lib):
    """the same set of instantiations u8 and cf32 have -- k_frontend: built-in x {3, 5 outputs per lane linear, planar}, generic x
    {3, 5 linear, planar} and the long geometry linear / planar = 8; k_chunk: built-in, generic, long = 3 -- counted by the
    format's template argument in the mangled name (Li<fmt>E first); none uses scratch"""
    k = _library_kernels(lib.LIB_PATH)
    for fmt in (lib.FMT_CF32, lib.FMT_U8, lib.FMT_S16):
        fr = {n: s for n, s in k.items() if re.match(r"_ZN4p25k10k_frontendILi%dE" % fmt, n)}
        ch = {n: s for n, s in k.items() if re.match(r"_ZN4p25k7k_chunkILi%dE" % fmt, n)}
        assert len(fr) == 8 and len(ch) == 3, (fmt, sorted(fr), sorted(ch))
        assert all(s == 0 for s in list(fr.values()) + list(ch.values())), (fmt, fr, ch)


def _random_tables(lib, **kw):
    rng = np.random.default_rng(5)
    dt = (rng.standard_normal(31) * 0.1).astype(np.float32)
    ct = (rng.standard_normal(41) * 0.1).astype(np.float32)
    return lib.make_config(decim_taps=list(dt), chan_taps=list(ct), **kw)


def test_probe_format_variant(lib, tmp_path, monkeypatch):
    monkeypatch.setenv("P25FE_QUIET", "1")
    monkeypatch.setenv("P25FE_CACHE_DIR", str(tmp_path / "cache"))
    monkeypatch.delenv("P25FE_SPEC_DIR", raising=False)
    L = lib.load()
    import ctypes as C
    dflt = lib.default_config()
    for fmt in (lib.FMT_CF32, lib.FMT_U8, lib.FMT_S16):
        assert lib.probe_format_variant(dflt, fmt) == lib.VARIANT_BUILTIN
    # other numbers, specialisation switched off: generic kernels for everybody
    off = _random_tables(lib, specialize=lib.SPECIALIZE_OFF)
    assert lib.probe_variant(off) == lib.VARIANT_GENERIC
    for fmt in (lib.FMT_CF32, lib.FMT_U8, lib.FMT_S16):
        assert lib.probe_format_variant(off, fmt) == lib.VARIANT_GENERIC
    # ... left to the library: u8 and cf32 get what p25fe_probe_variant says (specialised kernels, compiled here without a GPU), s16
    # the generic ones
    auto = _random_tables(lib)
    pv = lib.probe_variant(auto)
    assert lib.probe_format_variant(auto, lib.FMT_CF32) == pv and lib.probe_format_variant(auto, lib.FMT_U8) == pv
    assert lib.probe_format_variant(auto, lib.FMT_S16) == lib.VARIANT_GENERIC
    # ... demanded: s16 cannot have them
    req = _random_tables(lib, specialize=lib.SPECIALIZE_REQUIRE)
    assert L.p25fe_probe_format_variant(C.byref(req), lib.FMT_S16) == lib.ERR_JIT
    assert lib.probe_format_variant(req, lib.FMT_CF32) == lib.probe_variant(req)
    # FORCE with the build's own numbers: the built-in s16 kernels carry those numbers
    assert lib.probe_format_variant(lib.make_config(specialize=lib.SPECIALIZE_REQUIRE), lib.FMT_S16) == lib.VARIANT_BUILTIN
    for bad in (3, -1):
        assert L.p25fe_probe_format_variant(C.byref(dflt), bad) == lib.ERR_ARG
    assert L.p25fe_probe_format_variant(None, lib.FMT_S16) == lib.ERR_ARG
    assert L.p25fe_format_variant(None, lib.FMT_S16) == lib.ERR_ARG


def test_to_s16_rounds_and_clips():
    from p25rx_amd import c4fm
    iq = np.array([0.0 + 0.0j, 1.0 - 1.0j, 0.5 + 0.25j, 2.0 - 2.0j], dtype=np.complex64)
    s = c4fm.to_s16(iq)
    assert s.dtype == np.int16 and s.tolist() == [0, 0, 32767, -32767, 16384, 8192, 32767, -32768]
    assert c4fm.to_s16(iq[:2], full_scale=1000).tolist() == [0, 0, 1000, -1000]


def test_capture_survives_quantisation(c4fm_1s):
    """the 1 s capture the GPU tests use, as s16: the oracle recovers the modulator's dibits from it without an error"""
    from oracle import oracle as O
    from p25rx_amd import c4fm
    iq, truth, _ = c4fm_1s
    s = c4fm.to_s16(iq)
    conv = (s.astype(np.float32) * np.float32(2.0 ** -15)).view(np.complex64)
    d = O.run_cf32(conv)
    assert len(d) == 4769 and np.array_equal(d, O.run_cf32(iq))
    k, j, n, err = c4fm.align_dibits(d, truth)
    assert err == 0 and n > 4700
