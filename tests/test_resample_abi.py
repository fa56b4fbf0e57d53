"""CPU tests of the rational resampler's host side (docs/SPEC.md 3.0b): the ABI surface, the count function, the design helper and
the argument checks that need no device.  The GPU side is tests/test_gpu_resample.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import resample_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"p25fe_resampler_design", "p25fe_resampler_create", "p25fe_resampler_destroy", "p25fe_resampler_reset", "p25fe_n_resample",
       "p25fe_resample_dev", "p25fe_resample"}
# 16 tuner rates from 0.25 to 20 Msps: the RTL-SDR's customary ones, the Airspy's, the HackRF's span
RATES = (250000, 960000, 1024000, 1920000, 2000000, 2048000, 2400000, 2500000, 3000000, 4000000, 5000000, 6000000, 8000000,
         10000000, 12000000, 20000000)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from p25rx_amd import _lib
    return _lib


def test_abi_surface(lib):
    """header, ctypes and the Rust text name the same new symbols; the ABI version has not moved"""
    hdr = open(os.path.join(ROOT, "include", "p25fe.h")).read()
    assert re.search(r"#define P25FE_ABI_VERSION 6\b", hdr) and lib.ABI_VERSION == 6
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(p25fe_[a-z0-9_]+)\s*\(", code))
    assert NEW <= declared and NEW <= set(lib.SYMBOLS)
    assert {s for s in declared if "resampl" in s} == NEW
    rs = open(os.path.join(ROOT, "bindings", "p25fe.rs")).read()
    assert NEW <= set(re.findall(r"pub fn (p25fe_[a-z0-9_]+)\(", rs))
    L = lib.load()
    for s in NEW:
        assert getattr(L, s).argtypes is not None, s
    for name, val in (("L", 32), ("M", 1024), ("T", 1024), ("TABLE", 4096)):
        assert re.search(r"#define P25FE_RS_MAX_%s %d\b" % (name, val), hdr), name
        assert getattr(lib, "RS_MAX_" + name) == val
        assert "pub const RS_MAX_%s: i32 = %d;" % (name, val) in rs
    assert L.p25fe_n_resample.argtypes[2] is C.c_uint64 and L.p25fe_resample_dev.argtypes[6] is C.c_uint64
    m = re.search(r"pub fn p25fe_resample_dev\(([^)]*)\)", rs)
    assert [p.strip() for p in m.group(1).split(",")][6] == "abs_first: u64"


def test_n_resample(lib):
    """the count of {m : abs_first <= n_m < abs_first + n} by brute force for small cases, the closed form in Python integers at
    large positions, 0 for a ratio outside the limits"""
    L = lib.load()
    for (l, m) in ((1, 10), (12, 125), (15, 128), (3, 250), (24, 25), (2, 25), (31, 32), (1, 2), (32, 1023)):
        n_m = (np.arange(3000, dtype=np.int64) * m + m - 1) // l       # every output's input index, ascending
        for a in list(range(0, 2 * m + 3)) + [977, 1000]:
            for n in (0, 1, 2, 3, m // l, m // l + 1, m - 1, m, m + 1, 2 * m + 1, 777):
                want = int(np.count_nonzero((n_m >= a) & (n_m < a + n)))
                assert a + n < n_m[-1]
                assert L.p25fe_n_resample(l, m, a, n) == want == RM.n_resample(l, m, a, n), (l, m, a, n)
        for two in (32, 40, 56):
            for d in range(-m - 2, m + 3, 7):
                for n in (0, 1, 9, m, 16384, 240000, (1 << 31) + 7, (1 << 33) + 3):
                    a = (1 << two) + d
                    assert L.p25fe_n_resample(l, m, a, n) == RM.n_resample(l, m, a, n), (l, m, a, n)
        for a in ((1 << 62) - 1, (1 << 62) - 1 - m, (1 << 62) - 2):
            for n in (0, 1, m, 4099, (1 << 33) + 3):
                assert L.p25fe_n_resample(l, m, a, n) == RM.n_resample(l, m, a, n), (l, m, a, n)
    for (l, m) in ((2, 4), (10, 10), (11, 10), (0, 5), (33, 34), (1, 1025), (-1, 5), (6, 9)):
        assert L.p25fe_n_resample(l, m, 0, 100000) == 0, (l, m)


def _design(L, fs, cap=None):
    l, m, t = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    taps = np.full(cap if cap is not None else 4096, np.float32(np.nan), dtype=np.float32)
    rc = L.p25fe_resampler_design(fs, C.byref(l), C.byref(m), C.byref(t), taps.ctypes.data_as(C.c_void_p), taps.size)
    return rc, l.value, m.value, t.value, taps


def test_design_shapes_and_errors(lib):
    L = lib.load()
    for fs, shape in ((2400000, (1, 10, 80)), (2500000, (12, 125, 84)), (10000000, (3, 125, 334)), (2048000, (15, 128, 69)),
                      (250000, (24, 25, 9))):
        rc, l, m, t, taps = _design(L, fs)
        assert rc == lib.OK and (l, m, t) == shape, (fs, l, m, t)
        assert np.isfinite(taps[:l * t]).all() and np.isnan(taps[l * t:]).all()       # exactly L T floats written
        # too little room: the sizes are filled, the table is not touched
        rc, l, m, t, small = _design(L, fs, cap=shape[0] * shape[2] - 1)
        assert rc == lib.ERR_CAPACITY and (l, m, t) == shape and np.isnan(small).all()
        l_, m_, t_ = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        assert L.p25fe_resampler_design(fs, C.byref(l_), C.byref(m_), C.byref(t_), None, 0) == lib.ERR_CAPACITY
        assert (l_.value, m_.value, t_.value) == shape
    for fs in (240000, 0, 2400001):                                  # L = M; no rate; a reduced M of 2 400 001
        assert _design(L, fs)[0] == lib.ERR_ARG, fs
    assert L.p25fe_resampler_design(2400000, None, None, None, None, 0) == lib.ERR_ARG


@pytest.mark.parametrize("fs", RATES)
def test_design_response(lib, fs):
    """from the returned table: at most 0.15 dB of droop up to 12 kHz, at least 78 dB down from 199 kHz to L fs / 2, every phase's
    taps sum to 1 within 1e-3, all of them to L within 1e-5 L; and the table is the float64 restatement rounded once, to the last
    bit but for the library's own I0 and sin (a few ulp of a double before the rounding)"""
    L = lib.load()
    rc, l, m, t, taps = _design(L, fs)
    assert rc == lib.OK
    ml, mm, mt, hd = RM.design(fs)
    assert (l, m, t) == (ml, mm, mt) and l * t <= 4096
    h = taps[:l * t].astype(np.float64)
    nfft = 1 << 19
    H = np.abs(np.fft.rfft(h, nfft)) / l
    f = np.arange(len(H)) * (float(l) * fs / nfft)
    with np.errstate(divide="ignore"):
        db = 20.0 * np.log10(H)
    droop, stop = db[f <= 12000.0].min(), db[f >= 199000.0].max()
    print("fs %d: L/M/T %d/%d/%d droop %.4f dB stop %.2f dB" % (fs, l, m, t, droop, stop))
    assert droop >= -0.15, droop
    assert stop <= -78.0, stop
    per_phase = np.array([h[p::l].sum() for p in range(l)])
    assert np.abs(per_phase - 1.0).max() <= 1e-3, per_phase
    assert abs(h.sum() - l) <= 1e-5 * l
    assert np.abs(h - hd).max() <= 2.0 ** -23 * np.abs(hd).max()      # one fp32 rounding of the same prototype (half an ulp at the peak, and slack for libm)


def test_create_checks_its_arguments_before_any_device(lib):
    """a ratio that is not in lowest terms, L >= M, L T > 4096 and the other limits answer P25FE_ERR_ARG with no handle at all"""
    L = lib.load()
    taps = np.zeros(8192, dtype=np.float32)
    out = C.c_void_p(1)
    for (l, m, t) in ((2, 4, 8), (6, 9, 8), (10, 10, 8), (11, 10, 8), (8, 125, 513), (32, 1023, 129), (0, 10, 8), (33, 34, 8),
                      (1, 1025, 8), (1, 10, 0), (1, 10, 1025), (-3, 10, 8)):
        out.value = 1
        assert L.p25fe_resampler_create(None, l, m, t, taps.ctypes.data_as(C.c_void_p), C.byref(out)) == lib.ERR_ARG, (l, m, t)
        assert not out.value
    assert L.p25fe_resampler_create(None, 1, 10, 80, taps.ctypes.data_as(C.c_void_p), C.byref(out)) == lib.ERR_ARG   # no handle
    assert L.p25fe_resampler_create(None, 1, 10, 80, None, C.byref(out)) == lib.ERR_ARG
    assert L.p25fe_resampler_create(None, 1, 10, 80, taps.ctypes.data_as(C.c_void_p), None) == lib.ERR_ARG
    assert L.p25fe_resampler_reset(None) == lib.ERR_ARG
    L.p25fe_resampler_destroy(None)                                  # a no-op
    n_out = C.c_size_t(0)
    assert L.p25fe_resample(None, None, 0, 0, None, 0, C.byref(n_out)) == lib.ERR_ARG
    assert L.p25fe_resample_dev(None, None, 0, 0, 0, 0, 0, None, 0, None) == lib.ERR_ARG
