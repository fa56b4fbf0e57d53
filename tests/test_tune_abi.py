"""CPU tests of the tuner's host side (docs/SPEC.md 3.0c): the ABI surface, p25fe_tuner_freq, the rotator table, the argument checks
that need no device, and the numpy model (tests/tune_model.py) against the formula in double precision and against itself.  The GPU
side is tests/test_gpu_tune.py."""
import ctypes as C
import os
import re
from math import gcd

import numpy as np
import pytest

import resample_model as RM
import tune_model as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"p25fe_tuner_freq", "p25fe_tuner_rotator", "p25fe_tuner_create", "p25fe_tuner_destroy", "p25fe_tuner_reset", "p25fe_tune_dev",
       "p25fe_tune"}
# (tuner rate, channel offset in Hz, num, den)
FREQS = ((2500000, 137500, 11, 200), (2048000, -412500, -825, 4096), (10000000, 3012500, 241, 800), (2500000, 0, 0, 1))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from p25rx_amd import _lib
    return _lib


def _freq(L, fs, off):
    num, den = C.c_int32(-7), C.c_int32(-7)
    return L.p25fe_tuner_freq(fs, off, C.byref(num), C.byref(den)), num.value, den.value


def _rot(L, den):
    cs = np.full(2 * den, np.float32(np.nan), dtype=np.float32)
    assert L.p25fe_tuner_rotator(den, cs.ctypes.data_as(C.c_void_p), cs.size) == 0
    return cs[:den].copy(), cs[den:].copy()


def test_abi_surface(lib):
    """header, ctypes and the Rust text name the same seven functions and two limits; the ABI version has not moved"""
    hdr = open(os.path.join(ROOT, "include", "p25fe.h")).read()
    assert re.search(r"#define P25FE_ABI_VERSION 6\b", hdr) and lib.ABI_VERSION == 6
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(p25fe_[a-z0-9_]+)\s*\(", code))
    assert NEW <= declared and NEW <= set(lib.SYMBOLS)
    assert {s for s in declared if "tune" in s} == NEW
    rs = open(os.path.join(ROOT, "bindings", "p25fe.rs")).read()
    assert NEW <= set(re.findall(r"pub fn (p25fe_[a-z0-9_]+)\(", rs))
    L = lib.load()
    for s in NEW:
        assert getattr(L, s).argtypes is not None, s
    for name, val in (("CH", 256), ("DEN", 8192)):
        assert re.search(r"#define P25FE_TUNE_MAX_%s\s+%d\b" % (name, val), hdr), name
        assert getattr(lib, "TUNE_MAX_" + name) == val
        assert "pub const TUNE_MAX_%s: i32 = %d;" % (name, val) in rs
    assert L.p25fe_tune_dev.argtypes[5] is C.c_uint64 and L.p25fe_tuner_freq.argtypes[1] is C.c_int64
    m = re.search(r"pub fn p25fe_tune_dev\(([^)]*)\)", rs)
    assert [p.strip() for p in m.group(1).split(",")][5] == "abs_first: u64"


def test_freq(lib):
    L = lib.load()
    for fs, off, num, den in FREQS:
        assert _freq(L, fs, off) == (lib.OK, num, den), (fs, off)
        assert _freq(L, fs, -off) == (lib.OK, -num, den), (fs, off)
    assert _freq(L, 2400000, -12500 * 92) == (lib.OK, -23, 48) and _freq(L, 2400000, 12500 * 5) == (lib.OK, 5, 192)
    assert _freq(L, 2500000, 1250000) == (lib.OK, 1, 2) and _freq(L, 2500000, -1250000) == (lib.OK, -1, 2)     # Nyquist itself
    for fs, off in ((2500000, 1250001), (2500000, -1250001), (2500000, 1 << 40), (2500000, -(1 << 63)), (0, 0), (0, 100)):
        assert _freq(L, fs, off)[0] == lib.ERR_ARG, (fs, off)
    assert _freq(L, 2048000, 6250) == (lib.OK, 25, 8192)             # den 8192 is accepted,
    assert _freq(L, 2048000, 3125)[0] == lib.ERR_ARG                 # den 16384 is not
    n = C.c_int32(0)
    assert L.p25fe_tuner_freq(2500000, 0, None, C.byref(n)) == lib.ERR_ARG
    assert L.p25fe_tuner_freq(2500000, 0, C.byref(n), None) == lib.ERR_ARG


def test_rotator(lib):
    """every entry within one fp32 ulp of numpy's double cos / sin; entry 0 exact; capacity and argument errors"""
    L = lib.load()
    for den in (1, 2, 200, 4096, 8192):
        c, s = _rot(L, den)
        a = 2.0 * np.pi * np.arange(den, dtype=np.float64) / den
        for got, ref in ((c, np.cos(a)), (s, np.sin(a))):
            ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
            assert (np.abs(got.astype(np.float64) - ref) <= ulp).all(), den
        assert c[0] == 1.0 and s[0] == 0.0 and not np.signbit(s[0])
    cs = np.full(400, np.float32(np.nan), dtype=np.float32)
    assert L.p25fe_tuner_rotator(200, cs.ctypes.data_as(C.c_void_p), 399) == lib.ERR_CAPACITY and np.isnan(cs).all()
    assert L.p25fe_tuner_rotator(200, None, 0) == lib.ERR_CAPACITY
    for den in (0, -1, 8193):
        assert L.p25fe_tuner_rotator(den, cs.ctypes.data_as(C.c_void_p), cs.size) == lib.ERR_ARG, den


def test_create_checks_its_arguments_before_any_device(lib):
    """every limit answers P25FE_ERR_ARG with no handle at all"""
    L = lib.load()
    taps = np.zeros(8192, dtype=np.float32)
    tp = taps.ctypes.data_as(C.c_void_p)
    out = C.c_void_p(1)

    def create(l, m, t, nums, dens, k=None, taps_p=tp, out_p=None):
        num, den = np.array(nums, dtype=np.int32), np.array(dens, dtype=np.int32)
        out.value = 1
        rc = L.p25fe_tuner_create(None, l, m, t, taps_p, len(nums) if k is None else k, num.ctypes.data_as(C.c_void_p),
                                  den.ctypes.data_as(C.c_void_p), C.byref(out) if out_p is None else out_p)
        return rc
    one = ([1] * 257, [200] * 257)
    assert create(12, 125, 84, *one, k=0) == lib.ERR_ARG and not out.value
    assert create(12, 125, 84, *one, k=257) == lib.ERR_ARG and not out.value
    assert create(12, 125, 84, *one, k=-1) == lib.ERR_ARG
    for num, den in ((1, 0), (1, 8193), (0, -1), (2, 4), (0, 2), (0, 200), (3, 5), (-3, 5), (101, 200), (-(1 << 31), 8192), (6, 9)):
        assert create(12, 125, 84, [0, num], [1, den]) == lib.ERR_ARG, (num, den)
        assert not out.value
    for (l, m, t) in ((2, 4, 8), (10, 10, 8), (8, 125, 513), (0, 10, 8), (33, 34, 8), (1, 1025, 8), (1, 10, 0), (1, 10, 1025)):
        assert create(l, m, t, [1], [200]) == lib.ERR_ARG, (l, m, t)
    bad = np.zeros(12 * 84, dtype=np.float32)
    bad[77] = np.nan
    assert create(12, 125, 84, [1], [200], taps_p=bad.ctypes.data_as(C.c_void_p)) == lib.ERR_ARG
    assert create(12, 125, 84, [1], [200], taps_p=None) == lib.ERR_ARG
    assert create(12, 125, 84, [1], [200], out_p=None) == lib.ERR_ARG               # everything right but the handle
    num = np.array([1], dtype=np.int32)
    assert L.p25fe_tuner_create(None, 12, 125, 84, tp, 1, None, num.ctypes.data_as(C.c_void_p), C.byref(out)) == lib.ERR_ARG
    assert L.p25fe_tuner_create(None, 12, 125, 84, tp, 1, num.ctypes.data_as(C.c_void_p), None, C.byref(out)) == lib.ERR_ARG
    assert L.p25fe_tuner_create(None, 12, 125, 84, tp, 1, num.ctypes.data_as(C.c_void_p), num.ctypes.data_as(C.c_void_p), None) == lib.ERR_ARG
    assert L.p25fe_tuner_reset(None) == lib.ERR_ARG
    L.p25fe_tuner_destroy(None)                                      # a no-op
    n_out = C.c_size_t(0)
    assert L.p25fe_tune(None, None, 0, 0, None, 0, C.byref(n_out)) == lib.ERR_ARG
    assert L.p25fe_tune_dev(None, None, 0, 0, 0, 0, None, 0, None) == lib.ERR_ARG


def _design(lib, fs):
    from p25rx_amd.frontend import Resampler
    return Resampler.design(fs)


def _unit_noise(rng, n):
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return (x / np.abs(x).max()).astype(np.complex64)


@pytest.mark.parametrize("fs,n", [(2500000, 60000), (2048000, 50000), (3000000, 40000), (10000000, 20000)])
def test_model_against_double(lib, fs, n):
    """the fp32 model against 3.0c's formula in double (exact rotator), designed tables, unit-peak noise: SPEC 3.11's constant.
    Measured: see docs/SPEC.md 3.0c (the ratios are printed)."""
    L = lib.load()
    l, m, t, taps = _design(lib, fs)
    x = _unit_noise(np.random.default_rng(fs % 1000 + 3), n)
    hsum = max(np.abs(taps[p::l].astype(np.float64)).sum() for p in range(l))
    for ffs, off, num, den in FREQS:
        c, s = _rot(L, den)
        y = TM.tune(x, l, m, t, taps, num, den, c, s)
        ref = TM.tune_double(x, l, m, t, taps, num, den)
        err = np.abs(y.astype(np.complex128) - ref).max()
        print("fs %d %d/%d: max error %.3e = %.3e of the tap sum %.4f" % (fs, num, den, err, err / hsum, hsum))
        assert len(y) == len(ref) == RM.n_resample(l, m, 0, n) >= 480
        assert err <= 2e-6 * hsum, (fs, num, den, err / hsum)


def test_model_properties(lib):
    """num = 0 is the resampler's model bit for bit, exact zeros in the input included; a shift of the stream by lcm(M, den) samples
    reproduces the bits"""
    L = lib.load()
    l, m, t = 12, 125, 84
    rng = np.random.default_rng(5)
    taps = (rng.standard_normal(l * t) * 0.1).astype(np.float32)
    i16 = rng.integers(-3, 4, size=(30001, 2)).astype(np.int16)      # many exact zeros
    x = (i16[:, 0] * np.float32(2.0 ** -15) + 1j * (i16[:, 1] * np.float32(2.0 ** -15))).astype(np.complex64)
    assert (x.real == 0).sum() > 3000
    c1, s1 = _rot(L, 1)
    y0, r0 = TM.tune(x, l, m, t, taps, 0, 1, c1, s1), RM.resample(x, l, m, t, taps)
    assert np.array_equal(y0.view(np.uint32), r0.view(np.uint32))
    x = _unit_noise(rng, 30001)
    for num, den in ((11, 200), (-825, 4096)):
        c, s = _rot(L, den)
        period = m * den // gcd(m, den)
        y = TM.tune(x, l, m, t, taps, num, den, c, s)
        ys = TM.tune(np.concatenate([np.zeros(period, dtype=np.complex64), x]), l, m, t, taps, num, den, c, s)
        k = period * l // m
        assert np.array_equal(ys[k:].view(np.uint32), y.view(np.uint32)), (num, den)
        # ... and one that is a multiple of M alone does not
        ym = TM.tune(np.concatenate([np.zeros(m, dtype=np.complex64), x]), l, m, t, taps, num, den, c, s)
        assert not np.array_equal(ym[l:].view(np.uint32), y.view(np.uint32)), (num, den)


@pytest.mark.parametrize("fs,up,down,offsets", [(2500000, 125, 12, (-412500, 137500, 150000, 0)),
                                                (2048000, 128, 15, (-600000, 12500, 25000))])
def test_model_end_to_end(lib, fs, up, down, offsets):
    """the reference decodes the end-to-end case of tests/test_gpu_tune.py without a symbol error: C4FM sources at the offsets
    (adjacent 12.5 kHz channels among them) in one capture, the designed table, the model's rows, the oracle's receive chain"""
    from oracle import oracle as O
    L = lib.load()
    wide, truths = TM.site_capture(fs, up, down, offsets)
    l, m, t, taps = _design(lib, fs)
    assert (l, m) == (down, up)
    for off, truth in zip(offsets, truths):
        rc, num, den = _freq(L, fs, off)
        assert rc == lib.OK
        c, s = _rot(L, den)
        dib = O.run_cf32(TM.tune(wide, l, m, t, taps, num, den, c, s))
        k = min(len(dib), len(truth) - 24)
        errs = int(np.count_nonzero(dib[:k] != truth[24:24 + k]))
        print("fs %d offset %d: %d errors in %d symbols" % (fs, off, errs, k))
        assert k > 1100 and errs == 0, (off, errs, k)
