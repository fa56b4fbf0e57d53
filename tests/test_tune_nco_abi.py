"""CPU tests of the host side of the tuner's NCO channels (docs/SPEC.md 3.0d): the ABI surface, p25fe_nco_step, p25fe_nco_factor
against the numpy model (tests/tune_nco_model.py) bit for bit, the argument checks that need no device, and the model against the
rational tuner's model where the two coincide, against the formula in double precision and against itself.  The GPU side is
tests/test_gpu_tune_nco.py."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import resample_model as RM
import tune_model as TM
import tune_nco_model as NM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"p25fe_nco_step", "p25fe_nco_factor", "p25fe_nco_create"}
RATES = (960000, 1024000, 1200000, 1920000, 2000000, 2048000, 2400000, 2500000, 2880000, 3000000, 3200000, 5000000, 8000000,
         10000000, 12500000, 20000000)
# raster offsets and offsets off it: a crystal's few ppm at 850 MHz, fractions of a hertz, a sixth of the rate's resolution
OFFSETS = (0.0, 12500.0, -12500.0, 137500.0, -412500.0, 1871.3, -2210.7, 135289.3, -410628.7, 733.1, 0.001, -0.25, 406250.0 + 1e-3)
EDGE_STEPS = (0, 1, -1, 0x7fffffff, -(1 << 31), 1 << 24, -(1 << 24), 11 << 24, -37 << 24, 127 << 24, 64 << 24, 232387521, -3527459)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from p25rx_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def rot(lib):
    L = lib.load()
    cs = np.full(512, np.float32(np.nan), dtype=np.float32)
    assert L.p25fe_tuner_rotator(256, cs.ctypes.data_as(C.c_void_p), cs.size) == 0
    return cs[:256].copy(), cs[256:].copy()


def _step(L, fs, off):
    st = C.c_int32(-7)
    return L.p25fe_nco_step(fs, off, C.byref(st)), st.value


def _wrap(q):
    return (int(q) + (1 << 31)) % (1 << 32) - (1 << 31)


def test_abi_surface(lib):
    """header, ctypes and the Rust text name the same three functions; the object is p25fe_tuner_t; the ABI version has not moved"""
    hdr = open(os.path.join(ROOT, "include", "p25fe.h")).read()
    assert re.search(r"#define P25FE_ABI_VERSION 6\b", hdr) and lib.ABI_VERSION == 6
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(p25fe_[a-z0-9_]+)\s*\(", code))
    assert NEW <= declared and NEW <= set(lib.SYMBOLS)
    assert {s for s in declared if "nco" in s} == NEW
    rs = open(os.path.join(ROOT, "bindings", "p25fe.rs")).read()
    assert NEW <= set(re.findall(r"pub fn (p25fe_[a-z0-9_]+)\(", rs))
    L = lib.load()
    for s in NEW:
        assert getattr(L, s).argtypes is not None, s
    assert L.p25fe_nco_step.argtypes[1] is C.c_double and L.p25fe_nco_factor.argtypes[1] is C.c_uint64
    assert re.search(r"p25fe_nco_create\([^)]*p25fe_tuner_t \*\*out\)", code)
    m = re.search(r"pub fn p25fe_nco_create\(([^)]*)\)", rs)
    assert [p.strip() for p in m.group(1).split(",")][-1] == "out: *mut *mut Tuner"


def test_step(lib):
    """nearbyint(offset / fs * 2^32) in double, ties to even, wrapped to 32 bits; the frequency it stands for is within half a
    resolution step, fs / 2^33, of the one asked for"""
    L = lib.load()
    for fs in RATES:
        for off in OFFSETS + (fs / 2.0, -fs / 2.0, fs / 4.0, fs / 2.0 ** 33, 3 * fs / 2.0 ** 33, -fs / 2.0 ** 33, -3 * fs / 2.0 ** 33):
            rc, st = _step(L, fs, off)
            want = _wrap(np.rint(math.ldexp(off / fs, 32)))
            assert (rc, st) == (lib.OK, want), (fs, off, st, want)
            # the round trip, exactly: the step as it was before wrapping stands for a frequency within fs / 2^33 of the offset
            unwrapped = st + (1 << 32) if (st == -(1 << 31) and off > 0) else st
            assert abs(Fraction(unwrapped) * fs / (1 << 32) - Fraction(off)) <= Fraction(fs, 1 << 33), (fs, off, st)
        assert _step(L, fs, fs / 2.0) == (lib.OK, -(1 << 31)) and _step(L, fs, -fs / 2.0) == (lib.OK, -(1 << 31))   # Nyquist
        assert _step(L, fs, fs / 4.0) == (lib.OK, 1 << 30) and _step(L, fs, 0.0) == (lib.OK, 0)
        # ties go to even: 1/2 -> 0, 3/2 -> 2, -1/2 -> 0, -3/2 -> -2 (these offsets and quotients are exact in double)
        assert [_step(L, fs, k * fs / 2.0 ** 33)[1] for k in (1, 3, -1, -3, 5)] == [0, 2, 0, -2, 2]
        for bad in (fs / 2.0 + 0.001, -fs / 2.0 - 0.001, 1e300, -1e300, float("inf"), float("-inf"), float("nan")):
            assert _step(L, fs, bad) == (lib.ERR_ARG, -7), (fs, bad)
    assert _step(L, 2500000, 137500.0) == (lib.OK, 11 * (1 << 32) // 200) and _step(L, 2048000, 8000.0) == (lib.OK, 1 << 24)
    assert _step(L, 0, 0.0)[0] == lib.ERR_ARG and _step(L, 0, 100.0)[0] == lib.ERR_ARG
    assert L.p25fe_nco_step(2500000, 0.0, None) == lib.ERR_ARG


def test_factor_is_the_model(lib, rot):
    """p25fe_nco_factor, the host restatement of the kernel's operations, against the model bit for bit: random (step, n), positions
    around 2^32 and 2^56, the steps at which something changes"""
    L = lib.load()
    rng = np.random.default_rng(11)
    steps = list(EDGE_STEPS) + [int(s) for s in rng.integers(-(1 << 31), 1 << 31, size=40)]
    bases = [0, 12345, (1 << 32) - 40, (1 << 56) - 40, (1 << 40) + 77, (1 << 62) - 100] + [int(b) for b in rng.integers(0, 1 << 62, size=6)]
    cs = np.zeros(2, dtype=np.float32)
    n = 80
    for st in steps:
        for b in bases:
            c, s = NM.factor(st, b, n, *rot)
            for k in (0, 1, 39, 40, 41, n - 1) if st not in EDGE_STEPS[:5] else range(n):
                assert L.p25fe_nco_factor(st, b + k, cs.ctypes.data_as(C.c_void_p)) == lib.OK
                assert cs[0].view(np.uint32) == c[k].view(np.uint32) and cs[1].view(np.uint32) == s[k].view(np.uint32), (st, b, k)
    assert L.p25fe_nco_factor(0, 5, cs.ctypes.data_as(C.c_void_p)) == lib.OK and cs[0] == 1.0 and cs[1] == 0.0
    assert L.p25fe_nco_factor(1, 0, None) == lib.ERR_ARG
    # unit modulus to fp32: c and s each carry at most three roundings of half an ulp (the table's entry, the product, the fma) on
    # values <= 1, 9e-8, and the polynomials' truncation (t^4 / 24 <= 1e-9); |c^2 + s^2 - 1| <= 2 sqrt(2) 9e-8 = 2.6e-7 < 5e-7
    c, s = NM.factor(232387521, 0, 100000, *rot)
    assert np.abs(c.astype(np.float64) ** 2 + s.astype(np.float64) ** 2 - 1.0).max() < 5e-7


def test_is_the_rational_channel(lib, rot):
    """step = num 2^24, num odd, |num| <= 127: the residual is 0 and the mixer IS 3.0c's channel num / 256, bit for bit, at every
    position; step = 0 leaves the samples alone, exact zeros included"""
    rng = np.random.default_rng(12)
    x = (rng.standard_normal(5000) + 1j * rng.standard_normal(5000)).astype(np.complex64)
    x[::7] = 0
    for num in (1, -37, 55, 127, -127, 3, -1):
        for pos in (0, 12345, (1 << 40) + 77, (1 << 32) - 2500):
            a = NM.mix_nco(x, num << 24, pos, *rot)
            b = TM.mix(x, num, 256, *rot, abs0=pos)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (num, pos)
    assert np.array_equal(NM.mix_nco(x, 0, 12345, *rot).view(np.uint32), x.view(np.uint32))
    l, m, t = 12, 125, 84
    taps = (rng.standard_normal(l * t) * 0.1).astype(np.float32)
    assert np.array_equal(NM.tune_nco(x, l, m, t, taps, 0, *rot).view(np.uint32), RM.resample(x, l, m, t, taps).view(np.uint32))


def test_position_grid(lib, rot):
    """the mixer's phase has the period 2^32 / gcd(step, 2^32) in the position, and 2^32 for every step"""
    rng = np.random.default_rng(13)
    x = (rng.standard_normal(3000) + 1j * rng.standard_normal(3000)).astype(np.complex64)
    for st in (232387521, -3527459, 1, 0x7fffffff):
        a = NM.mix_nco(x, st, 977, *rot)
        for q in (1 << 32, 5 << 32, 1 << 56):
            assert np.array_equal(NM.mix_nco(x, st, q + 977, *rot).view(np.uint32), a.view(np.uint32)), (st, q)
        assert not np.array_equal(NM.mix_nco(x, st, 977 + 125, *rot).view(np.uint32), a.view(np.uint32)), st
    st = 3 << 20                                                     # gcd 2^20: the period is 2^12 samples
    a = NM.mix_nco(x, st, 977, *rot)
    assert np.array_equal(NM.mix_nco(x, st, 977 + (1 << 12), *rot).view(np.uint32), a.view(np.uint32))
    assert not np.array_equal(NM.mix_nco(x, st, 977 + (1 << 11), *rot).view(np.uint32), a.view(np.uint32))


def _unit_noise(rng, n):
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return (x / np.abs(x).max()).astype(np.complex64)


@pytest.mark.parametrize("fs,n", [(2500000, 60000), (2048000, 50000), (3000000, 40000), (10000000, 20000)])
def test_model_against_double(lib, rot, fs, n):
    """the fp32 model against 3.0d's formula in double (the exact phasor of the integer phase), designed tables, unit-peak noise:
    SPEC 3.11's constant, as tests/test_tune_abi.py::test_model_against_double asserts it for 3.0c.  Measured: 3.6e-8 to
    8.2e-8 of the tap sum over the four rates; docs/SPEC.md 3.0d records the values (the ratios are printed)."""
    from p25rx_amd.frontend import Resampler, Tuner
    l, m, t, taps = Resampler.design(fs)
    x = _unit_noise(np.random.default_rng(fs % 1000 + 4), n)
    hsum = max(np.abs(taps[p::l].astype(np.float64)).sum() for p in range(l))
    for st in (1, -1, 0x7fffffff, -(1 << 31), Tuner.nco_step(fs, 135289.3), Tuner.nco_step(fs, -410628.7)):
        y = NM.tune_nco(x, l, m, t, taps, st, *rot)
        ref = NM.tune_nco_double(x, l, m, t, taps, st)
        err = np.abs(y.astype(np.complex128) - ref).max()
        print("fs %d step %d: max error %.3e = %.3e of the tap sum %.4f" % (fs, st, err, err / hsum, hsum))
        assert len(y) == len(ref) == RM.n_resample(l, m, 0, n) >= 480
        assert err <= 2e-6 * hsum, (fs, st, err / hsum)


def test_create_checks_its_arguments_before_any_device(lib):
    """p25fe_tuner_create's refusals in its order, with no handle at all; every step value passes them"""
    L = lib.load()
    taps = np.zeros(8192, dtype=np.float32)
    tp = taps.ctypes.data_as(C.c_void_p)
    out = C.c_void_p(1)

    def create(l, m, t, steps, k=None, taps_p=tp, out_p=None):
        st = np.array(steps, dtype=np.int32)
        out.value = 1
        return L.p25fe_nco_create(None, l, m, t, taps_p, len(steps) if k is None else k, st.ctypes.data_as(C.c_void_p),
                                  C.byref(out) if out_p is None else out_p)
    many = [1] * 257
    assert create(12, 125, 84, many, k=0) == lib.ERR_ARG and not out.value
    assert create(12, 125, 84, many, k=257) == lib.ERR_ARG and not out.value
    assert create(12, 125, 84, many, k=-1) == lib.ERR_ARG and not out.value
    for (l, m, t) in ((2, 4, 8), (10, 10, 8), (8, 125, 513), (0, 10, 8), (33, 34, 8), (1, 1025, 8), (1, 10, 0), (1, 10, 1025)):
        assert create(l, m, t, [1]) == lib.ERR_ARG and not out.value, (l, m, t)
    bad = np.zeros(12 * 84, dtype=np.float32)
    bad[77] = np.nan
    assert create(12, 125, 84, [1], taps_p=bad.ctypes.data_as(C.c_void_p)) == lib.ERR_ARG
    assert create(12, 125, 84, [1], taps_p=None) == lib.ERR_ARG
    assert create(12, 125, 84, [1], out_p=None) == lib.ERR_ARG
    assert L.p25fe_nco_create(None, 12, 125, 84, tp, 1, None, C.byref(out)) == lib.ERR_ARG
    # everything right but the handle: no step is refused
    assert create(12, 125, 84, [0, 1, -1, 0x7fffffff, -(1 << 31), 11 << 24]) == lib.ERR_ARG and not out.value
    assert create(12, 125, 84, [5] * 256) == lib.ERR_ARG and not out.value


def test_model_end_to_end(lib, rot):
    """four C4FM sources a crystal's few ppm off the raster in one 2.5 Msps capture: tuned to the nearest raster frequency, as the
    rational tuner must, the reference finds no frame; mixed down by the exact offsets, every row decodes without a symbol error"""
    from oracle import oracle as O
    from p25rx_amd.frontend import Tuner
    fs = 2500000
    offsets = (-412500 + 1871.3, 137500 - 2210.7, 150000 - 2411.6, 733.1)
    wide, truths = TM.site_capture(fs, 125, 12, offsets)
    l, m, t, taps, steps = Tuner.design_nco(fs, offsets)
    assert (l, m, t) == (12, 125, 84)
    for off, st, truth in zip(offsets, steps, truths):
        dib = O.run_cf32(NM.tune_nco(wide, l, m, t, taps, st, *rot))
        k = min(len(dib), len(truth) - 24)
        errs = int(np.count_nonzero(dib[:k] != truth[24:24 + k]))
        print("offset %.1f step %d: %d errors in %d symbols" % (off, st, errs, k))
        assert k > 1100 and errs == 0, (off, errs, k)
        num, den = Tuner.freq(fs, int(round(off / 12500.0)) * 12500)
        c, s = (a.copy() for a in Tuner.rotator(den))
        assert len(O.run_cf32(TM.tune(wide, l, m, t, taps, num, den, c, s))) == 0, off
