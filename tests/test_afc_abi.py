"""CPU tests of the host side of AFC (docs/SPEC.md 3.0e: an NCO channel's phase offset and its step changed in a stream; 3.0f: the
frequency measure): the ABI surface, p25fe_afc_design, p25fe_afc_factor against the numpy model (tests/afc_model.py) bit for bit,
the continuity identity of p25fe_afc_set_step's arithmetic, p25fe_afc_hz, every refusal that needs no device, and the model end to
end on a capture whose channels are a crystal's few ppm off the raster.  The GPU side is tests/test_gpu_afc.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import afc_model as AM
import tune_model as TM
import tune_nco_model as NM
from test_tune_nco_abi import EDGE_STEPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"p25fe_afc_set_step", "p25fe_afc_get_step", "p25fe_afc_factor", "p25fe_afc_design", "p25fe_afc_create", "p25fe_afc_destroy",
       "p25fe_afc_measure_dev", "p25fe_afc_hz"}
MASK = (1 << 32) - 1


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


def _factor(L, step, ph0, n):
    cs = np.zeros(2, dtype=np.float32)
    assert L.p25fe_afc_factor(step, ph0, n, cs.ctypes.data_as(C.c_void_p)) == 0
    return int(cs[0].view(np.uint32)), int(cs[1].view(np.uint32))


def test_abi_surface(lib):
    """header, ctypes and the Rust text name the same eight functions, none of which carries one of the substrings the older ABI
    tests pin; the record is 32 bytes everywhere; the ABI version has not moved"""
    hdr = open(os.path.join(ROOT, "include", "p25fe.h")).read()
    assert re.search(r"#define P25FE_ABI_VERSION 6\b", hdr) and lib.ABI_VERSION == 6
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(p25fe_[a-z0-9_]+)\s*\(", code))
    assert {s for s in declared if s.startswith("p25fe_afc_")} == NEW and NEW <= set(lib.SYMBOLS)
    assert not [s for s in NEW if "nco" in s or "tune" in s or "resampl" in s]
    rs = open(os.path.join(ROOT, "bindings", "p25fe.rs")).read()
    assert NEW <= set(re.findall(r"pub fn (p25fe_[a-z0-9_]+)\(", rs))
    L = lib.load()
    for s in NEW:
        assert hasattr(L, s) and getattr(L, s).argtypes is not None, s
    assert L.p25fe_afc_set_step.argtypes[3] is C.c_uint64 and L.p25fe_afc_factor.argtypes[1] is C.c_uint32
    assert lib.AFC_ACC_DTYPE.itemsize == 32 and lib.AFC_ACC_DTYPE.names == ("re", "im", "pow", "n")
    m = re.search(r"typedef struct p25fe_afc_acc \{(.*?)\} p25fe_afc_acc_t;", code, re.S)
    assert re.sub(r"\s+", " ", m.group(1)).strip() == "int64_t re, im; int64_t pow; uint64_t n;"
    m = re.search(r"pub struct AfcAcc \{(.*?)\}", rs, re.S)
    assert re.sub(r"\s+", " ", m.group(1)).strip() == "pub re: i64, pub im: i64, pub pow: i64, pub n: u64,"
    for name, val in (("MIN_D", 2), ("MAX_D", 64), ("MAX_T", 512), ("MAX_CH", 256), ("MAX_SHIFT", 40)):
        assert re.search(r"#define P25FE_AFC_%s %d\b" % (name, val), hdr) and getattr(lib, "AFC_" + name) == val
        assert re.search(r"pub const AFC_%s: i32 = %d;" % (name, val), rs)


def test_design(lib):
    """Kaiser(7)-windowed sinc of T points with the given cutoff at 240 ksps, sum 1, evaluated in double and rounded once: against
    numpy's kaiser and sinc to half an ulp of the largest tap plus the two libms' last bits (1e-9 of the largest tap)"""
    L = lib.load()
    from p25rx_amd.frontend import Afc
    for D, T, fc in ((10, 240, 7000.0), (3, 7, 30000.0), (64, 512, 1500.0), (2, 1, 7000.0), (10, 241, 6250.0), (5, 2, 120000.0)):
        taps = Afc.design(D, T, fc)
        ref = AM.design(D, fc, T)
        assert taps.dtype == np.float32 and taps.shape == (T,)
        assert abs(float(taps.astype(np.float64).sum()) - 1.0) < T * 2.0 ** -25
        assert np.abs(taps.astype(np.float64) - ref).max() <= np.abs(ref).max() * (2.0 ** -24 + 1e-9), (D, T, fc)
        assert np.array_equal(taps, taps[::-1])                      # linear phase
    buf = np.full(8, np.float32(-3.0))
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.p25fe_afc_design(10, 7000.0, 8, p, 7) == lib.ERR_CAPACITY and (buf == -3.0).all()
    assert L.p25fe_afc_design(10, 7000.0, 8, None, 8) == lib.ERR_CAPACITY
    for D, T in ((1, 8), (65, 8), (0, 8), (-1, 8), (10, 0), (10, 513), (10, -1)):
        assert L.p25fe_afc_design(D, 7000.0, T, p, 8) == lib.ERR_ARG, (D, T)
    for fc in (0.0, -1.0, 120000.5, float("inf"), float("-inf"), float("nan"), 1e300):
        assert L.p25fe_afc_design(10, fc, 8, p, 8) == lib.ERR_ARG, fc
    assert (buf == -3.0).all()
    assert L.p25fe_afc_design(10, 120000.0, 8, p, 8) == lib.OK


def test_factor_is_the_model(lib, rot):
    """p25fe_afc_factor against the model bit for bit: the steps at which something changes x offsets x positions past 2^32; ph0 = 0
    is p25fe_nco_factor"""
    L = lib.load()
    rng = np.random.default_rng(21)
    steps = list(EDGE_STEPS) + [int(s) for s in rng.integers(-(1 << 31), 1 << 31, size=12)]
    offs = [0, 1, MASK, 1 << 31, (1 << 23) - 1, 1 << 23, 0x12345678] + [int(v) for v in rng.integers(0, 1 << 32, size=5)]
    bases = [0, 12345, (1 << 32) - 3, (1 << 32) + 77, (1 << 40) + 3, (1 << 56) - 3, (1 << 62) - 7]
    n = 6
    for st in steps:
        for ph0 in offs:
            for b in bases:
                c, s = AM.factor(st, ph0, b, n, *rot)
                for k in range(n):
                    assert _factor(L, st, ph0, b + k) == (int(c[k].view(np.uint32)), int(s[k].view(np.uint32))), (st, ph0, b, k)
    cs = np.zeros(2, dtype=np.float32)
    for st in steps:
        for b in bases:
            assert L.p25fe_nco_factor(st, b, cs.ctypes.data_as(C.c_void_p)) == 0
            assert _factor(L, st, 0, b) == (int(cs[0].view(np.uint32)), int(cs[1].view(np.uint32)))
    assert _factor(L, 0, 0, 5) == (int(np.float32(1.0).view(np.uint32)), 0)
    assert _factor(L, 0, 1 << 30, 5)[1] == int(np.float32(1.0).view(np.uint32))       # step 0 with an offset still turns: a quarter
    assert L.p25fe_afc_factor(1, 0, 0, None) == lib.ERR_ARG
    # the model with ph0 = 0 is 3.0d's
    x = (rng.standard_normal(500) + 1j * rng.standard_normal(500)).astype(np.complex64)
    for st in (232387521, 0, -3527459):
        a, b = AM.mix_nco(x, st, 0, (1 << 40) + 3, *rot), NM.mix_nco(x, st, (1 << 40) + 3, *rot)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_continuity_identity(lib):
    """for random (step, ph0, step', abs_at) the factor at abs_at is bit-identical before and after set_step's arithmetic; abs_at
    includes values at and above 2^32 and 2^56; the sample after abs_at differs when the steps do"""
    L = lib.load()
    rng = np.random.default_rng(22)
    ats = [0, 1, 125000, (1 << 32) - 1, 1 << 32, (1 << 32) + 77, (1 << 40) + 3, 1 << 56, (1 << 56) + 12345, (1 << 62) - 1]
    ats += [int(v) for v in rng.integers(0, 1 << 62, size=10)]
    for i in range(400):
        st, st2 = (int(v) for v in rng.integers(-(1 << 31), 1 << 31, size=2))
        if i < len(EDGE_STEPS):
            st2 = EDGE_STEPS[i]
        ph0 = int(rng.integers(0, 1 << 32)) if i % 3 else 0
        at = ats[i % len(ats)]
        new_step, new_ph0 = AM.set_step(st, ph0, st2, at)
        assert new_step == st2 and 0 <= new_ph0 <= MASK
        assert (new_ph0 + (st2 & MASK) * at) & MASK == (ph0 + (st & MASK) * at) & MASK
        assert _factor(L, st, ph0, at) == _factor(L, st2, new_ph0, at), (st, ph0, st2, at)
        if (st - st2) & MASK:
            d = ((st - st2) & MASK)
            assert ((ph0 + (st & MASK) * (at + 1)) - (new_ph0 + (st2 & MASK) * (at + 1))) & MASK == d
    # two changes compose: back to the first step at the same index gives the first offset back
    s1, p1 = AM.set_step(232387521, 0, -3527459, (1 << 40) + 3)
    assert AM.set_step(s1, p1, 232387521, (1 << 40) + 3) == (232387521, 0)


def test_hz(lib):
    """p25fe_afc_hz on hand-made records against Python's math.atan2 and math.hypot (1e-12 relative: two libms)"""
    L = lib.load()
    from p25rx_amd.frontend import Afc
    recs = [(1000, 0, 1000, 5), (0, 1000, 1000, 5), (-1000, 0, 1000, 5), (0, -1000, 2000, 5), (-1000, -1, 1000, 5), (-1000, 1, 1000, 5),
            (123456789, -987654321, 1 << 40, 77), ((1 << 62) + 12345, -(1 << 61), (1 << 63) - 1, 1 << 40), (3, 4, 5, 1),
            (-(1 << 63), (1 << 63) - 1, 1, 1)]
    for rec in recs:
        for D in (2, 10, 64):
            hz, coh = Afc.hz(rec, D)
            want = math.atan2(float(rec[1]), float(rec[0])) / (2.0 * math.pi) * 240000.0 / D
            assert hz == pytest.approx(want, rel=1e-12, abs=0.0), (rec, D)
            assert coh == pytest.approx(math.hypot(float(rec[0]), float(rec[1])) / float(rec[2]), rel=1e-12), (rec, D)
            assert abs(hz) <= 120000.0 / D
            assert (hz, coh) == pytest.approx(AM.hz(rec, D), rel=1e-12)
    assert Afc.hz((0, 1000, 1000, 5), 10)[0] == pytest.approx(6000.0, rel=1e-12)
    assert Afc.hz((3, 4, 5, 1), 10)[1] == pytest.approx(1.0, rel=1e-12)
    for rec in ((1000, 1000, 0, 5), (1000, -1000, -1, 5), (0, 0, 0, 0)):
        assert Afc.hz(rec, 10) == (0.0, 0.0)                         # pow <= 0
    assert Afc.hz((0, 0, 1000, 5), 10) == (0.0, 0.0)                 # re = im = 0
    rec = np.zeros(1, dtype=lib.AFC_ACC_DTYPE)
    hz, coh = C.c_double(-1.0), C.c_double(-1.0)
    p = rec.ctypes.data_as(C.c_void_p)
    assert L.p25fe_afc_hz(None, 10, C.byref(hz), C.byref(coh)) == lib.ERR_ARG
    assert L.p25fe_afc_hz(p, 10, None, C.byref(coh)) == lib.ERR_ARG and L.p25fe_afc_hz(p, 10, C.byref(hz), None) == lib.ERR_ARG
    for D in (1, 0, -1, 65):
        assert L.p25fe_afc_hz(p, D, C.byref(hz), C.byref(coh)) == lib.ERR_ARG
    assert (hz.value, coh.value) == (-1.0, -1.0)


def test_refusals_need_no_device(lib):
    """every refusal of create, measure and set_step / get_step, with no handle and no object"""
    L = lib.load()
    taps = np.full(512, np.float32(0.01))
    tp = taps.ctypes.data_as(C.c_void_p)
    out = C.c_void_p(1)

    def create(D, T, K, taps_p=tp, out_p=None):
        out.value = 1
        return L.p25fe_afc_create(None, D, T, taps_p, K, C.byref(out) if out_p is None else out_p)
    for D, T, K in ((1, 240, 1), (65, 240, 1), (0, 240, 1), (-5, 240, 1), (10, 0, 1), (10, 513, 1), (10, -1, 1), (10, 240, 0), (10, 240, 257),
                    (10, 240, -1), (2147483647, 240, 1), (10, 2147483647, 1), (10, 240, 2147483647)):
        assert create(D, T, K) == lib.ERR_ARG and not out.value, (D, T, K)
    bad = np.array(taps[:240])
    for v in (np.nan, np.inf, -np.inf):
        bad[239] = v                                                 # the LAST tap: the check reads exactly T of them
        assert create(10, 240, 1, taps_p=bad.ctypes.data_as(C.c_void_p)) == lib.ERR_ARG and not out.value
    assert create(10, 240, 1, taps_p=None) == lib.ERR_ARG and not out.value
    assert L.p25fe_afc_create(None, 10, 240, tp, 1, None) == lib.ERR_ARG
    for D, T, K in ((10, 240, 4), (2, 1, 1), (64, 512, 256)):        # everything right but the handle
        assert create(D, T, K) == lib.ERR_ARG and not out.value
    L.p25fe_afc_destroy(None)                                        # a no-op
    rec = np.zeros(4, dtype=lib.AFC_ACC_DTYPE)
    assert L.p25fe_afc_measure_dev(None, tp, 100, 0, 100, 0, 24, rec.ctypes.data_as(C.c_void_p), None) == lib.ERR_ARG
    step, ph0 = C.c_int32(-7), C.c_uint32(7)
    assert L.p25fe_afc_set_step(None, 0, 5, 0, None) == lib.ERR_ARG
    assert L.p25fe_afc_get_step(None, 0, C.byref(step), C.byref(ph0)) == lib.ERR_ARG and (step.value, ph0.value) == (-7, 7)


E_FS, E_OFFSETS = 2500000, (-412500 + 1871.3, 137500 - 2210.7, 150000 - 2411.6, 733.1)


def test_model_end_to_end(lib, rot):
    """tests/tune_model.py's site capture (four sources a crystal's few ppm off the raster, two of them 12.5 kHz apart) tuned at the
    raster frequencies; the default prefilter (D 10, T 240, cutoff 7 kHz) at shift 24.  Every estimate, from the whole capture AND
    from the first 1200 decimated samples (50 ms), lies within 150 Hz of the true error: the double-precision restatement found 71
    and 59 Hz, and the receive chain tolerates a residual of 600 Hz (lost at 800 Hz), four times the bound.  Then the stream is
    retuned through the model's set_step by the 50 ms estimate: range [0, 125000) at the raster step, abs_at = 125000, the second
    range with history.  The retuned rows decode with 0 symbol errors -- the second range on its own and behind the first (the
    frame sync inside it, 304 symbols to the end), and the whole capture at the corrected (step, ph0) (> 1100 symbols); the rows at
    the raster decode nothing."""
    from oracle import oracle as O
    from p25rx_amd.frontend import Afc, Tuner
    wide, truths = TM.site_capture(E_FS, 125, 12, E_OFFSETS)
    raster = [int(round(o / 12500.0)) * 12500 for o in E_OFFSETS]
    l, m, t, taps, steps = Tuner.design_nco(E_FS, raster)
    assert (l, m, t) == (12, 125, 84)
    D, T, fc = Afc.DEFAULT
    g = Afc.design(D, T, fc)
    cut_in, cut_out = 125000, 125000 * l // m
    assert cut_out == 12000 == 1200 * D
    for k, (off, f0, st, truth) in enumerate(zip(E_OFFSETS, raster, steps, truths)):
        row = NM.tune_nco(wide, l, m, t, taps, st, *rot)
        assert len(O.run_cf32(row)) == 0, off                        # uncorrected: no frame
        prod = AM.products(row, D, T, g, 24)
        whole, head = AM.record(prod), AM.record(prod, 0, 1200)
        assert whole[3] == len(row) // D and head[3] == 1200
        true_err = off - f0
        est_whole, coh_w = AM.hz(whole, D)
        est_head, coh_h = AM.hz(head, D)
        dbl = AM.hz_double(row, D, g)
        print("offset %.1f: true error %.1f Hz, whole %.1f (coherence %.3f), first 50 ms %.1f (%.3f), double %.1f"
              % (off, true_err, est_whole, coh_w, est_head, coh_h, dbl))
        assert abs(est_whole - true_err) <= 150.0 and abs(est_head - true_err) <= 150.0, (off, est_whole, est_head)
        assert abs(est_whole - dbl) < 1.0                            # the integer sums lose nothing that matters
        # retune in the stream
        new_step, new_ph0 = AM.set_step(st, 0, st + Tuner.nco_step(E_FS, est_head), cut_in)
        fixed = AM.tune(wide, l, m, t, taps, new_step, new_ph0, *rot)   # every window mixed with the new numbers: the second range is its tail
        dib = O.run_cf32(fixed)
        kk = min(len(dib), len(truth) - 24)
        errs = int(np.count_nonzero(dib[:kk] != truth[24:24 + kk]))
        print("    whole capture at the corrected step: %d errors in %d symbols" % (errs, kk))
        assert kk > 1100 and errs == 0, (off, errs, kk)
        for what, stream in (("second range", fixed[cut_out:]), ("both ranges", np.concatenate([row[:cut_out], fixed[cut_out:]]))):
            dib = O.run_cf32(stream)
            kk = min(len(dib), len(truth) - 888)
            errs = int(np.count_nonzero(dib[:kk] != truth[888:888 + kk]))
            print("    %s: %d errors in %d symbols" % (what, errs, kk))
            assert kk >= 290 and errs == 0, (off, what, errs, kk)
