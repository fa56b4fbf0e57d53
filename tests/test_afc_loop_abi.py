"""CPU tests of the AFC loop (docs/SPEC.md 3.0g): the ABI surface, p25fe_track_step against the integer model
(tests/afc_loop_model.py) field for field, the CORDIC angle against math.atan2 within the SPEC's bound, the arctangent table against
its formula, every refusal that needs no device, and the model end to end on a capture whose carrier drifts.  The GPU side is
tests/test_gpu_afc_loop.py.

The C names are p25fe_track_*: tests/test_afc_abi.py pins the set of names that begin with p25fe_afc_, and tests/test_tune_abi.py
the set of names that contain "tune"."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import afc_loop_model as LM
import afc_model as AM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"p25fe_track_create", "p25fe_track_destroy", "p25fe_track_records", "p25fe_track_measure_dev", "p25fe_track_update_dev",
       "p25fe_track_run_dev", "p25fe_track_read", "p25fe_track_step", "p25fe_track_hz"}
MASK = (1 << 32) - 1
I64 = (1 << 63) - 1
ANGLE_BOUND = 1.0          # units of 2^-32 turn: SPEC 3.0g's bound for 32 iterations (the issue's condition: no looser than 2^-20 turn)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from p25rx_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def rot(lib):
    L = lib.load()
    cs = np.zeros(512, dtype=np.float32)
    assert L.p25fe_tuner_rotator(256, cs.ctypes.data_as(C.c_void_p), cs.size) == 0
    return cs[:256].copy(), cs[256:].copy()


def _cfg(lib, **kw):
    from p25rx_amd.frontend import AfcLoop
    return AfcLoop.config(**kw)


def _c_step(lib, cfg, L, M, D, step_ref, acc, st, abs_at):
    """p25fe_track_step -> (acc as a tuple of Python integers, state as the model's dict)"""
    from p25rx_amd.frontend import AfcLoop
    a, s = AfcLoop.step(cfg, L, M, D, step_ref, acc, st, abs_at)
    return tuple(int(v) for v in a), {f: int(s[f]) for f in LM.STATE_FIELDS}


def test_abi_surface(lib):
    """header, ctypes and the Rust text name the same nine functions; the three records are 32 bytes everywhere; ABI version 6"""
    hdr = open(os.path.join(ROOT, "include", "p25fe.h")).read()
    assert re.search(r"#define P25FE_ABI_VERSION 6\b", hdr) and lib.ABI_VERSION == 6
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(p25fe_[a-z0-9_]+)\s*\(", code))
    assert {s for s in declared if s.startswith("p25fe_track_")} == NEW and NEW <= set(lib.SYMBOLS)
    rs = open(os.path.join(ROOT, "bindings", "p25fe.rs")).read()
    assert NEW <= set(re.findall(r"pub fn (p25fe_[a-z0-9_]+)\(", rs))
    L = lib.load()
    for s in NEW:
        assert hasattr(L, s) and getattr(L, s).argtypes is not None, s
    assert L.p25fe_track_update_dev.argtypes[1] is C.c_uint64 and L.p25fe_track_run_dev.argtypes[6] is C.c_uint64
    assert lib.TRACK_CFG_DTYPE.itemsize == 32 and lib.TRACK_STATE_DTYPE.itemsize == 32
    assert lib.TRACK_STATE_DTYPE.names == LM.STATE_FIELDS
    m = re.search(r"typedef struct p25fe_track_state \{(.*?)\} p25fe_track_state_t;", code, re.S)
    assert re.sub(r"\s+", " ", m.group(1)).strip() == ("int32_t step; uint32_t ph0; int32_t last_theta; int32_t last_dstep; "
                                                       "uint32_t n_applied, n_rejected, n_short; uint32_t status;")
    m = re.search(r"typedef struct p25fe_track_cfg \{(.*?)\} p25fe_track_cfg_t;", code, re.S)
    assert re.findall(r"(\w+);", m.group(1)) == list(lib.TRACK_CFG_DTYPE.names)
    m = re.search(r"pub struct TrackState \{(.*?)\}", rs, re.S)
    assert re.findall(r"pub (\w+): (\w+),", m.group(1)) == [(n, {"<i4": "i32", "<u4": "u32"}[lib.TRACK_STATE_DTYPE[n].str])
                                                            for n in LM.STATE_FIELDS]
    m = re.search(r"pub struct TrackCfg \{(.*?)\}", rs, re.S)
    assert [n for n, _ in re.findall(r"pub (\w+): (\w+),", m.group(1))] == list(lib.TRACK_CFG_DTYPE.names)
    for name, val in (("NONE", 0), ("SHORT", 1), ("REJECT", 2), ("APPLY", 3)):
        assert re.search(r"#define P25FE_TRACK_%s\s+%d\b" % (name, val), hdr) and getattr(lib, "TRACK_" + name) == val
        assert re.search(r"pub const TRACK_%s: u32 = %d;" % (name, val), rs) and getattr(LM, name) == val


def test_table_constants():
    """P25FE_AFC_CORDIC_ATAN[i] = round(atan(2^-i) / (2 pi) 2^48): against exact rational arithmetic (the model's), and against
    libm's atan to the one unit double precision can decide at 46 bits"""
    spec = open(os.path.join(ROOT, "include", "p25fe_spec.h")).read()
    for name, val in (("N", LM.CORDIC_N), ("NORM", LM.CORDIC_NORM), ("FRAC", LM.CORDIC_FRAC)):
        assert re.search(r"#define P25FE_AFC_CORDIC_%s %d\b" % (name, val), spec)
    m = re.search(r"P25FE_AFC_CORDIC_ATAN\[(\d+)\] = \{(.*?)\};", spec, re.S)
    vals = [int(v) for v in re.findall(r"(\d+)LL", m.group(2))]
    assert int(m.group(1)) == 32 == len(vals) and vals == LM.atan_table() == LM.ATAN
    assert vals[0] == 1 << 45                                        # an eighth of a turn, exactly
    for i, v in enumerate(vals):
        assert abs(v - math.atan(2.0 ** -i) / (2.0 * math.pi) * 2.0 ** 48) <= 0.5 + 2.0 ** -6, i
    assert sum(vals) > (1 << 46) * 1.1                               # the iterations reach past a quarter turn (99.88 degrees)


def _records(rng):
    """(re, im, pow, n) that the law's branches and the arithmetic's edges depend on"""
    recs = [(0, 0, 0, 0), (0, 0, 0, 5000), (0, 0, 1000, 5000), (1000, 0, 1000, 599), (1000, 0, 1000, 600), (1000, 5, 0, 5000),
            (1000, 5, -1, 5000), (1000, 5, -I64 - 1, 5000), (-I64 - 1, -I64 - 1, I64, 1 << 40), (I64, -I64 - 1, I64, (1 << 64) - 1),
            (3, 4, 5, 600), (3, 4, 7, 600), (-1, 0, 1, 600), (1, 0, 1, 600), (0, 1, 1, 600), (0, -1, 1, 600)]
    # coherence just under and just over the gate 24576 / 32768 = 3 / 4, small (exact) and large (shifted) magnitudes
    for s in (0, 10, 30, 46):
        recs += [(3000 << s, 0, 4000 << s, 700), (2999 << s, 0, 4000 << s, 700), (3001 << s, 0, 4000 << s, 700),
                 (0, -(3000 << s), (4000 << s) + (1 << s), 700), (-(2122 << s), 2122 << s, 4000 << s, 700), (2121 << s, 2121 << s, 4000 << s, 700)]
    # the axes and diagonals at magnitudes 1 .. 2^62, either sign
    for b in (0, 1, 15, 16, 17, 31, 32, 47, 59, 60, 61, 62):
        v = 1 << b
        for re, im in ((v, 0), (-v, 0), (0, v), (0, -v), (v, v), (-v, v), (v, -v), (-v, -v), (v, 1), (-v, 1), (-v, -1), (1, v), (1, -v)):
            recs.append((re, im, max(abs(re), abs(im)), 1200))
    for _ in range(300):
        b = int(rng.integers(1, 63))
        re, im = (int(v) for v in rng.integers(-(1 << b), 1 << b, size=2))
        recs.append((re, im, int(rng.integers(1, 1 << b)) + max(abs(re), abs(im)) // 2, int(rng.integers(0, 3000))))
    return recs


def test_step_is_the_model(lib):
    """p25fe_track_step equals the model field for field: the seeded records x positions whose low 32 bits alone may matter x
    steps near +-2^31 x configurations in which each clamp bites.  The factor at abs_at (p25fe_afc_factor) is the same bits
    before and after every update."""
    L = lib.load()
    rng = np.random.default_rng(31)
    recs = _records(rng)
    ats = [0, MASK, 1 << 32, (1 << 40) + 5]
    cfgs = [dict(LM.RECOMMENDED), dict(LM.RECOMMENDED, max_pull=100), dict(LM.RECOMMENDED, max_dev=1000),
            dict(LM.RECOMMENDED, gain_q16=32768, coh_min_q15=0), dict(LM.RECOMMENDED, gain_q16=1, coh_min_q15=32768, min_products=1),
            dict(LM.RECOMMENDED, shift=0, max_pull=(1 << 31) - 1, max_dev=(1 << 31) - 1)]
    steps = [0, 232387521, -3527459, (1 << 31) - 1, -(1 << 31), (1 << 31) - 500, -(1 << 31) + 500]
    ratios = [(12, 125, 10), (24, 25, 10), (1, 2, 2), (32, 1023, 64)]
    seen, cs = set(), np.zeros(2, dtype=np.float32)

    def factor(step, ph0, n):
        assert L.p25fe_afc_factor(step, ph0, n, cs.ctypes.data_as(C.c_void_p)) == 0
        return cs.tobytes()
    for i, rec in enumerate(recs):
        cfg = cfgs[i % len(cfgs)]
        c = _cfg(lib, **cfg)
        l, m, d = ratios[i % len(ratios)]
        for j, at in enumerate(ats):
            step = steps[(i + j) % len(steps)]
            ref = max(-(1 << 31), min((1 << 31) - 1, step + (0, 700, -2000)[(i + j) % 3]))
            st = LM.new_state(step, int(rng.integers(0, 1 << 32)))
            st.update(n_applied=MASK if i % 7 == 0 else 3, n_rejected=MASK if i % 5 == 0 else 2, n_short=MASK if i % 3 == 0 else 1,
                      last_theta=-5, last_dstep=9)
            want_acc, want = LM.step(cfg, l, m, d, ref, (AM.wrap64(rec[0]), AM.wrap64(rec[1]), AM.wrap64(rec[2]), rec[3]), st, at)
            got_acc, got = _c_step(lib, c, l, m, d, ref, rec, st, at)
            assert got == want and got_acc == want_acc, (rec, cfg, (l, m, d), step, ref, at, got, want)
            # only the low 32 bits of abs_at matter, and the phase at abs_at stays
            assert _c_step(lib, c, l, m, d, ref, rec, st, at & MASK) == (got_acc, got)
            assert factor(st["step"], st["ph0"], at) == factor(got["step"], got["ph0"], at)
            if want["status"] == LM.APPLY:
                pulled = abs(want["last_dstep"]) == cfg["max_pull"]
                held = want["step"] != max(-(1 << 31), min((1 << 31) - 1, st["step"] + want["last_dstep"]))
                seen.add(("apply", pulled, held))
                assert ref - cfg["max_dev"] <= want["step"] <= ref + cfg["max_dev"] or abs(st["step"] - ref) > cfg["max_dev"]
            else:
                seen.add(want["status"])
                assert (got["step"], got["ph0"], got["last_theta"], got["last_dstep"]) == (st["step"], st["ph0"], -5, 9)
                assert got_acc == ((0, 0, 0, 0) if want["status"] == LM.REJECT else
                                   (AM.wrap64(rec[0]), AM.wrap64(rec[1]), AM.wrap64(rec[2]), rec[3]))
    assert {LM.SHORT, LM.REJECT, ("apply", False, False), ("apply", True, False), ("apply", False, True)} <= seen, seen


def test_gate_edges(lib):
    """3 / 4 exactly passes (>=), one part in 3000 under it fails; pow <= 0 fails whatever the gate; the gate 0 passes (0, 0)"""
    c = _cfg(lib)
    st = LM.new_state(1000)
    for rec, want in (((3000, 0, 4000, 700), LM.APPLY), ((2999, 0, 4000, 700), LM.REJECT), ((1800, 2400, 4000, 700), LM.APPLY),
                      ((1800, 2399, 4000, 700), LM.REJECT), ((3000, 0, 0, 700), LM.REJECT), ((3000, 0, -4000, 700), LM.REJECT),
                      ((3000, 0, 4000, 599), LM.SHORT), ((0, 0, 4000, 700), LM.REJECT)):
        assert _c_step(lib, c, 12, 125, 10, 1000, rec, st, 0)[1]["status"] == want == LM.step(LM.RECOMMENDED, 12, 125, 10, 1000, rec, st, 0)[1]["status"], rec
    got = _c_step(lib, _cfg(lib, coh_min_q15=0), 12, 125, 10, 1000, (0, 0, 4000, 700), st, 0)[1]
    assert (got["status"], got["step"], got["last_theta"]) == (LM.APPLY, 1000, 0)


def test_angle_against_atan2(lib):
    """theta of an applied update (gate 0, so every pair is applied) against math.atan2 within SPEC 3.0g's bound, 2^-32 turn --
    4096 times tighter than the 2^-20 turn the measure's own accuracy asks for.  Wrap-aware: a half turn is either sign."""
    rng = np.random.default_rng(32)
    c = _cfg(lib, coh_min_q15=0, min_products=1)
    st = LM.new_state(0)
    pairs = [(re, im) for re, im, _, _ in _records(rng) if re or im]
    for b in (2, 8, 20, 33, 50, 61, 63):
        pairs += [tuple(int(v) for v in rng.integers(-(1 << b) + 1, 1 << b, size=2)) for _ in range(150)]
    pairs = [(AM.wrap64(re), AM.wrap64(im)) for re, im in pairs if re or im]
    worst = 0.0
    for re, im in pairs:
        got = _c_step(lib, c, 12, 125, 10, 0, (re, im, 1, 1), st, 0)[1]
        assert got["status"] == LM.APPLY and got["last_theta"] == LM.angle(re, im)
        ref = math.atan2(float(im), float(re)) / (2.0 * math.pi) * 2.0 ** 32
        err = abs((got["last_theta"] - ref + 2.0 ** 31) % 2.0 ** 32 - 2.0 ** 31)
        worst = max(worst, err)
        assert err <= ANGLE_BOUND, (re, im, got["last_theta"], ref)
    print("angle: worst error %.3f units of 2^-32 turn over %d pairs" % (worst, len(pairs)))
    assert ANGLE_BOUND * 2.0 ** -32 <= 2.0 ** -20


def test_sign_and_size_agree_with_the_one_shot_path(lib):
    """gain 1 and no clamp: one update moves the step by what p25fe_replay -a adds, p25fe_nco_step(fs, p25fe_afc_hz(record)), to
    within the roundings of the two conversions (half a step each, plus the angle's 2^-32 turn in steps: L / (M D) < 1)"""
    from p25rx_amd.frontend import Afc, AfcLoop, Tuner
    rng = np.random.default_rng(33)
    c = _cfg(lib, max_pull=(1 << 31) - 1, max_dev=(1 << 31) - 1)
    for fs, l, m in ((2500000, 12, 125), (250000, 24, 25)):
        for _ in range(200):
            ang = float(rng.uniform(-math.pi, math.pi))
            mag = int(rng.integers(1 << 20, 1 << 50))
            rec = (int(mag * math.cos(ang)), int(mag * math.sin(ang)), mag, 1200)
            hz, coh = Afc.hz(rec, 10)
            a, s = AfcLoop.step(c, l, m, 10, 0, rec, LM.new_state(0), 0)
            assert int(s["status"]) == LM.APPLY
            assert abs(int(s["step"]) - Tuner.nco_step(fs, hz)) <= 2, (rec, hz, int(s["step"]))
            assert AfcLoop.hz(s, 10) == pytest.approx(hz, abs=240000.0 / 10 * 2.0 ** -31)
            assert (int(s["step"]) > 0) == (hz > 0) or abs(hz) < fs * 2.0 ** -32


def test_refusals_need_no_device(lib):
    """every refusal of the loop's entry points, with no handle and no object"""
    L = lib.load()
    good = dict(LM.RECOMMENDED)
    acc, st = np.zeros(1, dtype=lib.AFC_ACC_DTYPE), np.zeros(1, dtype=lib.TRACK_STATE_DTYPE)
    ap, sp = acc.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p)

    def step(cfg, l=12, m=125, d=10, a=ap, s=sp, ao=ap, so=sp):
        c = None if cfg is None else _cfg(lib, **cfg).ctypes.data_as(C.c_void_p)
        return L.p25fe_track_step(c, l, m, d, 0, a, s, 0, ao, so)
    assert step(good) == lib.OK and int(st["status"][0]) == LM.SHORT
    bad_cfgs = [dict(good, shift=-1), dict(good, shift=41), dict(good, min_products=0), dict(good, coh_min_q15=-1),
                dict(good, coh_min_q15=32769), dict(good, gain_q16=0), dict(good, gain_q16=65537), dict(good, gain_q16=-1),
                dict(good, max_pull=0), dict(good, max_pull=-5), dict(good, max_dev=0), dict(good, max_dev=-(1 << 31)),
                dict(good, reserved=1)]
    st[0] = 0
    for cfg in bad_cfgs:
        assert step(cfg) == lib.ERR_ARG, cfg
    for cfg in (dict(good, shift=0), dict(good, shift=40), dict(good, coh_min_q15=0), dict(good, coh_min_q15=32768),
                dict(good, gain_q16=1), dict(good, max_pull=(1 << 31) - 1, max_dev=(1 << 31) - 1), dict(good, min_products=(1 << 64) - 1)):
        assert step(cfg) == lib.OK, cfg
    st[0] = 0
    assert step(None) == lib.ERR_ARG
    for l, m, d in ((0, 125, 10), (33, 125, 10), (12, 12, 10), (12, 1025, 10), (6, 8, 10), (12, 125, 1), (12, 125, 65), (-1, 5, 10)):
        assert step(good, l, m, d) == lib.ERR_ARG, (l, m, d)
    for kw in (dict(a=None), dict(s=None), dict(ao=None), dict(so=None)):
        assert step(good, **kw) == lib.ERR_ARG
    assert int(st["status"][0]) == 0 and int(st["n_short"][0]) == 0   # nothing was written by a refused call
    hz = C.c_double(-1.0)
    assert L.p25fe_track_hz(None, 10, C.byref(hz)) == lib.ERR_ARG and L.p25fe_track_hz(sp, 10, None) == lib.ERR_ARG
    for d in (1, 0, -1, 65):
        assert L.p25fe_track_hz(sp, d, C.byref(hz)) == lib.ERR_ARG
    assert hz.value == -1.0
    st["last_theta"] = 1 << 30
    assert L.p25fe_track_hz(sp, 10, C.byref(hz)) == lib.OK and hz.value == 6000.0
    st["last_theta"] = -(1 << 31)
    assert L.p25fe_track_hz(sp, 2, C.byref(hz)) == lib.OK and hz.value == -60000.0
    # create: a loop needs a tuner and a measure, and the configuration is looked at before either
    out = C.c_void_p(1)
    cp = _cfg(lib).ctypes.data_as(C.c_void_p)
    assert L.p25fe_track_create(None, None, cp, C.byref(out)) == lib.ERR_ARG and not out.value
    assert L.p25fe_track_create(None, None, cp, None) == lib.ERR_ARG
    out.value = 1
    assert L.p25fe_track_create(None, None, None, C.byref(out)) == lib.ERR_ARG and not out.value
    L.p25fe_track_destroy(None)                                      # a no-op
    assert L.p25fe_track_measure_dev(None, ap, 100, 0, 100, 0, None) == lib.ERR_ARG
    assert L.p25fe_track_update_dev(None, 0, None) == lib.ERR_ARG
    assert L.p25fe_track_run_dev(None, ap, 0, 0, 128, 0, 1024, ap, 128, 0, None) == lib.ERR_ARG
    assert L.p25fe_track_read(None, sp) == lib.ERR_ARG and L.p25fe_track_records(None, ap, None) == lib.ERR_ARG


E_FS, E_WINDOW, E_RASTER, E_DRIFT = 2500000, 125000, 137500, 3000.0


@pytest.fixture(scope="module")
def drifting():
    return LM.drifting_capture(drift_hz_s=E_DRIFT)


def test_model_end_to_end(lib, rot, drifting):
    """c4fm.synth(0.75, seed=13, snr_db=25.0) at 2.5 Msps, 1871.3 Hz above the raster frequency 137500 Hz and drifting by +3000 Hz/s,
    tuned at the raster step; the recommended loop (D 10, T 240, 7 kHz, shift 24, 50 ms windows, gain 1, half a window of products,
    gate 0.75) on the bit-exact model of tuner, measure and law.  Every window is applied, and from the first update on the residual
    at every window's end -- taken just BEFORE that boundary's update, where it is largest -- stays within the 600 Hz the receive
    chain tolerates (SPEC 3.0f).  Measured on this model: at most 321 Hz (the double-precision simulation without the tuner gave
    315), coherence 0.915 - 0.932.  The tracked row decodes with 0 symbol errors from the first frame sync after the first update
    (symbol 888 of the generator's) to the end."""
    from oracle import oracle as O
    from p25rx_amd.frontend import Afc, Tuner
    wide, truth = drifting
    l, m, t, taps, steps = Tuner.design_nco(E_FS, [E_RASTER])
    assert (l, m, t) == (12, 125, 84) and len(wide) == 15 * E_WINDOW
    D, T, fc = Afc.DEFAULT
    g = Afc.design(D, T, fc)
    assert LM.RECOMMENDED["min_products"] == E_WINDOW * l // m // D // 2
    row, states, judged = LM.track(wide, l, m, t, taps, steps[0], *rot, D, T, g, LM.RECOMMENDED, E_WINDOW)
    assert len(states) == 15 and len(row) == len(wide) * l // m
    hz_per_step = E_FS / 2.0 ** 32
    worst = 0.0
    for w, (st, rec) in enumerate(zip(states, judged)):
        true = 1871.3 + E_DRIFT * (w + 1) * E_WINDOW / E_FS           # the carrier's offset from the raster at this boundary
        before = true - ((states[w - 1]["step"] if w else steps[0]) - steps[0]) * hz_per_step
        after = true - (st["step"] - steps[0]) * hz_per_step
        est, coh = AM.hz(rec, D)
        print("window %2d: coherence %.3f, estimate %7.1f Hz, residual before the update %7.1f Hz, after %6.1f Hz" % (w, coh, est, before, after))
        assert st["status"] == LM.APPLY and rec[3] == 1200 and st["n_applied"] == w + 1
        assert LM.hz(st, D) == pytest.approx(est, abs=1e-3)
        if w >= 1:
            worst = max(worst, abs(before))
            assert abs(before) <= 600.0, (w, before)
    print("largest residual at a window's end after the first update: %.1f Hz" % worst)
    dib = O.run_cf32(row)
    k = min(len(dib), len(truth) - 888)
    assert k > 2600 and np.array_equal(dib[:k], truth[888:888 + k])
    # the one-shot correction of p25fe_replay -a 50 on the same capture loses the stream: the residual passes 800 Hz
    one = (states[0]["step"] - steps[0]) * hz_per_step
    t800 = (800.0 + one - 1871.3) / E_DRIFT
    assert 0.2 < t800 < 0.35                                          # about 0.27 s in


def test_noise_row_is_rejected(lib, rot):
    """a row with nothing but white noise in it: every window is REJECTED at the recommended gate and the step never moves.  Its
    coherence is not near 0: it is the prefilter's own lag-1 autocorrelation, 0.55 - 0.59 on this model (signal rows: 0.91 - 0.93),
    and 0.75 lies between the two."""
    from p25rx_amd.frontend import Afc, Tuner
    l, m, t, taps, steps = Tuner.design_nco(E_FS, [-412500.0])
    D, T, fc = Afc.DEFAULT
    g = Afc.design(D, T, fc)
    rng = np.random.default_rng(100)
    x = (0.1 * (rng.standard_normal(3 * E_WINDOW) + 1j * rng.standard_normal(3 * E_WINDOW))).astype(np.complex64)
    row, states, judged = LM.track(x, l, m, t, taps, steps[0], *rot, D, T, g, LM.RECOMMENDED, E_WINDOW)
    assert len(states) == 3
    for w, (st, rec) in enumerate(zip(states, judged)):
        est, coh = AM.hz(rec, D)
        print("noise window %d: coherence %.3f, estimate %.1f Hz" % (w, coh, est))
        assert st["status"] == LM.REJECT and st["step"] == steps[0] and st["ph0"] == 0 and st["n_rejected"] == w + 1
        assert 0.45 < coh < 0.70 and rec[3] == 1200
