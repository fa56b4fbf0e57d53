"""CPU tests of the host side of the survey over time (docs/SPEC.md 3.0i): the ABI surface, every refusal that needs no device,
p25fe_waterfall_slots against the formula at positions past 2^32 and 2^40, and p25fe_waterfall_keys against the rule in numpy
(tests/waterfall_model.py) -- hysteresis, min_slots, a row of zero frames, a short output array, ordering, slot0 > 0 -- and on the
model's rows of the keyed scene the tests share, whose own numbers are held here.  The GPU side is tests/test_gpu_waterfall.py."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import scan_model as SM
import waterfall_model as WM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"p25fe_waterfall_slots", "p25fe_waterfall_dev", "p25fe_waterfall_open", "p25fe_waterfall", "p25fe_waterfall_read",
       "p25fe_waterfall_keys"}
KEY_C = ("int32_t raster_index; int32_t reserved; uint64_t first_slot; uint64_t n_slots; double centre_hz; double offset_hz; "
         "double peak_db_over_floor;")
KEY_RS = ("pub raster_index: i32, pub reserved: i32, pub first_slot: u64, pub n_slots: u64, pub centre_hz: f64, pub offset_hz: f64, "
          "pub peak_db_over_floor: f64,")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from p25rx_amd import _lib
    return _lib


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _keys(L, rows, N, fs, slot0=0, raster=12500.0, half_bw=4000.0, on=20.0, off=14.0, min_slots=2, cap=64, stride=None):
    from p25rx_amd._lib import WATERFALL_KEY_DTYPE
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    out = np.zeros(cap + 2, dtype=WATERFALL_KEY_DTYPE)
    out["reserved"] = -99                                            # what the call does not write stays, two records behind cap too
    n = C.c_size_t(12345)
    rc = L.p25fe_waterfall_keys(vp(rows), rows.shape[0], rows.shape[1] if stride is None else stride, N, fs, slot0, raster, half_bw,
                                on, off, min_slots, vp(out), cap, C.byref(n))
    return rc, out, n.value


def _same(got, ref):
    """the library's records against the model's tuples: integer fields equal, doubles within 1e-9 relative (sums of fewer than
    10^4 non-negative doubles carry at most n 2^-53; the centroid's numerator has one sign per channel side, |f_b| <= fs / 2)"""
    assert len(got) == len(ref), (got, ref)
    for g, (r, first, n, fc, off, peak) in zip(got, ref):
        assert (int(g["raster_index"]), int(g["first_slot"]), int(g["n_slots"]), int(g["reserved"])) == (r, first, n, 0), (g, r, first, n)
        assert g["centre_hz"] == fc
        assert g["offset_hz"] == pytest.approx(off, rel=1e-9, abs=1e-9 * max(abs(fc), 1.0)), (g, off)
        assert g["peak_db_over_floor"] == pytest.approx(peak, rel=1e-9), (g, peak)


def test_abi_surface(lib):
    """header, ctypes and the Rust text name the same six functions; none begins with p25fe_scan or with a prefix the older ABI
    tests pin; the key record is 48 bytes everywhere; positions and slots are 64-bit; the ABI version has not moved"""
    hdr = open(os.path.join(ROOT, "include", "p25fe.h")).read()
    assert re.search(r"#define P25FE_ABI_VERSION 6\b", hdr) and lib.ABI_VERSION == 6
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(p25fe_[a-z0-9_]+)\s*\(", code))
    assert {s for s in declared if s.startswith("p25fe_waterfall")} == NEW and NEW <= set(lib.SYMBOLS)
    assert not [s for s in NEW if s.startswith(("p25fe_scan", "p25fe_afc_", "p25fe_track_")) or "nco" in s or "tune" in s or "resampl" in s]
    rs = open(os.path.join(ROOT, "bindings", "p25fe.rs")).read()
    assert NEW <= set(re.findall(r"pub fn (p25fe_[a-z0-9_]+)\(", rs))
    L = lib.load()
    for s in NEW:
        assert hasattr(L, s) and getattr(L, s).argtypes is not None, s
    assert L.p25fe_waterfall_dev.argtypes[5] is C.c_uint64 and L.p25fe_waterfall_dev.argtypes[7] is C.c_uint64
    assert L.p25fe_waterfall_dev.argtypes[6] is C.c_uint32
    m = re.search(r"pub fn p25fe_waterfall_dev\((.*?)\)", rs, re.S)
    assert [a.split(":")[1].strip() for a in m.group(1).split(",") if a.strip()][5:8] == ["u64", "u32", "u64"]
    m = re.search(r"int p25fe_waterfall_dev\((.*?)\)", code, re.S)
    assert [a.strip() for a in m.group(1).split(",")][5:8] == ["uint64_t abs_first", "uint32_t B", "uint64_t slot0"]
    assert lib.WATERFALL_KEY_DTYPE.itemsize == 48
    assert lib.WATERFALL_KEY_DTYPE.names == ("raster_index", "reserved", "first_slot", "n_slots", "centre_hz", "offset_hz",
                                             "peak_db_over_floor")
    m = re.search(r"typedef struct p25fe_waterfall_key \{(.*?)\} p25fe_waterfall_key_t;", code, re.S)
    assert re.sub(r"\s+", " ", m.group(1)).strip() == KEY_C
    m = re.search(r"pub struct WaterfallKey \{(.*?)\}", rs, re.S)
    assert re.sub(r"\s+", " ", m.group(1)).strip() == KEY_RS
    # the kernel's source is a dependency of the library and not among the sources embedded for hipRTC
    mk = open(os.path.join(ROOT, "p25rx_amd", "csrc", "Makefile")).read()
    ksrc = re.search(r"^KSRC\s*:=(.*)$", mk, re.M).group(1)
    assert "p25fe_waterfall.inc" not in ksrc and "p25fe_waterfall.inc" in mk


def test_refusals_need_no_device(lib):
    """every refusal of the calls with no object, and of the host-only calls: nothing here reaches a device"""
    L = lib.load()
    buf = np.zeros(4096, dtype=np.float32)
    rows = np.zeros((2, 4097), dtype=np.uint64)
    bp, rp = vp(buf), vp(rows)
    # no object: everything else right, then each further refusal -- all P25FE_ERR_ARG like p25fe_scan_dev's
    for d_iq, d_rows, abs_first, B, stride, n_rows in (
            (bp, rp, 0, 6, 4097, 2), (None, rp, 0, 6, 4097, 2), (bp, None, 0, 6, 4097, 2),
            (C.c_void_p(buf.ctypes.data + 8), rp, 0, 6, 4097, 2), (bp, C.c_void_p(rows.ctypes.data + 4), 0, 6, 4097, 2),
            (bp, rp, 1 << 62, 6, 4097, 2), (bp, rp, 0, 0, 4097, 2), (bp, rp, 0, (1 << 20) + 1, 4097, 2), (bp, rp, 0, 6, 1024, 2),
            (bp, rp, 0, 6, 4097, 0)):
        assert L.p25fe_waterfall_dev(None, d_iq, lib.FMT_CF32, 0, 2048, abs_first, B, 0, d_rows, n_rows, stride, None) == lib.ERR_ARG
    assert L.p25fe_waterfall_dev(None, bp, 7, 0, 2048, 0, 6, 0, rp, 2, 4097, None) == lib.ERR_ARG       # an unknown format
    assert not rows.any()
    n = C.c_size_t(5)
    assert L.p25fe_waterfall_open(None, 6, 16) == lib.ERR_ARG
    assert L.p25fe_waterfall(None, bp, lib.FMT_CF32, 16) == lib.ERR_ARG
    assert L.p25fe_waterfall_read(None, rp, 2, C.byref(n)) == lib.ERR_ARG and n.value == 0
    # slots
    first = C.c_uint64(9)
    for hop, B, abs_first, cnt in ((0, 6, 0, 100), (4, 6, 0, 100), (12, 6, 0, 100), (8192, 6, 0, 100), (-8, 6, 0, 100), (96, 6, 0, 100),
                                   (2048, 0, 0, 100), (2048, (1 << 20) + 1, 0, 100), (2048, 6, 1 << 62, 100), (2048, 6, 0, 1 << 62)):
        assert L.p25fe_waterfall_slots(hop, B, abs_first, cnt, C.byref(first), C.byref(n)) == lib.ERR_ARG, (hop, B, abs_first, cnt)
    assert L.p25fe_waterfall_slots(2048, 6, 0, 100, None, C.byref(n)) == lib.ERR_ARG
    assert L.p25fe_waterfall_slots(2048, 6, 0, 100, C.byref(first), None) == lib.ERR_ARG
    # keys
    ok = dict(N=1024, fs=1024000)
    good = np.ones((3, 1025), dtype=np.uint64)
    assert _keys(L, good, **ok)[0] == lib.OK
    for kw in (dict(on=14.0, off=20.0), dict(on=float("nan")), dict(off=float("nan")), dict(on=float("inf")), dict(off=float("-inf")),
               dict(min_slots=0), dict(raster=0.0), dict(raster=float("nan")), dict(raster=-1.0), dict(half_bw=-1.0),
               dict(half_bw=float("inf")), dict(stride=1024), dict(N=512), dict(N=2048), dict(fs=0)):
        assert _keys(L, good, **dict(ok, **kw))[0] == lib.ERR_ARG, kw
    out = np.zeros(4, dtype=lib.WATERFALL_KEY_DTYPE)
    assert L.p25fe_waterfall_keys(None, 3, 1025, 1024, 1024000, 0, 12500.0, 4000.0, 20.0, 14.0, 2, vp(out), 4, C.byref(n)) == lib.ERR_ARG
    assert L.p25fe_waterfall_keys(vp(good), 3, 1025, 1024, 1024000, 0, 12500.0, 4000.0, 20.0, 14.0, 2, vp(out), 4, None) == lib.ERR_ARG
    assert L.p25fe_waterfall_keys(vp(good), 3, 1025, 1024, 1024000, 0, 12500.0, 4000.0, 20.0, 14.0, 2, None, 4, C.byref(n)) == lib.ERR_ARG
    assert L.p25fe_waterfall_keys(vp(good), 0, 1025, 1024, 1024000, 0, 12500.0, 4000.0, 20.0, 14.0, 2, vp(out), 4, C.byref(n)) == lib.OK
    assert n.value == 0


def test_slots_are_the_formula(lib):
    """first slot floor(f0 / B) and the count, against Python integers: small positions, positions past 2^32 and 2^40, ranges
    that own no frame, a range inside one slot, B = 1 and B = 2^20"""
    L = lib.load()
    from p25rx_amd import Scanner
    rng = np.random.default_rng(40)
    cases = [(2048, 6, 0, 0), (2048, 6, 0, 2047), (2048, 6, 1, 2046), (2048, 6, 1, 2047), (2048, 6, 2047, 1), (8, 1, 5, 3), (8, 1, 5, 2),
             (64, 7, (1 << 32) + 13, 100000), (2048, 6, (1 << 40) + 5, 100000), (8, 1 << 20, (1 << 40) + 8 * 3 + 1, 1 << 30),
             (1024, 5, (1 << 40) + 1023, 1), (1024, 5, (1 << 40) + 1023, 0), (4096, 3, (1 << 61) + 77, 1 << 33)]
    for _ in range(200):
        hop = int(rng.choice([8, 64, 512, 2048, 4096]))
        base = int(rng.choice([0, 1 << 32, 1 << 40, (1 << 61)]))
        cases.append((hop, int(rng.integers(1, 50)), base + int(rng.integers(0, 1 << 20)), int(rng.integers(0, 40 * hop))))
    some_empty = 0
    for hop, B, first, n in cases:
        ref = WM.slots(hop, B, first, n)
        f0, f1 = first // hop, (first + n) // hop
        assert ref == (f0 // B, 0 if f1 == f0 else (f1 - 1) // B - f0 // B + 1)
        assert Scanner.slots(hop, B, first, n) == ref, (hop, B, first, n)
        some_empty += ref[1] == 0
    assert some_empty >= 4 and Scanner.slots(2048, 6, (1 << 40) + 5, 100000) == (((1 << 40) + 5) // 2048 // 6, 9)


def test_the_models_batches_and_contributors():
    """what tests/test_gpu_waterfall_edges.py's premises are asserted with: WM.batch at the shapes that file launches (and at
    the formula's three regimes), WM.contributors on cases counted by hand"""
    for N, hop, frames, F in ((1024, 512, 70, 8), (1024, 256, 70, 16), (4096, 1024, 70, 16), (4096, 2048, 40, 8), (1024, 512, 9221, 10)):
        assert WM.batch(N, hop, frames) == F, (N, hop, frames)
    assert WM.batch(1024, 8, 9230) == 512 and WM.batch(1024, 64, 70) == 64 and WM.batch(4096, 4096, 1) == 8
    assert WM.batch(1024, 512, 8 * 1024) == 8 and WM.batch(1024, 512, 8 * 1024 + 1) == 9
    assert WM.batch(1024, 1024, (1 << 30) + 1) == 1 << 20
    # frames 5 .. 14 in batches of 4 (workgroup 0: 5 .. 8, 1: 9 .. 12, 2: 13, 14), slots of 3 (slot 1: 5; 2: 6 .. 8; 3: 9 .. 11;
    # 4: 12 .. 14)
    assert WM.contributors(5, 10, 4, 3) == [{0}, {0}, {1}, {1, 2}]
    # frames 6 .. 14 in batches of 2 (6 7 | 8 9 | 10 11 | 12 13 | 14), slots of 6 (slot 1: 6 .. 11; 2: 12 .. 14)
    assert WM.contributors(6, 9, 2, 6) == [{0, 1, 2}, {3, 4}]
    # frames 7 .. 11 in batches of 4 (7 .. 10 | 11), slots of 4 (slot 1: 7; 2: 8 .. 11): both workgroups meet in the second row
    assert WM.contributors(7, 5, 4, 4) == [{0}, {0, 1}]
    assert WM.contributors(3, 4, 8, 1 << 20) == [{0}] and WM.contributors(3, 0, 8, 5) == []
    for fa, k, F, B in ((5, 10, 4, 3), (6, 9, 2, 6), (0, 70, 8, 29), ((1 << 40) + 3, 70, 16, 17)):
        con = WM.contributors(fa, k, F, B)
        assert len(con) == WM.group(np.zeros((k, 2)), fa, B)[1].shape[0] == WM.slots(1, B, fa, k)[1]
        assert set().union(*con) == set(range(-(-k // F)))


def _quiet(n_rows, N=1024, frames=6):
    """rows of a flat floor: every bin 100 per frame"""
    rows = np.full((n_rows, N + 1), 100 * frames, dtype=np.uint64)
    rows[:, N] = frames
    return rows


def test_keys_follow_the_rule(lib):
    """synthetic rows at N = 1024, fs = 1.024 Msps (bins 1000 Hz apart; r = 2 on bin 25, r = -4 on bin N - 50): against the model
    and against what the rule says -- hysteresis, min_slots, a row of zero frames, a short cap, the order, slot0 > 0"""
    L = lib.load()
    N, fs = 1024, 1024000
    kw = dict(N=N, fs=fs)
    floor = 9 * 600.0                                                # nine bins within 4 kHz of a centre, 600 each

    def level(db):
        return int(round(floor * 10.0 ** (db / 10.0)))               # one bin this strong is `db` over the floor, nearly
    # hysteresis: 30 dB, a dip to 17 dB (between off and on) does not split; a dip to 10 dB (below off) does
    rows = _quiet(12)
    rows[1:10, 25] = level(30.0)
    rows[4, 25] = level(17.0)
    rows[7, 25] = level(10.0)
    rc, out, n = _keys(L, rows, **kw)
    ref = WM.keys(rows, N, fs)
    assert rc == lib.OK and n == 2 and [(k[0], k[1], k[2]) for k in ref] == [(2, 1, 6), (2, 8, 2)]
    _same(out[:n], ref)
    assert (out["reserved"][n:] == -99).all() and len(out) == 66
    assert out["peak_db_over_floor"][0] == pytest.approx(30.0, abs=0.01) and abs(out["offset_hz"][0]) < 3.0
    # 17 dB alone never turns a channel on
    rows = _quiet(6)
    rows[1:5, 25] = level(17.0)
    assert _keys(L, rows, **kw)[2] == 0 and WM.keys(rows, N, fs) == []
    # min_slots: intervals of 1, 2 and 3 rows
    rows = _quiet(12)
    rows[1, 25] = rows[3:5, 25] = rows[6:9, 25] = level(30.0)
    for m, want in ((1, [(1, 1), (3, 2), (6, 3)]), (2, [(3, 2), (6, 3)]), (3, [(6, 3)]), (4, [])):
        rc, out, n = _keys(L, rows, min_slots=m, **kw)
        assert rc == lib.OK and [(int(k["first_slot"]), int(k["n_slots"])) for k in out[:n]] == want, m
        _same(out[:n], WM.keys(rows, N, fs, min_slots=m))
    # a row of zero frames in the middle ends the interval, whatever its words say; the end of the rows ends one too
    rows = _quiet(10)
    rows[2:, 25] = level(30.0)
    rows[5, N] = 0
    rc, out, n = _keys(L, rows, **kw)
    assert [(int(k["first_slot"]), int(k["n_slots"])) for k in out[:n]] == [(2, 3), (6, 4)]
    _same(out[:n], WM.keys(rows, N, fs))
    # order (first slot, then raster index), slot0 > 0, a spike off the centre, a short cap with the full count
    rows = _quiet(12)
    rows[3:9, 28] = level(30.0)                                      # r = 2, 3 kHz above its centre
    rows[3:7, N - 50] = level(25.0)                                  # r = -4, the same first slot
    rows[1:4, 100] = level(35.0)                                     # r = 8
    slot0 = (1 << 40) + 3
    rc, out, n = _keys(L, rows, slot0=slot0, **kw)
    ref = WM.keys(rows, N, fs, slot0=slot0)
    assert rc == lib.OK and n == 3
    assert [(int(k["raster_index"]), int(k["first_slot"]) - slot0, int(k["n_slots"])) for k in out[:n]] == [(8, 1, 3), (-4, 3, 4), (2, 3, 6)]
    _same(out[:n], ref)
    assert 2900.0 < out["offset_hz"][2] < 3000.0 and list(out["centre_hz"][:3]) == [100000.0, -50000.0, 25000.0]
    rc, short, n = _keys(L, rows, slot0=slot0, cap=2, **kw)
    assert rc == lib.OK and n == 3 and (short["reserved"][2:] == -99).all()
    _same(short[:2], ref[:2])
    rc, none, n = _keys(L, rows, slot0=slot0, cap=0, **kw)
    assert rc == lib.OK and n == 3 and (none["reserved"] == -99).all()
    # padding words behind N + 1 are not looked at
    wide = np.full((12, N + 5), (1 << 64) - 1, dtype=np.uint64)
    wide[:, :N + 1] = rows
    rc, out, n = _keys(L, wide, slot0=slot0, **kw)
    _same(out[:n], ref)
    # frames but no power at all: nothing turns on
    z = np.zeros((4, N + 1), dtype=np.uint64)
    z[:, N] = 6
    assert _keys(L, z, **kw)[2] == 0 and WM.keys(z, N, fs) == []
    from p25rx_amd import Scanner
    got = Scanner.keys(rows, fs, slot0=slot0)
    _same(got, ref)


@pytest.fixture(scope="module")
def scene_rows():
    """the model's rows of the keyed scene in all three formats: format -> uint64 [51, 4097]"""
    x = WM.keyed_scene()
    spec = json.load(open(os.path.join(ROOT, "tests", "golden", "spec.json")))
    caps = {"cf32": x, "s16": SM.convert_s16(SM.to_s16(x)), "u8": SM.convert_u8(SM.to_u8(x), spec["u8_scale"], spec["u8_offset"])}
    out = {}
    for f, c in caps.items():
        slot0, rows = WM.rows(c, WM.KEY_N, WM.KEY_HOP, SM.window(WM.KEY_N), WM.KEY_SHIFT, WM.KEY_B)
        assert slot0 == 0
        out[f] = rows
    return out


def test_the_keyed_scene_on_the_models_rows(lib, scene_rows):
    """0.25 s at 2.5 Msps, N 4096, hop 2048, B 6: 305 frames in 51 slots.  The model's own numbers, held here: a keyed channel
    stands at least 37.5 dB over the floor in every slot the keying covers whole (asserted: 35) and 28.6 dB in a partly keyed edge
    slot (asserted: 25); every channel neither keyed nor next to a keyed one stays at or below 6.8 dB (asserted: 10) -- so at
    20 / 14 dB nothing rests on the thresholds.  The condition: exactly the five intervals, each within one slot of the truth at
    either end, none on a channel that was never keyed; offsets within 200 Hz of the truth (the model's largest deviation: 159 Hz);
    the library agrees with the model"""
    L = lib.load()
    truth = WM.keyed_truth()
    assert [(r, a, b) for r, a, b, _o in truth] == [(-33, 0, 50), (11, 2, 23), (12, 8, 34), (40, 14, 44), (11, 27, 49)]
    worst = 0.0
    for fmt, rows in scene_rows.items():
        assert rows.shape == (51, WM.KEY_N + 1) and list(rows[:, WM.KEY_N]) == [6] * 50 + [5]
        idx, db = WM.channel_db(rows, WM.KEY_N, WM.KEY_FS)
        whole, edge, near = (np.zeros(db.shape, dtype=bool) for _ in range(3))
        for r, a, b, _off in truth:
            whole[a + 1:b, idx[r]] = True
            if a > 0:
                edge[a, idx[r]] = True
            if b < 50:
                edge[b, idx[r]] = True
            near[max(a - 1, 0):b + 2, idx[r] - 1:idx[r] + 2] = True
        edge &= ~whole
        print(fmt, "whole slots %.1f .. %.1f dB, edge slots %.1f .. %.1f dB, idle channels at most %.1f dB"
              % (db[whole].min(), db[whole].max(), db[edge].min(), db[edge].max(), db[~near].max()))
        assert db[whole].min() >= 35.0 and db[edge].min() >= 25.0 and db[~near].max() <= 10.0
        rc, out, n = _keys(L, rows, WM.KEY_N, WM.KEY_FS)
        assert rc == lib.OK and n == 5, (fmt, n)
        got = out[:n]
        ref = WM.keys(rows, WM.KEY_N, WM.KEY_FS)
        _same(got, ref)
        for k, (r, a, b, off) in zip(got, truth):
            first, last = int(k["first_slot"]), int(k["first_slot"]) + int(k["n_slots"]) - 1
            assert int(k["raster_index"]) == r and abs(first - a) <= 1 and abs(last - b) <= 1, (fmt, k, (r, a, b))
            worst = max(worst, abs(k["offset_hz"] - off))
            assert abs(k["offset_hz"] - off) <= 200.0, (fmt, k, off)
            assert k["peak_db_over_floor"] >= 35.0
        assert set(int(r) for r in got["raster_index"]) == {-33, 11, 12, 40}
    print("largest deviation of offset_hz from the true offsets: %.1f Hz" % worst)
