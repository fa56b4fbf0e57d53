"""CPU tests of the host side of the survey (docs/SPEC.md 3.0h): the ABI surface, p25fe_scan_window against the formula bit for
bit, every refusal that needs no device, and p25fe_scan_channels on the records of the numpy model (tests/scan_model.py) for the
scene the survey's tests share -- four C4FM sources a crystal's few ppm off the raster in a 2.5 Msps capture with white noise --
in all three formats, plus ties, a short output array and a record of zero frames; and the model's own per-frame records with
the premise of the clamp test (bin 100 surely saturated, no ambiguous bin).  The GPU side is tests/test_gpu_scan.py and
tests/test_gpu_scan_edges.py."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import scan_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"p25fe_scan_window", "p25fe_scan_create", "p25fe_scan_destroy", "p25fe_scan_reset", "p25fe_scan_dev", "p25fe_scan",
       "p25fe_scan_read", "p25fe_scan_channels"}
FS = SM.SCENE_FS


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from p25rx_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def records():
    """the model's records of the scene: (N, format) -> uint64 [N + 1] at hop N / 2, shift 16, and the 16-frame one"""
    x, _truths = SM.scene()
    spec = json.load(open(os.path.join(ROOT, "tests", "golden", "spec.json")))
    caps = {"cf32": x, "s16": SM.convert_s16(SM.to_s16(x)), "u8": SM.convert_u8(SM.to_u8(x), spec["u8_scale"], spec["u8_offset"])}
    rec = {(N, f): SM.record(c, N, N // 2, SM.window(N), 16) for N in (1024, 4096) for f, c in caps.items()}
    rec[(4096, "16 frames")] = SM.record(x, 4096, 2048, SM.window(4096), 16, 0, 16 * 2048)
    return rec


def _channels(L, acc, N, fs, raster=12500.0, half_bw=4000.0, thr=20.0, cap=None, lib=None):
    from p25rx_amd._lib import SCAN_CHAN_DTYPE
    acc = np.ascontiguousarray(acc, dtype=np.uint64)
    cap = N if cap is None else cap
    out = np.zeros(max(cap, 1), dtype=SCAN_CHAN_DTYPE)
    out["reserved"] = -99                                            # what the call does not write stays
    n = C.c_size_t(12345)
    rc = L.p25fe_scan_channels(acc.ctypes.data_as(C.c_void_p), N, fs, raster, half_bw, thr, out.ctypes.data_as(C.c_void_p), cap,
                               C.byref(n))
    return rc, out, n.value


def test_abi_surface(lib):
    """header, ctypes and the Rust text name the same eight functions, none of which begins with a prefix the older ABI tests pin;
    the channel record is 32 bytes everywhere; positions are 64-bit at the header's argument index; the ABI version has not moved"""
    hdr = open(os.path.join(ROOT, "include", "p25fe.h")).read()
    assert re.search(r"#define P25FE_ABI_VERSION 6\b", hdr) and lib.ABI_VERSION == 6
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(p25fe_[a-z0-9_]+)\s*\(", code))
    assert {s for s in declared if s.startswith("p25fe_scan")} == NEW and NEW <= set(lib.SYMBOLS)
    assert not [s for s in NEW if s.startswith(("p25fe_afc_", "p25fe_track_")) or "nco" in s or "tune" in s or "resampl" in s]
    rs = open(os.path.join(ROOT, "bindings", "p25fe.rs")).read()
    assert NEW <= set(re.findall(r"pub fn (p25fe_[a-z0-9_]+)\(", rs))
    L = lib.load()
    for s in NEW:
        assert hasattr(L, s) and getattr(L, s).argtypes is not None, s
    assert L.p25fe_scan_dev.argtypes[5] is C.c_uint64
    m = re.search(r"pub fn p25fe_scan_dev\((.*?)\)", rs, re.S)
    assert [a.split(":")[1].strip() for a in m.group(1).split(",") if a.strip()][5] == "u64"
    m = re.search(r"int p25fe_scan_dev\((.*?)\)", code, re.S)
    assert m.group(1).split(",")[5].strip() == "uint64_t abs_first"
    assert lib.SCAN_CHAN_DTYPE.itemsize == 32
    assert lib.SCAN_CHAN_DTYPE.names == ("raster_index", "reserved", "centre_hz", "db_over_floor", "offset_hz")
    m = re.search(r"typedef struct p25fe_scan_chan \{(.*?)\} p25fe_scan_chan_t;", code, re.S)
    assert re.sub(r"\s+", " ", m.group(1)).strip() == \
        "int32_t raster_index; int32_t reserved; double centre_hz; double db_over_floor; double offset_hz;"
    m = re.search(r"pub struct ScanChan \{(.*?)\}", rs, re.S)
    assert re.sub(r"\s+", " ", m.group(1)).strip() == \
        "pub raster_index: i32, pub reserved: i32, pub centre_hz: f64, pub db_over_floor: f64, pub offset_hz: f64,"
    assert re.search(r"#define P25FE_SCAN_MAX_SHIFT 40\b", hdr) and lib.SCAN_MAX_SHIFT == 40
    assert re.search(r"pub const SCAN_MAX_SHIFT: i32 = 40;", rs)
    # the kernel's source is not among the sources embedded for hipRTC
    mk = open(os.path.join(ROOT, "p25rx_amd", "csrc", "Makefile")).read()
    ksrc = re.search(r"^KSRC\s*:=(.*)$", mk, re.M).group(1)
    assert "p25fe_scan.inc" not in ksrc and "p25fe_scan.inc" in mk


def test_window_is_the_formula(lib):
    """periodic Hann evaluated in double and rounded once, bit for bit; the refusals"""
    L = lib.load()
    from p25rx_amd import Scanner
    for N in (1024, 4096):
        w = Scanner.design(N)
        assert w.dtype == np.float32 and w.shape == (N,)
        assert np.array_equal(w.view(np.uint32), SM.window(N).view(np.uint32)), N
        assert w[0] == 0.0 and w[N // 2] == 1.0 and np.array_equal(w[1:], w[1:][::-1])
    buf = np.full(1024, np.float32(-3.0))
    p = buf.ctypes.data_as(C.c_void_p)
    for N in (0, -1, 512, 2048, 1023, 8192, 2147483647):
        assert L.p25fe_scan_window(N, p, 1 << 20) == lib.ERR_ARG, N
    assert L.p25fe_scan_window(1024, p, 1023) == lib.ERR_CAPACITY and L.p25fe_scan_window(1024, None, 1024) == lib.ERR_CAPACITY
    assert (buf == -3.0).all()


def test_refusals_need_no_device(lib):
    """every refusal of create with no handle, and of the calls on an object with no object: nothing here reaches a device"""
    L = lib.load()
    win = np.full(4096, np.float32(0.5))
    wp = win.ctypes.data_as(C.c_void_p)
    out = C.c_void_p(1)

    def create(N, hop, shift, win_p=wp, out_p=None):
        out.value = 1
        return L.p25fe_scan_create(None, N, hop, win_p, shift, C.byref(out) if out_p is None else out_p)
    for N in (0, -1, 512, 2048, 1000, 8192, 2147483647):             # bad N
        assert create(N, 8, 16) == lib.ERR_ARG and not out.value, N
    for N, hop in ((1024, 0), (1024, 4), (1024, 12), (1024, 24), (1024, 2048), (1024, -8), (1024, 1032), (4096, 8192), (4096, 96),
                   (4096, 4095), (4096, 2147483640), (1024, 4096)):  # bad hop: < 8, not a multiple of 8, not a divisor, > N
        assert create(N, hop, 16) == lib.ERR_ARG and not out.value, (N, hop)
    for shift in (-1, 41, 2147483647, -2147483648):
        assert create(4096, 2048, shift) == lib.ERR_ARG and not out.value, shift
    for N in (1024, 4096):
        bad = np.array(win[:N])
        for v in (np.nan, np.inf, -np.inf):
            bad[N - 1] = v                                           # the LAST value: the check reads exactly N of them
            assert create(N, N // 2, 16, win_p=bad.ctypes.data_as(C.c_void_p)) == lib.ERR_ARG and not out.value
    assert L.p25fe_scan_create(None, 4096, 2048, wp, 16, None) == lib.ERR_ARG
    for N, hop, shift, w in ((4096, 2048, 16, wp), (1024, 8, 0, None), (1024, 1024, 40, wp), (4096, 4096, 16, None)):
        assert create(N, hop, shift, win_p=w) == lib.ERR_ARG and not out.value      # everything right but the handle
    L.p25fe_scan_destroy(None)                                       # a no-op
    rec = np.zeros(4097, dtype=np.uint64)
    rp = rec.ctypes.data_as(C.c_void_p)
    assert L.p25fe_scan_reset(None) == lib.ERR_ARG
    assert L.p25fe_scan_read(None, rp, 0) == lib.ERR_ARG
    assert L.p25fe_scan(None, wp, lib.FMT_CF32, 16) == lib.ERR_ARG
    # no object: a null pointer, a misaligned pointer and a position at 2^62 are refused like everything else
    for d_iq, d_acc, abs_first in ((None, rp, 0), (wp, None, 0), (C.c_void_p(win.ctypes.data + 8), rp, 0),
                                   (wp, C.c_void_p(rec.ctypes.data + 4), 0), (wp, rp, 1 << 62), (wp, rp, (1 << 64) - 1), (wp, rp, 0)):
        assert L.p25fe_scan_dev(None, d_iq, lib.FMT_CF32, 0, 2048, abs_first, d_acc, None) == lib.ERR_ARG
    assert not rec.any()


def test_channels_on_the_models_records(lib, records):
    """exactly the raster indices {-33, 0, 11, 12} for all three formats at N = 1024 and 4096 and for the 16-frame record; every
    db_over_floor at least 35; no other channel within 10 dB of the threshold on either side; offset_hz within 200 Hz of the true
    offsets (the largest deviation of the model is 147 Hz; the receive chain tolerates 600 Hz); the library agrees with the model"""
    L = lib.load()
    worst = 0.0
    for (N, what), acc in records.items():
        rc, out, n = _channels(L, acc, N, FS)
        assert rc == lib.OK and n == 4, (N, what, n)
        got = out[:n]
        assert set(int(r) for r in got["raster_index"]) == set(SM.SCENE_CHANNELS), (N, what)
        assert (got["reserved"] == 0).all() and (out["reserved"][n:] == -99).all()
        assert (got["db_over_floor"] >= 35.0).all(), (N, what, got["db_over_floor"])
        assert (np.diff(got["db_over_floor"]) <= 0).all()            # strongest first
        for ch in got:
            r = int(ch["raster_index"])
            assert ch["centre_hz"] == r * 12500.0
            dev = abs(ch["offset_hz"] - SM.SCENE_CHANNELS[r])
            worst = max(worst, dev)
            assert dev <= 200.0, (N, what, r, ch["offset_hz"])
        # every eligible channel, listed with no threshold: none within 10 dB of the 20 dB threshold
        rc, every, n_all = _channels(L, acc, N, FS, thr=-400.0)
        assert rc == lib.OK and n_all == 199                         # |r| <= 99 at 2.5 Msps
        db = every["db_over_floor"][:n_all]
        assert ((db >= 30.0) | (db <= 10.0)).all(), (N, what, db[(db < 30.0) & (db > 10.0)])
        print(N, what, "frames", int(acc[N]), "over floor %.1f .. %.1f dB" % (got["db_over_floor"].min(), got["db_over_floor"].max()),
              "fifth %.1f dB" % db[4])
        # the model's list
        ref = SM.channels(acc, FS)
        assert [r for r, _c, _d, _o in ref] == [int(r) for r in got["raster_index"]]
        for (r, c, d, o), ch in zip(ref, got):
            assert ch["db_over_floor"] == pytest.approx(d, abs=1e-9) and ch["offset_hz"] == pytest.approx(o, abs=1e-6)
    print("largest deviation of offset_hz from the true offsets: %.1f Hz" % worst)
    from p25rx_amd import Scanner
    chans = Scanner.channels(records[(4096, "cf32")], FS)
    assert [int(r) for r in chans["raster_index"]] == [r for r, _c, _d, _o in SM.channels(records[(4096, "cf32")], FS)]


def test_ties_short_output_and_empty_records(lib):
    """two channels of equal power: the smaller raster index first; cap < n_out: the count is whole and only cap records are
    written; a record of zero frames has no channel; the refusals"""
    L = lib.load()
    N, fs = 1024, 1024000                                            # bins 1000 Hz apart
    acc = np.ones(N + 1, dtype=np.uint64)
    acc[N] = 3
    acc[25] = 1000000                                                # r = 2 at 25 kHz, on a bin
    acc[N - 50] = 1000000                                            # r = -4 at -50 kHz, on a bin
    rc, out, n = _channels(L, acc, N, fs)
    assert rc == lib.OK and n == 2
    assert [int(r) for r in out["raster_index"][:2]] == [-4, 2]      # the tie goes to the smaller r
    assert out["db_over_floor"][0] == out["db_over_floor"][1] and out["db_over_floor"][0] > 40.0
    assert np.abs(out["offset_hz"][:2]).max() < 1e-6 and list(out["centre_hz"][:2]) == [-50000.0, 25000.0]
    assert [(r, c) for r, c, _d, _o in SM.channels(acc, fs)] == [(-4, -50000.0), (2, 25000.0)]
    acc[25] += 1
    rc, out, n = _channels(L, acc, N, fs)
    assert n == 2 and [int(r) for r in out["raster_index"][:2]] == [2, -4]
    # a spike off the centre moves the centroid, not the index
    acc2 = np.ones(N + 1, dtype=np.uint64)
    acc2[28] = 1000000
    rc, out, n = _channels(L, acc2, N, fs)
    assert n == 1 and int(out["raster_index"][0]) == 2 and 2900.0 < out["offset_hz"][0] < 3000.0
    # cap < n_out
    rc, out, n = _channels(L, acc, N, fs, cap=1)
    assert rc == lib.OK and n == 2 and int(out["raster_index"][0]) == 2
    rc, out, n = _channels(L, acc, N, fs, cap=0)
    assert rc == lib.OK and n == 2 and out["reserved"][0] == -99
    n_sz = C.c_size_t(7)
    assert L.p25fe_scan_channels(acc.ctypes.data_as(C.c_void_p), N, fs, 12500.0, 4000.0, 20.0, None, 0, C.byref(n_sz)) == lib.OK
    assert n_sz.value == 2
    # zero frames
    acc[N] = 0
    rc, out, n = _channels(L, acc, N, fs)
    assert rc == lib.OK and n == 0 and out["reserved"][0] == -99 and SM.channels(acc, fs) == []
    rc, out, n = _channels(L, np.zeros(N + 1, dtype=np.uint64), N, fs)
    assert rc == lib.OK and n == 0
    # frames but no power at all: nothing is active (0 >= 0 does not count)
    z = np.zeros(N + 1, dtype=np.uint64)
    z[N] = 5
    rc, out, n = _channels(L, z, N, fs)
    assert rc == lib.OK and n == 0
    # a raster wider than the capture
    rc, out, n = _channels(L, acc2, N, fs, raster=2e6)
    assert rc == lib.OK and n == 0
    # refusals
    ap = acc2.ctypes.data_as(C.c_void_p)
    op = out.ctypes.data_as(C.c_void_p)
    assert L.p25fe_scan_channels(None, N, fs, 12500.0, 4000.0, 20.0, op, 4, C.byref(n_sz)) == lib.ERR_ARG
    assert L.p25fe_scan_channels(ap, N, fs, 12500.0, 4000.0, 20.0, op, 4, None) == lib.ERR_ARG
    assert L.p25fe_scan_channels(ap, N, fs, 12500.0, 4000.0, 20.0, None, 4, C.byref(n_sz)) == lib.ERR_ARG
    for bad_n in (0, 512, 2048, -1):
        assert L.p25fe_scan_channels(ap, bad_n, fs, 12500.0, 4000.0, 20.0, op, 4, C.byref(n_sz)) == lib.ERR_ARG
    assert L.p25fe_scan_channels(ap, N, 0, 12500.0, 4000.0, 20.0, op, 4, C.byref(n_sz)) == lib.ERR_ARG
    for raster in (0.0, -12500.0, float("nan"), float("inf")):
        assert L.p25fe_scan_channels(ap, N, fs, raster, 4000.0, 20.0, op, 4, C.byref(n_sz)) == lib.ERR_ARG
    for bw in (-1.0, float("nan"), float("inf")):
        assert L.p25fe_scan_channels(ap, N, fs, 12500.0, bw, 20.0, op, 4, C.byref(n_sz)) == lib.ERR_ARG
    for thr in (float("nan"), float("inf"), float("-inf")):
        assert L.p25fe_scan_channels(ap, N, fs, 12500.0, 4000.0, thr, op, 4, C.byref(n_sz)) == lib.ERR_ARG


def _converted(raw):
    spec = json.load(open(os.path.join(ROOT, "tests", "golden", "spec.json")))
    return {"cf32": raw["cf32"], "s16": SM.convert_s16(raw["s16"]), "u8": SM.convert_u8(raw["u8"], spec["u8_scale"], spec["u8_offset"])}


def test_the_models_record_is_the_wrapping_sum_of_its_frames():
    """record() of a range equals the sum modulo 2^64 of frame_records() of the same frames, word for word: on a noisy signal at
    a small hop with part of the history missing, and on the saturating scene, where four frames of 2^62 wrap bin 100 to zero"""
    rng = np.random.default_rng(11)
    x = (0.3 * (rng.standard_normal(3000) + 1j * rng.standard_normal(3000))).astype(np.complex64)
    w = SM.window(1024)
    for first, n, n_hist in ((1024 + 24, 70 * 8 + 16, None), (520, 1400, 100), (0, 3000, 0)):
        X = SM.spectra(x, 1024, 8, w, first, n, n_hist)
        rec = SM.frame_records(X, 16)
        assert rec.shape == (SM.n_frames(8, first, n), 1025) and (rec[:, 1024] == 1).all()
        assert np.array_equal(SM.wrapping_sum(rec), SM.record(x, 1024, 8, w, 16, first, n, n_hist))
    cf = _converted(SM.saturating_capture())
    N, H = SM.SAT_N, SM.SAT_HOP
    for fmt, c in cf.items():
        X = SM.spectra(c, N, H, SM.saturating_window(), N, 4 * H)
        rec = SM.frame_records(X, SM.SAT_SHIFT)
        assert (rec[:, SM.SAT_BIN] == np.uint64(1 << 62)).all(), fmt
        whole = SM.record(c, N, H, SM.saturating_window(), SM.SAT_SHIFT, N, 4 * H)
        assert np.array_equal(SM.wrapping_sum(rec), whole) and int(whole[SM.SAT_BIN]) == 0 and int(whole[N]) == 4
        assert int(SM.wrapping_sum(rec[:3])[SM.SAT_BIN]) == 3 << 62
        assert sum(int(v) for v in rec[:, SM.SAT_BIN]) == 1 << 64    # (as Python integers: the sum the words wrapped)


def test_the_saturating_scene_has_no_ambiguous_bin():
    """what tests/test_gpu_scan_edges.py's clamp test rests on, in all three formats: in every frame with full history bin 100's
    scaled power exceeds 2^62 by more than 3.0h's bound, so any conforming implementation clamps it; every other bin stays below
    2^62 by more than the bound, so none may; and the largest of those is above 2^61, so a clamp set one bit low would show"""
    cf = _converted(SM.saturating_capture())
    N, H, w = SM.SAT_N, SM.SAT_HOP, SM.saturating_window()
    for fmt, c in cf.items():
        X = SM.spectra(c, N, H, w, N, 4 * H)
        assert X.shape == (4, N)
        v = np.ldexp((X.real * X.real + X.imag * X.imag).astype(np.float32).astype(np.float64), SM.SAT_SHIFT)
        bound = SM.frame_bound(X, SM.delta(N, w, c), SM.SAT_SHIFT)
        others = np.arange(N) != SM.SAT_BIN
        assert (v[:, SM.SAT_BIN] - bound[:, SM.SAT_BIN] > 2.0 ** 62).all(), fmt
        assert (v[:, others] + bound[:, others] < 2.0 ** 62).all(), fmt
        top = v[:, others].max() / 2.0 ** 62
        print("%s: bin 100 at %.2f x 2^62, the largest other bin at %.3f x 2^62" % (fmt, v[:, SM.SAT_BIN].min() / 2.0 ** 62, top))
        assert 0.5 < top < 0.6
