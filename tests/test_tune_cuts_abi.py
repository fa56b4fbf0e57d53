"""CPU tests of the host side of the tuner's cuts (docs/SPEC.md 3.0j): the ABI surface, p25fe_cuts_from_keys against the Python
model (tests/tune_cuts_model.py) and its refusals, the refusals of p25fe_cuts_create that come before any device, and the model's
own consistency (a cut is a slice; slices of a split cut add up).  The GPU side is tests/test_gpu_tune_cuts.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import resample_model as RM
import tune_cuts_model as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"p25fe_cuts_from_keys", "p25fe_cuts_create", "p25fe_cuts_destroy", "p25fe_cuts_dev"}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from p25rx_amd import _lib
    return _lib


def _keys(lib, rows):
    """(raster_index, first_slot, n_slots, centre_hz, offset_hz) tuples -> the C records"""
    k = np.zeros(len(rows), dtype=lib.WATERFALL_KEY_DTYPE)
    for i, (r, first, cnt, centre, off) in enumerate(rows):
        k[i] = (r, 0, first, cnt, centre, off, 30.0)
    return k


def _from_keys(lib, keys, N, hop, B, fs, margin, r0, rn, cap=None):
    L = lib.load()
    cap = len(keys) if cap is None else cap
    out = np.zeros(max(cap, 1), dtype=lib.CUT_DTYPE)
    out["step"] = -7
    n = C.c_size_t(99)
    rc = L.p25fe_cuts_from_keys(keys.ctypes.data_as(C.c_void_p), len(keys), N, hop, B, fs, margin, r0, rn,
                                out.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    return rc, n.value, out


def test_abi_surface(lib):
    """header, ctypes and the Rust text name the same four functions; the record is 24 bytes; the ABI version has not moved"""
    hdr = open(os.path.join(ROOT, "include", "p25fe.h")).read()
    assert re.search(r"#define P25FE_ABI_VERSION 6\b", hdr) and lib.ABI_VERSION == 6
    assert re.search(r"#define P25FE_CUTS_MAX 4096\b", hdr) and lib.CUTS_MAX == CM.CUTS_MAX == 4096
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(p25fe_[a-z0-9_]+)\s*\(", code))
    assert NEW <= declared and NEW <= set(lib.SYMBOLS)
    assert {s for s in declared if "cuts" in s} == NEW
    rs = open(os.path.join(ROOT, "bindings", "p25fe.rs")).read()
    assert NEW <= set(re.findall(r"pub fn (p25fe_[a-z0-9_]+)\(", rs))
    L = lib.load()
    for s in NEW:
        assert getattr(L, s).argtypes is not None, s
    # sizeof(p25fe_cut_t) == 24: the header's fields, the ctypes record and the library's own stride
    m = re.search(r"typedef struct p25fe_cut \{(.*?)\} p25fe_cut_t;", code, re.S)
    fields = re.findall(r"(uint64_t|int32_t|uint32_t)\s+([a-z0-9_, ]+);", m.group(1))
    assert [(t, [v.strip() for v in names.split(",")]) for t, names in fields] == \
        [("uint64_t", ["abs_first", "n"]), ("int32_t", ["step"]), ("uint32_t", ["ph0"])]
    assert lib.CUT_DTYPE.itemsize == 24 and lib.CUT_DTYPE.names == ("abs_first", "n", "step", "ph0")
    keys = _keys(lib, [(1, 3, 2, 12500.0, 0.0), (2, 5, 2, 25000.0, 10.0)])
    rc, n, out = _from_keys(lib, keys, 4096, 2048, 6, 2500000, 0, 0, 1 << 30)
    assert rc == lib.OK and n == 2
    raw = out.view(np.uint8).reshape(-1, 24)                        # record j starts 24 bytes after record j - 1
    assert int(raw[1, :8].view("<u8")[0]) == 5 * 6 * 2048 + 2048 - 4096 and int(raw[1, 16:20].view("<i4")[0]) == CM.nco_step(2500000, 25010.0)


def test_from_keys_is_the_model(lib):
    """hand-made keys: slot 0 (clipped on the left), past the range (n = 0), on both of its edges, margins 0 and N, positions past
    2^40, frequencies on both sides and off the raster"""
    N, hop, B, fs = 4096, 2048, 6, 2500000
    slot = hop * B
    for N, hop, B in ((4096, 2048, 6), (1024, 8, 1), (4096, 4096, 1 << 20), (1024, 512, 3)):
        slot = hop * B
        for r0, rn in ((0, 625000), (5007, 300001), ((1 << 40) + 3, 48000), (0, 0), (3 * slot, slot)):
            s0 = r0 // slot
            rows = [(-33, 0, 51, -412500.0, 1871.3), (11, s0, 1, 137500.0, -2210.7), (12, s0 + 2, 20, 150000.0, -2411.6),
                    (40, s0 + 3, 1, 500000.0, 733.1), (0, (r0 + rn) // slot + 3, 4, 0.0, 0.0), (-1, s0 + 1000000, 7, -12500.0, 0.25),
                    (5, max(s0 - 9, 0), 2, 62500.0, -0.001), (99, (r0 + rn) // slot, 1, 1237500.0, 0.0), (7, 1 << 44, 1 << 20, 87500.0, 1.0)]
            keys = _keys(lib, rows)
            for margin in (0, N, 12345):
                want = CM.from_keys(rows, N, hop, B, fs, margin, r0, rn)
                rc, n, out = _from_keys(lib, keys, N, hop, B, fs, margin, r0, rn)
                assert rc == lib.OK and n == len(rows)
                got = [(int(c["abs_first"]), int(c["n"]), int(c["step"]), int(c["ph0"])) for c in out[:n]]
                assert got == want, (N, hop, B, r0, rn, margin, got, want)
                for a, cnt, _st, _ph in got:                         # inside the range, every one
                    assert r0 <= a and a + cnt <= r0 + rn
    # the cases by hand: the first frame of slot 0 starts at hop - N < 0; the last sample is (first + n) slot + hop - 1
    keys = _keys(lib, [(1, 0, 2, 12500.0, 0.0), (1, 60, 2, 12500.0, 0.0), (1, 4, 3, 12500.0, 0.0)])
    rc, n, out = _from_keys(lib, keys, 4096, 2048, 6, 2500000, 0, 0, 625000)
    assert [(int(c["abs_first"]), int(c["n"])) for c in out[:3]] == [(0, 2 * 12288 + 2048), (625000, 0), (4 * 12288 - 2048, 3 * 12288 + 4096)]
    rc, n, out = _from_keys(lib, keys, 4096, 2048, 6, 2500000, 4096, 0, 625000)
    assert [(int(c["abs_first"]), int(c["n"])) for c in out[:3]] == [(0, 2 * 12288 + 2048 + 4096), (625000, 0),
                                                                     (4 * 12288 - 2048 - 4096, 3 * 12288 + 4096 + 8192)]
    assert int(out[0]["step"]) == CM.nco_step(2500000, 12500.0) == 21474836 and int(out[0]["ph0"]) == 0
    # no keys: nothing to do, and no pointer needed
    n = C.c_size_t(5)
    assert lib.load().p25fe_cuts_from_keys(None, 0, 4096, 2048, 6, 2500000, 0, 0, 100, None, 0, C.byref(n)) == lib.OK and n.value == 0


def test_from_keys_refusals(lib):
    """the survey's shape refusals, a frequency past Nyquist or not finite, positions of 2^62 and beyond, null pointers: nothing is
    written; a capacity below the key count is P25FE_ERR_CAPACITY with the count"""
    L = lib.load()
    good = [(1, 3, 2, 12500.0, 0.0), (2, 5, 2, 25000.0, 10.0)]
    keys = _keys(lib, good)

    def refused(k=keys, N=4096, hop=2048, B=6, fs=2500000, margin=0, r0=0, rn=625000):
        rc, n, out = _from_keys(lib, k, N, hop, B, fs, margin, r0, rn)
        assert (out["step"] == -7).all() and n == 0
        return rc == lib.ERR_ARG
    assert _from_keys(lib, keys, 4096, 2048, 6, 2500000, 0, 0, 625000)[0] == lib.OK
    for N in (0, 512, 2048, 4095, 8192, -4096):
        assert refused(N=N), N
    for hop in (0, 4, 12, 2047, 3000, 8192, -8):
        assert refused(hop=hop), hop
    assert refused(N=1024, hop=2048) and _from_keys(lib, keys, 1024, 1024, 1, 2500000, 0, 0, 100)[0] == lib.OK
    for B in (0, (1 << 20) + 1, (1 << 32) - 1):
        assert refused(B=B), B
    assert refused(fs=0)
    for big in (1 << 62, (1 << 64) - 1):
        assert refused(margin=big) and refused(r0=big) and refused(rn=big), big
    assert _from_keys(lib, keys, 4096, 2048, 6, 2500000, (1 << 62) - 1, (1 << 62) - 1, (1 << 62) - 1)[0] == lib.OK
    for centre, off in ((1250000.0, 0.5), (-1250000.0, -0.5), (float("nan"), 0.0), (0.0, float("inf")), (1e300, 0.0)):
        assert refused(k=_keys(lib, good + [(3, 1, 1, centre, off)])), (centre, off)
    assert _from_keys(lib, _keys(lib, good + [(3, 1, 1, 1250000.0, 0.0)]), 4096, 2048, 6, 2500000, 0, 0, 625000)[0] == lib.OK   # Nyquist itself
    n = C.c_size_t(5)
    out = np.zeros(2, dtype=lib.CUT_DTYPE)
    kp, op = keys.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert L.p25fe_cuts_from_keys(kp, 2, 4096, 2048, 6, 2500000, 0, 0, 100, op, 2, None) == lib.ERR_ARG
    assert L.p25fe_cuts_from_keys(None, 2, 4096, 2048, 6, 2500000, 0, 0, 100, op, 2, C.byref(n)) == lib.ERR_ARG and n.value == 0
    assert L.p25fe_cuts_from_keys(kp, 2, 4096, 2048, 6, 2500000, 0, 0, 100, None, 2, C.byref(n)) == lib.ERR_ARG and n.value == 0
    # capacity: the count, and nothing written
    rc, cnt, o = _from_keys(lib, keys, 4096, 2048, 6, 2500000, 0, 0, 625000, cap=1)
    assert rc == lib.ERR_CAPACITY and cnt == 2 and (o["step"] == -7).all()
    assert L.p25fe_cuts_from_keys(kp, 2, 4096, 2048, 6, 2500000, 0, 0, 100, None, 0, C.byref(n)) == lib.ERR_CAPACITY and n.value == 2


def test_create_checks_its_arguments_before_any_device(lib):
    """p25fe_cuts_create's refusals with no tuner at all (the tuner is looked at last, so a list that passes every check is refused
    BECAUSE there is none); p25fe_cuts_dev and p25fe_cuts_destroy on a null object"""
    L = lib.load()
    out = C.c_void_p(1)
    mx = C.c_size_t(77)

    def create(cuts, n=None, cuts_p=0, out_p=0):
        c = np.array(cuts, dtype=lib.CUT_DTYPE)
        out.value, mx.value = 1, 77
        return L.p25fe_cuts_create(None, c.ctypes.data_as(C.c_void_p) if cuts_p == 0 else cuts_p, len(c) if n is None else n, None,
                                   C.byref(mx), C.byref(out) if out_p == 0 else out_p)
    one = [(100, 5000, 12345, 0)]
    assert create(one, n=0) == lib.ERR_ARG and not out.value and mx.value == 0
    assert create(one * 4097) == lib.ERR_ARG and not out.value
    assert create(one, cuts_p=None) == lib.ERR_ARG and not out.value
    assert create(one, out_p=None) == lib.ERR_ARG
    for bad in ((1 << 62, 1, 0, 0), (5, 1 << 62, 0, 0), ((1 << 64) - 1, (1 << 64) - 1, 0, 0)):
        assert create(one + [bad]) == lib.ERR_ARG and not out.value, bad
    # everything right but the tuner: every step and phase offset, lengths 0 and 2^62 - 1, 4096 cuts
    assert create([(0, 0, 0, 0), ((1 << 62) - 1, (1 << 62) - 1, -(1 << 31), (1 << 32) - 1), (7, 9, 0x7fffffff, 1)]) == lib.ERR_ARG and not out.value
    assert create(one * 4096) == lib.ERR_ARG and not out.value and mx.value == 0
    assert L.p25fe_cuts_dev(None, None, 0, 0, 0, 0, None, 0, None) == lib.ERR_ARG
    L.p25fe_cuts_destroy(None)


def test_the_model_is_consistent():
    """slices of a cut split at any sample are adjacent and add up to the cut's; a cut's slice lies inside the call's row; the
    workgroup counts follow the sub-tile of the two designed tables (12/125, T 84: R > 1; 3/125, T 334: R = 1, tile < gl)"""
    assert CM.tile(12, 125, 84) == 180 and CM.tile(3, 125, 334) == 41 and CM.tile(24, 25, 9) == 192
    rng = np.random.default_rng(3)
    for L, M in ((12, 125), (3, 125), (15, 128)):
        for _ in range(200):
            call = int(rng.integers(0, 1 << 45))
            a = call + int(rng.integers(0, 5000))
            n = int(rng.integers(0, 4000))
            s = int(rng.integers(0, n + 1))
            m0, cnt = CM.slice_of(L, M, call, a, n)
            m1, c1 = CM.slice_of(L, M, call, a, s)
            m2, c2 = CM.slice_of(L, M, call, a + s, n - s)
            assert (m1, m1 + c1, c1 + c2) == (m0, m2, cnt)
            assert m0 + cnt <= RM.n_resample(L, M, call, a + n - call)
    cuts = [(0, 0, 0, 0), (8, 2, 0, 0), (7, 7500, 0, 0), (7, 7511, 0, 0), (0, 22500, 0, 0)]
    assert CM.wg_counts(12, 125, 84, cuts) == [0, 0, 1, 2, 3] and RM.n_resample(12, 125, 7, 7500) == 720 == 4 * CM.tile(12, 125, 84)
