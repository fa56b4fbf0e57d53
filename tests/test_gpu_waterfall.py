"""The survey over time on the GPU (docs/SPEC.md 3.0i: k_waterfall), through the C ABI, against tests/waterfall_model.py and against
the survey itself (3.0h: k_scan, one frame per call -- tests/scan_model.py's scan_frames).

A frame's quantised values are k_scan's and the sums are integers, so everything but the comparison with the numpy model is bit for
bit: B = 1 rows against the per-frame records, slots whose boundaries fall at every place in a batch, splits of a range (inside a
slot too), the wrapping sum of the rows against p25fe_scan_dev's record, positions past 2^40, rows that keep their padding and
their neighbours, about a thousand workgroups, the host streaming form mixed with p25fe_scan, and the keyed scene.  The only
tolerance is 3.0h's per-frame bound (test 1).  Shapes and captures are tests/test_gpu_scan_edges.py's.
Every B here is below the batch F; slots spanning workgroups, the u8 table, two streams, wrapping rows: test_gpu_waterfall_edges.py.

Largest error observed on an MI355X as a fraction of the per-frame bound: see docs/MEASUREMENTS.md, "Survey over time"."""
import ctypes as C

import numpy as np
import pytest

import scan_model as SM
import waterfall_model as WM
from test_gpu_scan import SHIFT, words
from test_gpu_scan_edges import SHAPES, case, first_frame, gpu_frames
from test_gpu_wide_fmt import conv, dev

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A5A5A5A5A
B1_CASES = [(s, f) for s in ("N1024_H64", "N1024_H256", "N4096_H64", "N4096_H1024") for f in ("cf32", "s16", "u8")
            if f == "cf32" or s in ("N1024_H64", "N4096_H64")]


@pytest.fixture(scope="module")
def mods():
    from p25rx_amd import _lib, Scanner
    from p25rx_amd.frontend import FrontEnd
    return _lib, FrontEnd, Scanner


def rows_of(t):
    """int64 device rows -> uint64 [n_rows, width] on the host"""
    return t.cpu().numpy().view(np.uint64).copy()


def summed(rows, N):
    return SM.wrapping_sum(rows[:, :N + 1])


# ---- 1. B = 1: a row is that frame's record ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,fmt", B1_CASES)
def test_one_frame_per_slot_is_the_frames_record(mods, shape, fmt):
    """one launch over the shape's range with B = 1: row i equals p25fe_scan_dev's record of frame f0 + i alone in all 8 (N + 1)
    bytes, and every word is within 3.0h's per-frame bound of the model"""
    _lib, FE, Scanner = mods
    c = case(*SHAPES[shape])
    f0 = first_frame(c)
    at = f0 * c.hop
    sc = Scanner(FE(), c.N, c.hop, shift=SHIFT)
    got = rows_of(sc.waterfall_dev(dev(c.raw[fmt]), 1, n_hist=c.N - 1, abs0=at, offset=at, n=c.frames * c.hop))
    assert got.shape == (c.frames, c.N + 1) and (got[:, c.N] == 1).all()
    rec = gpu_frames(mods, shape, fmt)
    assert np.array_equal(got, rec), np.argwhere(got != rec)[:8]
    X = SM.spectra(c.cf[fmt], c.N, c.hop, c.w, at, c.frames * c.hop)
    ref = SM.quantise(X, SHIFT)                                      # (below 2^53: exact in double, and so is the difference)
    bound = SM.frame_bound(X, SM.delta(c.N, c.w, c.cf[fmt]), SHIFT)
    err = np.abs(got[:, :c.N].astype(np.float64) - ref)
    frac = err / bound
    f, b = np.unravel_index(int(frac.argmax()), frac.shape)
    print("%s %s: largest error %.4f of the per-frame bound (row %d of %d, bin %d: |error| %.0f of %.0f)"
          % (shape, fmt, frac.max(), f, c.frames, b, err[f, b], bound[f, b]))
    assert ref.max() > 2.0 ** 30                                     # the tones are there
    assert (err <= bound).all(), np.argwhere(err > bound)[:8]


# ---- 2. slot boundaries at every place in a batch -------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 5, 7])
@pytest.mark.parametrize("shape,fmt", [("N1024_H64", "cf32"), ("N4096_H64", "u8"), ("N1024_H256", "cf32")])
def test_slot_boundaries_at_every_place_in_a_batch(mods, shape, fmt, B):
    """B coprime to the batch (8, 16, 64 or 256 frames): a slot's boundary falls at every place in a batch, batches end inside
    slots, the first and the last slot are partial.  Rows = the per-frame records summed by f // B, word N the frames per slot"""
    _lib, FE, Scanner = mods
    c = case(*SHAPES[shape])
    rec = gpu_frames(mods, shape, fmt)
    f0 = first_frame(c)
    lo = 1 if (f0 + 1) % B else 2                                    # frames dropped in front, so that the first slot is partial
    hi = c.frames - (1 if (f0 + c.frames - 1) % B else 2)            # ... and the last
    fa, k = f0 + lo, hi - lo
    assert fa % B and (fa + k) % B and k > 2 * B
    sc = Scanner(FE(), c.N, c.hop, shift=SHIFT)
    got = rows_of(sc.waterfall_dev(dev(c.raw[fmt]), B, n_hist=c.N - 1, abs0=fa * c.hop, offset=fa * c.hop, n=k * c.hop))
    slot0, ref = WM.group(rec[lo:hi], fa, B)
    assert Scanner.slots(c.hop, B, fa * c.hop, k * c.hop) == (slot0, ref.shape[0])
    assert got.shape == ref.shape and np.array_equal(got, ref), np.argwhere(got != ref)[:8]
    per = [min((slot0 + i + 1) * B, fa + k) - max((slot0 + i) * B, fa) for i in range(ref.shape[0])]
    assert list(got[:, c.N]) == per and per[0] < B and per[-1] < B and sum(per) == k


# ---- 3. splits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["cf32", "s16", "u8"])
@pytest.mark.parametrize("N,hop", [(1024, 64), (4096, 512)])
def test_splits_and_the_sum_of_the_rows(mods, N, hop, fmt):
    """a range of 10 frames and 5 samples, d samples off the loader's vectors (d = 0 and odd values), B = 4: the same rows from one
    call, from two and from three (cuts at multiples of 8 samples, one of them inside a slot and inside a hop); their wrapping
    sum equals p25fe_scan_dev's record of the range"""
    _lib, FE, Scanner = mods
    c = case(N, hop, 12)
    sc = Scanner(FE(), N, hop, shift=SHIFT)
    t = dev(c.raw[fmt])
    B, offset, n = 4, N + 8, 10 * hop + 5
    import torch
    for d in {"u8": (0, 3, 7), "s16": (0, 1, 3), "cf32": (0, 1)}[fmt]:
        abs0 = offset + d
        slot0, n_rows = Scanner.slots(hop, B, abs0, n)
        assert n_rows >= 3
        one = rows_of(sc.waterfall_dev(t, B, n_hist=offset, abs0=abs0, offset=offset, n=n))
        assert one.shape == (n_rows, N + 1) and int(one[:, N].sum()) == 10
        whole = words(sc.scan_dev(t, n_hist=offset, abs0=abs0, offset=offset, n=n))
        assert np.array_equal(summed(one, N), whole), d
        for cuts in ((5 * hop + 8,), (8, 2 * hop + 3 * hop // 4 + (8 if hop == 64 else 0))):
            rows = torch.zeros((n_rows, N + 1), dtype=torch.int64, device=t.device)
            edges = (0,) + cuts + (n,)
            for a, b in zip(edges[:-1], edges[1:]):
                assert a % 8 == 0 and (abs0 + a) % 8 == d
                n_hist = N - 1 if len(cuts) == 2 else offset + a     # exactly what continuation needs, or everything there is
                sc.waterfall_dev(t, B, n_hist=n_hist, abs0=abs0 + a, offset=offset + a, n=b - a, rows=rows, slot0=slot0)
            assert np.array_equal(rows_of(rows), one), (d, cuts)
        # a cut inside a slot: the two pieces touch the same row
        a = cuts[-1]
        assert Scanner.slots(hop, B, abs0, a)[1] and sum(Scanner.slots(hop, B, abs0 + x, y)[1] for x, y in ((0, a), (a, n - a))) == n_rows + 1


# ---- 4. positions ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,d", [("cf32", 1), ("s16", 3), ("u8", 5)])
def test_positions_past_two_to_the_forty(mods, fmt, d):
    """abs_first = 2^40 + 8 k + d with slot0 = f0 // B gives the rows of the same samples at a small position with the same
    f0 mod B and the same place in a hop, bit for bit; rows handed over with a stride of N + 5 and a guard row on each side keep
    their padding and their neighbours; slot0 one too high and n_rows one too low are P25FE_ERR_CAPACITY and write nothing"""
    import torch
    _lib, FE, Scanner = mods
    N, hop, B = 1024, 64, 5
    c = case(N, hop, 70)
    sc = Scanner(FE(), N, hop, shift=SHIFT)
    t = dev(c.raw[fmt])
    offset, n = N + 8, 33 * hop + 40
    small = offset + d
    big = small + -(-(1 << 40) // (hop * B)) * hop * B                # the same place in a hop, the same f0 mod B
    assert big > 1 << 40 and (big - (1 << 40)) % 8 == d and (big // hop) % B == (small // hop) % B and big % hop == small % hop
    ref = rows_of(sc.waterfall_dev(t, B, n_hist=offset, abs0=small, offset=offset, n=n))
    slot0, n_rows = Scanner.slots(hop, B, big, n)
    assert slot0 == big // hop // B > 1 << 30 and n_rows == ref.shape[0] >= 7

    def poisoned():
        return torch.full((n_rows + 2, N + 5), POISON, dtype=torch.int64, device=t.device)
    buf = poisoned()
    sc.waterfall_dev(t, B, n_hist=offset, abs0=big, offset=offset, n=n, rows=buf[1:-1], slot0=slot0)
    got = rows_of(buf)
    assert (got[0] == POISON).all() and (got[-1] == POISON).all() and (got[1:-1, N + 1:] == POISON).all()
    assert np.array_equal(got[1:-1, :N + 1] - np.uint64(POISON), ref)          # (uint64 arithmetic wraps)
    # a second call adds, and still leaves the padding and the guards alone
    sc.waterfall_dev(t, B, n_hist=offset, abs0=big, offset=offset, n=n, rows=buf[1:-1], slot0=slot0)
    got = rows_of(buf)
    assert (got[0] == POISON).all() and (got[-1] == POISON).all() and (got[1:-1, N + 1:] == POISON).all()
    assert np.array_equal(got[1:-1, :N + 1] - np.uint64(POISON), ref + ref)
    for kw in (dict(rows=slice(1, -1), slot0=slot0 + 1), dict(rows=slice(1, -2), slot0=slot0), dict(rows=slice(1, -1), slot0=slot0 - n_rows),
               dict(rows=slice(1, 2), slot0=slot0 + 1)):
        buf = poisoned()
        with pytest.raises(_lib.P25feError) as e:
            sc.waterfall_dev(t, B, n_hist=offset, abs0=big, offset=offset, n=n, rows=buf[kw["rows"]], slot0=kw["slot0"])
        assert e.value.status == _lib.ERR_CAPACITY, kw
        torch.cuda.synchronize()
        assert (rows_of(buf) == POISON).all(), kw
    # a range that owns no frame writes nothing and needs no row
    buf = poisoned()
    at = (big // hop + 1) * hop - 40
    sc.waterfall_dev(t, B, n_hist=offset, abs0=at, offset=offset, n=39, rows=buf[1:1], slot0=0)
    torch.cuda.synchronize()
    assert (rows_of(buf) == POISON).all() and Scanner.slots(hop, B, at, 39)[1] == 0


# ---- 5. many workgroups -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,frames", [(8, 9230), (512, 9221)])
def test_many_workgroups(mods, hop, frames):
    """N = 1024, B = 7 over random bytes from position 0: hop 8 with 9230 frames (19 workgroups of 512 frames: 73 slots and more
    inside each batch) and hop 512 with 9221 (923 workgroups of 10 frames: a slot's boundary in most batches, many batches inside
    one slot never).  The wrapping sum of the rows equals the one-call record; every 50th row equals p25fe_scan_dev over that
    slot's range"""
    _lib, FE, Scanner = mods
    N, B = 1024, 7
    raw = np.random.default_rng(frames).integers(0, 256, size=2 * (frames * hop + 5), dtype=np.uint8)
    t = dev(raw)
    sc = Scanner(FE(), N, hop, shift=SHIFT)
    rows = rows_of(sc.waterfall_dev(t, B))
    n_rows = -(-frames // B)
    assert rows.shape == (n_rows, N + 1)
    assert list(rows[:, N]) == [B] * (frames // B) + ([frames % B] if frames % B else [])
    whole = words(sc.scan_dev(t))
    assert int(whole[N]) == frames and np.array_equal(summed(rows, N), whole)
    for i in list(range(0, n_rows, 50)) + [n_rows - 1]:
        a, b = i * B * hop, min((i + 1) * B * hop, frames * hop + 5)
        one = words(sc.scan_dev(t, n_hist=a, abs0=a, offset=a, n=b - a))
        assert np.array_equal(rows[i], one), i


# ---- 6. the host streaming form ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["u8", "cf32"])
def test_host_streaming(mods, fmt):
    """p25fe_waterfall at N = 1024, hop 64, B = 3 in chunks of odd sizes equals one p25fe_waterfall_dev over the capture; mixed
    with p25fe_scan on the same object every call's frames go where that call sends them; p25fe_scan_reset starts over with zeroed
    rows; a call that would pass the last row is P25FE_ERR_CAPACITY and consumes nothing, behind the argument and format checks;
    p25fe_scan past the last row, or an open on a stream already past it, leaves the read at the rows there are"""
    _lib, FE, Scanner = mods
    c = case(*SHAPES["N1024_H64"])
    N, hop, B = c.N, c.hop, 3
    raw = c.raw[fmt]
    n = len(c.cf[fmt])
    per = 1 if fmt == "cf32" else 2
    t = dev(raw)
    sc = Scanner(FE(), N, hop, shift=SHIFT)
    whole = rows_of(sc.waterfall_dev(t, B))
    n_rows = -(-(n // hop) // B)
    assert whole.shape == (n_rows, N + 1) and int(whole[:, N].sum()) == n // hop
    with pytest.raises(_lib.P25feError) as e:                        # no open yet
        sc.waterfall(raw[:per * 8])
    assert e.value.status == _lib.ERR_ARG
    with pytest.raises(_lib.P25feError) as e:
        sc.read_waterfall()
    assert e.value.status == _lib.ERR_ARG
    edges = np.concatenate([[0], np.cumsum([1, 3, 7, 63, 64, 65, 1000, 0, 191, 193, 577]), [n]])
    sc.open_waterfall(B, n_rows)
    assert sc.read_waterfall().shape == (0, N + 1)
    for a, b in zip(edges[:-1], edges[1:]):
        sc.waterfall(raw[per * a:per * b])
    assert np.array_equal(sc.read_waterfall(), whole)
    assert not sc.read().any()                                       # the object's own record was not touched
    # reset: zeroed rows, position 0; then mixed with p25fe_scan -- odd calls into the rows, even calls into the record.  The
    # reference: the per-frame rows (B = 1, test 1), each frame going where the call that owns it sends it
    sc.reset()
    assert sc.read_waterfall().shape == (0, N + 1)
    frames = rows_of(sc.waterfall_dev(t, 1))
    assert frames.shape == (n // hop, N + 1)
    ref_rows, ref_acc = np.zeros_like(whole), np.zeros(N + 1, dtype=np.uint64)
    for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        own = range(a // hop, b // hop)
        if i % 2:
            sc.waterfall(raw[per * a:per * b])
            for f in own:
                ref_rows[f // B] += frames[f]
        else:
            sc.scan(raw[per * a:per * b])
            for f in own:
                ref_acc += frames[f]
    got = sc.read_waterfall()
    assert ref_rows[:, N].sum() > 20 and ref_acc[N] > 20
    assert got.shape == whole.shape and np.array_equal(got, ref_rows) and not np.array_equal(got, whole)
    assert np.array_equal(sc.read(), ref_acc)
    assert np.array_equal(summed(got, N) + ref_acc, summed(whole, N))
    # past the last row: a second open replaces the first, with one row too few for the whole capture
    sc.reset()
    sc.open_waterfall(B, n_rows - 1)
    cut = (n_rows - 1) * B * hop - 1                                 # one sample short of the end of the last frame that has a row
    sc.waterfall(raw[:per * cut])
    before = sc.read_waterfall()
    assert before.shape == (n_rows - 1, N + 1) and np.array_equal(before[:-1], whole[:n_rows - 2]) and int(before[-1, N]) == B - 1
    with pytest.raises(_lib.P25feError) as e:
        sc.waterfall(raw[per * cut:per * n])
    assert e.value.status == _lib.ERR_CAPACITY
    assert np.array_equal(sc.read_waterfall(), before)
    sc.waterfall(raw[per * cut:per * (cut + 1)])                     # nothing was consumed: this sample completes the last row
    assert np.array_equal(sc.read_waterfall(), whole[:n_rows - 1])
    with pytest.raises(_lib.P25feError) as e:
        sc.waterfall(raw[per * (cut + 1):per * (cut + 1 + hop)])     # the next frame has no row
    assert e.value.status == _lib.ERR_CAPACITY
    assert np.array_equal(sc.read_waterfall(), whole[:n_rows - 1])
    # the arguments and the format are looked at before the rows: the same call with no samples or in another format
    fmt_id, other = (_lib.FMT_CF32, _lib.FMT_U8) if fmt == "cf32" else (_lib.FMT_U8, _lib.FMT_CF32)
    some = np.zeros(8 * hop, dtype=np.uint8)
    assert sc.lib.p25fe_waterfall(sc.sc, None, fmt_id, hop) == _lib.ERR_ARG
    assert sc.lib.p25fe_waterfall(sc.sc, some.ctypes.data_as(C.c_void_p), 7, hop) == _lib.ERR_ARG
    assert sc.lib.p25fe_waterfall(sc.sc, some.ctypes.data_as(C.c_void_p), other, hop) == _lib.ERR_FORMAT
    assert sc.lib.p25fe_waterfall(sc.sc, some.ctypes.data_as(C.c_void_p), fmt_id, hop) == _lib.ERR_CAPACITY
    # p25fe_scan moves the same position and has no last row: past it the read still gives the rows there are, no more
    sc.scan(raw[per * (cut + 1):per * n])
    count = C.c_size_t(0)
    assert sc.lib.p25fe_waterfall_read(sc.sc, None, 0, C.byref(count)) == _lib.ERR_CAPACITY and count.value == n_rows - 1
    got = sc.read_waterfall()
    assert got.shape == (n_rows - 1, N + 1) and np.array_equal(got, whole[:n_rows - 1])
    assert int(sc.read()[N]) == n // hop - (n_rows - 1) * B         # (the record took the frames the rows could not)
    with pytest.raises(_lib.P25feError) as e:
        sc.waterfall(raw[:per * hop])
    assert e.value.status == _lib.ERR_CAPACITY
    sc.waterfall(raw[:per * 8])                                      # a call that owns no frame needs no row
    # an open on a stream that is already past the rows it asks for: they are there, zeroed, and no others
    sc.open_waterfall(B, 2)
    got = sc.read_waterfall()
    assert got.shape == (2, N + 1) and not got.any()
    guard = np.full((3, N + 1), POISON, dtype=np.uint64)
    assert sc.lib.p25fe_waterfall_read(sc.sc, guard.ctypes.data_as(C.c_void_p), 3, C.byref(count)) == _lib.OK and count.value == 2
    assert not guard[:2].any() and (guard[2] == POISON).all()
    for bad in ((0, 4), ((1 << 20) + 1, 4), (B, 0), (B, (1 << 20) + 1)):
        with pytest.raises(_lib.P25feError) as e:
            sc.open_waterfall(*bad)
        assert e.value.status == _lib.ERR_ARG, bad


# ---- 7. the keyed scene --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["cf32", "u8"])
def test_the_keyed_scene(mods, fmt):
    """tests/waterfall_model.py's scene (tests/test_waterfall_abi.py holds the model's numbers for it) in one launch: the keys of
    the GPU's rows have the integer fields of the keys of the model's rows -- the five intervals --, and offsets within 200 Hz
    of the truth"""
    _lib, FE, Scanner = mods
    x = WM.keyed_scene()
    raw = x if fmt == "cf32" else SM.to_u8(x)
    cf = x if fmt == "cf32" else conv(raw)
    sc = Scanner(FE(), WM.KEY_N, WM.KEY_HOP, shift=WM.KEY_SHIFT)
    rows = rows_of(sc.waterfall_dev(dev(raw), WM.KEY_B))
    slot0, model = WM.rows(cf, WM.KEY_N, WM.KEY_HOP, SM.window(WM.KEY_N), WM.KEY_SHIFT, WM.KEY_B)
    assert slot0 == 0 and rows.shape == model.shape == (51, WM.KEY_N + 1) and np.array_equal(rows[:, WM.KEY_N], model[:, WM.KEY_N])
    got = Scanner.keys(rows, WM.KEY_FS)
    ref = WM.keys(model, WM.KEY_N, WM.KEY_FS)
    truth = WM.keyed_truth()
    assert len(got) == len(ref) == len(truth) == 5
    for k, m, (r, a, b, off) in zip(got, ref, truth):
        assert (int(k["raster_index"]), int(k["first_slot"]), int(k["n_slots"])) == (m[0], m[1], m[2]), (k, m)
        assert int(k["raster_index"]) == r and abs(int(k["first_slot"]) - a) <= 1
        assert abs(int(k["first_slot"]) + int(k["n_slots"]) - 1 - b) <= 1
        print("%s r %d slots %d .. %d: offset %.1f Hz (true %.1f), %.1f dB over the floor"
              % (fmt, r, k["first_slot"], k["first_slot"] + k["n_slots"] - 1, k["offset_hz"], off, k["peak_db_over_floor"]))
        assert abs(k["offset_hz"] - off) <= 200.0, (k, off)
