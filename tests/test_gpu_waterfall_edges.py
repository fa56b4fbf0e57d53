"""The survey over time on the GPU (docs/SPEC.md 3.0i: k_waterfall) where tests/test_gpu_waterfall.py does not go: slots LONGER
than a workgroup's batch F (there every B is below F), so that a row is assembled from three and more workgroups, whole batches lie
inside one slot and flush with the slot's countdown still running, and a workgroup's first frame lies deep inside a slot; about a
thousand workgroups adding into ten rows and into one; the u8 table instantiations; two launches adding into the same rows from two
streams at once; rows that wrap modulo 2^64; rows between two disjoint calls; slots past 2^30.

The reference is a chain of three, so that a defect in one frame or in one flush cannot hide in a sum: (1) rows against
WM.group of the GPU's per-frame records (k_scan, one frame per call: SM.scan_frames), bit for bit in all 8 (N + 1) bytes -- a
frame's quantised values are k_scan's and integer sums commute; (2) those per-frame records against the double-precision model,
frame by frame and bin by bin, under 3.0h's bound, the only tolerance here; (3) the model's largest value is above 2^30.  Every test
asserts its own premise with WM.batch (the kernel's F) and WM.contributors (which workgroups add into which row).

Largest error observed on an MI355X as a fraction of the per-frame bound: see docs/MEASUREMENTS.md, "Survey over time"."""
import numpy as np
import pytest

import scan_model as SM
import waterfall_model as WM
from test_gpu_scan import SHIFT, words
from test_gpu_scan_edges import case, first_frame, within
from test_gpu_waterfall import POISON, rows_of, summed
from test_gpu_wide_fmt import conv, dev

pytestmark = pytest.mark.gpu

# N, hop, frames of one call -> F; the last is the shape of tools/waterfall_time.py and of the keyed scene
SHAPES = {"N1024_H512": (1024, 512, 70), "N1024_H256": (1024, 256, 70), "N4096_H1024": (4096, 1024, 70), "N4096_H2048": (4096, 2048, 40)}
BATCH = {"N1024_H512": 8, "N1024_H256": 16, "N4096_H1024": 16, "N4096_H2048": 8}
ALL_FORMATS = ("N1024_H512", "N4096_H2048")
CASES = [(s, f) for s in SHAPES for f in ("cf32", "s16", "u8") if f == "cf32" or s in ALL_FORMATS]
M64 = 1 << 64


@pytest.fixture(scope="module")
def mods():
    from p25rx_amd import _lib, Scanner
    from p25rx_amd.frontend import FrontEnd
    return _lib, FrontEnd, Scanner


_FRAMES, _STREAMS = {}, []


def frames_of(key, make):
    """the GPU's per-frame records of one capture, made once and never written: uint64 [frames, N + 1]"""
    if key not in _FRAMES:
        _FRAMES[key] = make()
        _FRAMES[key].setflags(write=False)
    return _FRAMES[key]


def gpu_frames(mods, shape, fmt):
    _lib, FE, Scanner = mods
    c = case(*SHAPES[shape])

    def make():
        return SM.scan_frames(Scanner(FE(), c.N, c.hop, shift=SHIFT), dev(c.raw[fmt]), first_frame(c), c.frames)
    return frames_of((shape, fmt), make)


def feeds(con):
    """WM.contributors' rows -> per workgroup, in order, the rows it adds into"""
    out = [[] for _ in range(1 + max(max(s) for s in con))]
    for i, s in enumerate(con):
        for g in s:
            out[g].append(i)
    return out


def start(c, B, ok, hi=None):
    """the fewest leading frames to drop from the shape's range so that the first slot is partial and ok(contributors) holds"""
    f0, hi = first_frame(c), c.frames if hi is None else hi
    for lo in range(hi):
        if (f0 + lo) % B and ok(WM.contributors(f0 + lo, hi - lo, WM.batch(c.N, c.hop, hi - lo), B)):
            return lo
    raise AssertionError("no start of this shape does what the test is about")


def launch(mods, shape, fmt, B, lo, hi):
    """one launch over the frames lo .. hi - 1 of the shape's range against WM.group of their per-frame records: all words of all
    rows, and the slots the library names -> (rows, contributors, the Scanner, the device capture, first frame, frames)"""
    _lib, FE, Scanner = mods
    c = case(*SHAPES[shape])
    rec = gpu_frames(mods, shape, fmt)
    fa, k = first_frame(c) + lo, hi - lo
    F = WM.batch(c.N, c.hop, k)
    assert F == BATCH[shape] and k > 0
    sc = Scanner(FE(), c.N, c.hop, shift=SHIFT)
    t = dev(c.raw[fmt])
    got = rows_of(sc.waterfall_dev(t, B, n_hist=c.N - 1, abs0=fa * c.hop, offset=fa * c.hop, n=k * c.hop))
    slot0, ref = WM.group(rec[lo:hi], fa, B)
    assert Scanner.slots(c.hop, B, fa * c.hop, k * c.hop) == WM.slots(c.hop, B, fa * c.hop, k * c.hop) == (slot0, ref.shape[0])
    assert got.shape == ref.shape == (ref.shape[0], c.N + 1)
    assert np.array_equal(got, ref), (B, lo, hi, np.argwhere(got != ref)[:8])
    assert int(got[:, c.N].sum()) == k
    con = WM.contributors(fa, k, F, B)
    assert len(con) == got.shape[0] and len(feeds(con)) == -(-k // F)
    return got, con, sc, t, fa, k


# ---- 1. slots that span workgroups ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,fmt", CASES)
def test_the_per_frame_records_of_the_new_shapes(mods, shape, fmt):
    """steps 2 and 3 of the chain: p25fe_scan_dev's record of every frame of the shape's range by itself against Q(P_f[b]) of the
    model, frame by frame and bin by bin under 3.0h's bound; word N is 1; the tones are there"""
    c = case(*SHAPES[shape])
    rec = gpu_frames(mods, shape, fmt)
    at = first_frame(c) * c.hop
    X = SM.spectra(c.cf[fmt], c.N, c.hop, c.w, at, c.frames * c.hop)
    assert rec.shape == (c.frames, c.N + 1) == (X.shape[0], X.shape[1] + 1) and (rec[:, c.N] == 1).all()
    ref = SM.quantise(X, SHIFT)                                      # (below 2^53: exact in double, and so is the difference)
    bound = SM.frame_bound(X, SM.delta(c.N, c.w, c.cf[fmt]), SHIFT)
    err = np.abs(rec[:, :c.N].astype(np.float64) - ref)
    frac = err / bound
    f, b = np.unravel_index(int(frac.argmax()), frac.shape)
    print("%s %s: largest error %.4f of the per-frame bound (frame %d of %d, bin %d: |error| %.0f of %.0f)"
          % (shape, fmt, frac.max(), f, c.frames, b, err[f, b], bound[f, b]))
    assert ref.max() > 2.0 ** 30                                     # the tones are there
    assert (err <= bound).all(), np.argwhere(err > bound)[:8]


@pytest.mark.parametrize("shape,fmt", CASES)
def test_a_slot_one_frame_longer_than_a_batch(mods, shape, fmt):
    """B = F + 1, the first slot partial: every complete row is fed by two workgroups, a slot's boundary falls inside batches
    (those workgroups flush twice), and one whole batch lies inside one slot (it flushes once, at its end, with the slot's
    countdown still running or just run out)"""
    c = case(*SHAPES[shape])
    B = BATCH[shape] + 1

    def ok(con):
        n = [len(r) for r in feeds(con)]
        return 1 in n[:-1] and 2 in n
    got, con, _sc, _t, fa, k = launch(mods, shape, fmt, B, start(c, B, ok), c.frames)
    assert fa % B and k > 2 * B
    full = [i for i in range(len(con)) if int(got[i, c.N]) == B]
    assert len(full) >= 2 and all(len(con[i]) == 2 for i in full)
    n = [len(r) for r in feeds(con)]
    assert 1 in n[:-1] and 2 in n                                    # (n[:-1]: workgroups of F frames; the last may be short)


@pytest.mark.parametrize("r", ["on", "after", "before"])
@pytest.mark.parametrize("shape,fmt", CASES)
def test_a_slot_of_two_batches(mods, shape, fmt, r):
    """B = 2 F with the first frame at 0, B - 1 and 1 modulo B (leading frames dropped): a slot's boundary exactly on a batch's
    boundary -- the countdown reaches zero in the iteration in which the batch ends, every workgroup feeds one row and every
    complete row is fed by two --, one frame after it, and one frame before it; off the boundary a complete row is fed by three"""
    c = case(*SHAPES[shape])
    F = BATCH[shape]
    B = 2 * F
    m = {"on": 0, "after": B - 1, "before": 1}[r]
    lo = (m - first_frame(c)) % B
    got, con, _sc, _t, fa, k = launch(mods, shape, fmt, B, lo, c.frames)
    assert fa % B == m and k > B
    inner = [s * B - fa for s in range(fa // B + 1, (fa + k - 1) // B + 1)]      # slot boundaries inside the range, in frames from fa
    assert inner and all(0 < d < k for d in inner)
    assert all(d % F == {"on": 0, "after": 1, "before": F - 1}[r] for d in inner)
    per = [len(v) for v in feeds(con)]
    full = [len(con[i]) for i in range(len(con)) if int(got[i, c.N]) == B]
    if r == "on":
        assert set(per) == {1} and full and set(full) == {2}
    else:
        assert 2 in per and 1 in per
    if r == "after":
        assert full and set(full) == {3}


@pytest.mark.parametrize("shape,fmt", CASES)
def test_a_slot_of_three_batches_and_five_frames(mods, shape, fmt):
    """B = 3 F + 5, the first slot partial: some row takes frames from at least three workgroups, a slot's boundary falls inside a
    batch, and some workgroup starts deep inside a slot -- its first-frame division leaves more than F frames of the slot in front
    of it and more than F to go, so it lies wholly inside the slot and ends with the countdown far from zero"""
    c = case(*SHAPES[shape])
    F = BATCH[shape]
    B = 3 * F + 5

    def ok(con):
        n = [len(r) for r in feeds(con)]
        return max(len(s) for s in con) >= 3 and 1 in n[:-1] and 2 in n
    _got, con, _sc, _t, fa, k = launch(mods, shape, fmt, B, start(c, B, ok), c.frames)
    assert fa % B and len(con) >= 2
    assert max(len(s) for s in con) >= 3
    n = [len(r) for r in feeds(con)]
    assert 1 in n[:-1] and 2 in n
    deep = [g for g in range(len(n) - 1) if (fa + g * F) % B > F and B - (fa + g * F) % B > F]
    assert deep and all(n[g] == 1 for g in deep)


@pytest.mark.parametrize("B", ["frames + 3", "2^20"])
@pytest.mark.parametrize("shape,fmt", CASES)
def test_one_row_takes_everything(mods, shape, fmt, B):
    """B = frames + 3 (the range trimmed at its end, where it has to be, to lie inside slot 0) and B = 2^20: every workgroup of the
    launch, five or nine, adds into the one row; the row is p25fe_scan_dev's record of the range, bit for bit"""
    c = case(*SHAPES[shape])
    f0 = first_frame(c)
    B = c.frames + 3 if B == "frames + 3" else 1 << 20
    hi = min(c.frames, B - f0)                                       # frames f0 .. f0 + hi - 1 < B: slot 0
    got, con, sc, t, fa, k = launch(mods, shape, fmt, B, 0, hi)
    assert fa % B and k >= c.frames - 2
    assert len(con) == 1 and con[0] == set(range(-(-k // BATCH[shape]))) and len(con[0]) in (5, 9)
    whole = words(sc.scan_dev(t, n_hist=c.N - 1, abs0=fa * c.hop, offset=fa * c.hop, n=k * c.hop))
    assert int(whole[c.N]) == k and np.array_equal(got[0], whole)


# ---- 2. about a thousand workgroups into a handful of rows ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1000, 1 << 20])
def test_a_thousand_workgroups_into_a_handful_of_rows(mods, B):
    """test_gpu_waterfall.py's 9221 frames of random bytes at N = 1024, hop 512 (923 workgroups of 10 frames) in slots of 1000
    frames -- ten rows, a hundred workgroups adding into each of nine and into its count word -- and in one slot: every row equals
    p25fe_scan_dev over that slot's samples, the counts are the frames, the wrapping sum of the rows is the one-call record"""
    _lib, FE, Scanner = mods
    N, hop, frames = 1024, 512, 9221
    F = WM.batch(N, hop, frames)
    assert F == 10
    con = WM.contributors(0, frames, F, B)
    assert len(feeds(con)) == 923
    if B == 1000:
        assert [len(s) for s in con] == [100] * 9 + [23]
    else:
        assert [len(s) for s in con] == [923]
    raw = np.random.default_rng(frames).integers(0, 256, size=2 * (frames * hop + 5), dtype=np.uint8)
    t = dev(raw)
    sc = Scanner(FE(), N, hop, shift=SHIFT)
    rows = rows_of(sc.waterfall_dev(t, B))
    assert Scanner.slots(hop, B, 0, frames * hop + 5) == WM.slots(hop, B, 0, frames * hop + 5) == (0, len(con))
    assert rows.shape == (len(con), N + 1)
    assert list(rows[:, N]) == ([1000] * 9 + [221] if B == 1000 else [frames])
    whole = words(sc.scan_dev(t))
    assert int(whole[N]) == frames and whole[:N].all() and np.array_equal(summed(rows, N), whole)
    for i in range(len(con)):
        a, b = i * B * hop, min((i + 1) * B * hop, frames * hop + 5)
        one = words(sc.scan_dev(t, n_hist=a, abs0=a, offset=a, n=b - a))
        assert np.array_equal(rows[i], one), (i, np.flatnonzero(rows[i] != one)[:8])


# ---- 3. the u8 table instantiations ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,hop,frames", [(1024, 64, 70), (4096, 1024, 70)])
def test_the_u8_table(mods, N, hop, frames):
    """k_waterfall<U8, true, N> on a handle with a caller's table that is nothing affine, B = 5 and B = 3 F + 5, the first slot
    partial: the rows from the bytes equal the rows from the looked-up samples as cf32 on the same handle and WM.group of the same
    handle's per-frame records of the bytes (k_scan with the table), bit for bit; they are not a default handle's rows of the
    same bytes.  At (4096, 1024) a row of B = 53 is fed by three workgroups and a slot's boundary falls inside a batch"""
    _lib, FE, Scanner = mods
    c = case(N, hop, frames)
    lut = (np.sin(np.arange(256) * 0.37) * 0.9).astype(np.float32)   # test_gpu_scan.py's: nothing affine about it
    sc_t = Scanner(FE(u8_lut=lut, specialize=_lib.SPECIALIZE_OFF), N, hop, shift=SHIFT)
    sc_d = Scanner(FE(), N, hop, shift=SHIFT)
    raw = c.raw["u8"]
    t, t_cf = dev(raw), dev(conv(raw, lut))
    f0 = first_frame(c)
    rec = frames_of((N, hop, frames, "table"), lambda: SM.scan_frames(sc_t, t, f0, frames))
    fa, k = f0 + 1, frames - 1                                       # one frame dropped in front: the first slot is partial
    F = WM.batch(N, hop, k)
    assert F == {64: 64, 1024: 16}[hop]
    kw = dict(n_hist=N - 1, abs0=fa * hop, offset=fa * hop, n=k * hop)
    for B in (5, 3 * F + 5):
        got = rows_of(sc_t.waterfall_dev(t, B, **kw))
        slot0, ref = WM.group(rec[1:], fa, B)
        assert fa % B and Scanner.slots(hop, B, fa * hop, k * hop) == (slot0, ref.shape[0])
        assert np.array_equal(got, ref), (B, np.argwhere(got != ref)[:8])
        assert np.array_equal(got, rows_of(sc_t.waterfall_dev(t_cf, B, **kw))), B
        other = rows_of(sc_d.waterfall_dev(t, B, **kw))
        assert other.shape == got.shape and np.array_equal(other[:, N], got[:, N])
        assert not np.array_equal(other[:, :N], got[:, :N]), B       # the table was looked at
    if hop == 1024:                                                  # (at hop 64 a batch is 64 frames: one workgroup and 5 frames)
        con = WM.contributors(fa, k, F, 3 * F + 5)
        assert max(len(s) for s in con) >= 3 and 2 in [len(r) for r in feeds(con)]


# ---- 4. two streams, one set of rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["cf32", "u8"])
def test_two_streams_add_into_the_same_rows(mods, fmt):
    """a range cut inside a slot and inside a hop, the two pieces enqueued on two streams with nothing between them (what a
    double-buffered caller of p25fe_waterfall_dev does), B = 21: the rows are the one-call rows bit for bit, in either order"""
    import torch
    _lib, FE, Scanner = mods
    shape, B = "N1024_H512", 21
    c = case(*SHAPES[shape])
    N, hop = c.N, c.hop
    one, con, sc, t, fa, k = launch(mods, shape, fmt, B, 0, c.frames)
    at, n = fa * hop, k * hop
    cut = 30 * hop + 264
    slot0, n_rows = Scanner.slots(hop, B, at, n)
    (sa, na), (sb, nb) = Scanner.slots(hop, B, at, cut), Scanner.slots(hop, B, at + cut, n - cut)
    assert cut % 8 == 0 and cut % hop and (at + cut) // hop % B          # a multiple of 8 samples, inside a hop, inside a slot
    assert sa + na - 1 == sb and na + nb == n_rows + 1 and n_rows >= 4   # the pieces meet in one row
    assert WM.batch(N, hop, 30) == WM.batch(N, hop, 40) == 8 and max(len(s) for s in con) >= 3
    if not _STREAMS:
        _STREAMS.extend([torch.cuda.Stream(), torch.cuda.Stream()])      # two, for every case of this test
    s1, s2 = _STREAMS
    pieces = ((0, cut), (cut, n - cut))
    for order in ((0, 1), (1, 0)):
        cur = torch.cuda.current_stream()
        rows = torch.zeros((n_rows, N + 1), dtype=torch.int64, device=t.device)
        s1.wait_stream(cur)
        s2.wait_stream(cur)
        for s, i in zip((s1, s2), order):
            a, cnt = pieces[i]
            with torch.cuda.stream(s):
                sc.waterfall_dev(t, B, n_hist=N - 1, abs0=at + a, offset=at + a, n=cnt, rows=rows, slot0=slot0)
        cur.wait_stream(s1)
        cur.wait_stream(s2)
        got = rows_of(rows)
        assert np.array_equal(got, one), (order, np.argwhere(got != one)[:8])


# ---- 5. wrapping rows ----------------------------------------------------------------------------------------------------------------------
SAT_F0, SAT_FRAMES = 4, 60


@pytest.mark.parametrize("fmt", ["cf32", "s16", "u8"])
def test_rows_that_wrap(mods, fmt):
    """the saturating scene (a caller's window 8 x Hann at shift 40; bin SAT_BIN is 2^62 in every frame) lengthened to 60 frames
    with full history, hop 256, so F = 16: B = 5 and B = 37, which spans batches.  Rows equal the per-frame records summed per slot
    modulo 2^64; as Python integers column SAT_BIN of a row passes 2^64, so the row wrapped; the per-frame records are within
    3.0h's bound of the model, compared as integers"""
    _lib, FE, Scanner = mods
    N, H, w = SM.SAT_N, SM.SAT_HOP, SM.saturating_window()
    raw = SM.saturating_capture((SAT_F0 + SAT_FRAMES) * H + 16)[fmt]
    cf = raw if fmt == "cf32" else conv(raw)
    sc = Scanner(FE(), N, H, window=w, shift=SM.SAT_SHIFT)
    t = dev(raw)
    rec = frames_of(("saturating", fmt), lambda: SM.scan_frames(sc, t, SAT_F0, SAT_FRAMES))
    at, n = SAT_F0 * H, SAT_FRAMES * H
    X = SM.spectra(cf, N, H, w, at, n)
    ok, frac = within(rec[:, :N], SM.quantise(X, SM.SAT_SHIFT), SM.frame_bound(X, SM.delta(N, w, cf), SM.SAT_SHIFT))
    print("saturating %s: largest error %.4f of the per-frame bound" % (fmt, frac))
    assert ok and (rec[:, N] == 1).all() and (rec[:, SM.SAT_BIN] == np.uint64(1 << 62)).all()
    F = WM.batch(N, H, SAT_FRAMES)
    assert F == 16
    for B in (5, 37):
        got = rows_of(sc.waterfall_dev(t, B, n_hist=N - 1, abs0=at, offset=at, n=n))
        slot0, ref = WM.group(rec, SAT_F0, B)
        assert SAT_F0 % B and Scanner.slots(H, B, at, n) == (slot0, ref.shape[0])
        assert np.array_equal(got, ref), (B, np.argwhere(got != ref)[:8])
        true = [sum(int(rec[f - SAT_F0, SM.SAT_BIN]) for f in range(max(s * B, SAT_F0), min((s + 1) * B, SAT_F0 + SAT_FRAMES)))
                for s in range(slot0, slot0 + ref.shape[0])]
        assert max(true) > M64 and [int(v) for v in got[:, SM.SAT_BIN]] == [v % M64 for v in true]
        assert list(got[:, N]) == [v >> 62 for v in true]            # (the counts did not wrap)
        if B == 37:
            assert max(len(s) for s in WM.contributors(SAT_F0, SAT_FRAMES, F, B)) >= 3
            assert int(got[0, N]) * (1 << 62) > M64                  # the row that wrapped is one that three workgroups fed


# ---- 6. untouched rows between disjoint calls, and a far position ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["cf32", "u8"])
def test_rows_between_two_disjoint_calls_stay_untouched(mods, fmt):
    """two calls into one poisoned buffer (stride N + 5, a guard row on each side, row 0 = slot 0), B = 5: frames 3 .. 22 and
    41 .. 72 of the N1024_H512 range.  Slots 5 .. 7 lie between them and keep the poison in every word, word N included, as do the
    padding and the guards; the touched rows minus the poison are WM.group of the per-frame records"""
    import torch
    _lib, FE, Scanner = mods
    shape, B = "N1024_H512", 5
    c = case(*SHAPES[shape])
    N, hop, f0 = c.N, c.hop, first_frame(c)
    rec = gpu_frames(mods, shape, fmt)
    sc = Scanner(FE(), N, hop, shift=SHIFT)
    t = dev(c.raw[fmt])
    ranges = ((f0, 20), (f0 + 38, c.frames - 38))
    n_rows = (f0 + c.frames - 1) // B + 1
    ref = np.zeros((n_rows, N + 1), dtype=np.uint64)
    touched = set()
    for fa, k in ranges:
        slot0, r = WM.group(rec[fa - f0:fa - f0 + k], fa, B)
        ref[slot0:slot0 + r.shape[0]] += r
        touched |= set(range(slot0, slot0 + r.shape[0]))
        assert WM.batch(N, hop, k) == 8 and k > 16 and fa % B and (fa + k) % B        # several workgroups; partial slots at both ends
    between = sorted(set(range(min(touched), max(touched) + 1)) - touched)
    assert between == [5, 6, 7] and 0 in touched and n_rows - 1 in touched
    buf = torch.full((n_rows + 2, N + 5), POISON, dtype=torch.int64, device=t.device)
    for fa, k in ranges:
        sc.waterfall_dev(t, B, n_hist=N - 1, abs0=fa * hop, offset=fa * hop, n=k * hop, rows=buf[1:-1], slot0=0)
    got = rows_of(buf)
    assert (got[0] == POISON).all() and (got[-1] == POISON).all() and (got[1:-1, N + 1:] == POISON).all()
    assert (got[1:-1][between] == POISON).all()
    assert np.array_equal(got[1:-1, :N + 1] - np.uint64(POISON), ref)                 # (uint64 arithmetic wraps)
    assert int(ref[:, N].sum()) == 20 + c.frames - 38 and not ref[between].any()


@pytest.mark.parametrize("fmt,d", [("cf32", 1), ("s16", 3), ("u8", 5)])
def test_slots_past_two_to_the_thirty(mods, fmt, d):
    """the B = 3 F + 5 = 29 case of N1024_H512 at abs_first past 2^43, so that slot0 is past 2^30 (the workgroup's 64-bit division
    and the row offset slot - slot0): the rows of the same samples at a small position with the same place in a hop and the same
    f0 mod B, bit for bit; those sum to p25fe_scan_dev's record.  The same for the shape's whole frames, whose small-position rows
    are WM.group of the per-frame records"""
    _lib, FE, Scanner = mods
    N, hop, B = 1024, 512, 29
    c = case(N, hop, 70)
    sc = Scanner(FE(), N, hop, shift=SHIFT)
    t = dev(c.raw[fmt])
    offset, n = N + 8, 69 * hop + 40
    assert offset + n <= len(c.cf[fmt])
    small = offset + d
    big = small + ((1 << 30) + 1) * hop * B                          # the same place in a hop, the same f0 mod B
    assert big > 1 << 40 and (big - small) % 8 == 0 and (big // hop) % B == (small // hop) % B and big % hop == small % hop
    fa, k = small // hop, SM.n_frames(hop, small, n)
    F = WM.batch(N, hop, k)
    con = WM.contributors(fa, k, F, B)
    assert F == 8 and fa % B and max(len(s) for s in con) >= 4
    ref = rows_of(sc.waterfall_dev(t, B, n_hist=offset, abs0=small, offset=offset, n=n))
    assert ref.shape == (len(con), N + 1) and len(con) >= 3 and int(ref[:, N].sum()) == k
    assert np.array_equal(summed(ref, N), words(sc.scan_dev(t, n_hist=offset, abs0=small, offset=offset, n=n)))
    slot0, n_rows = Scanner.slots(hop, B, big, n)
    assert (slot0, n_rows) == WM.slots(hop, B, big, n) and slot0 > 1 << 30 and n_rows == len(con)
    got = rows_of(sc.waterfall_dev(t, B, n_hist=offset, abs0=big, offset=offset, n=n))
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:8]
    # ... and the whole frames of the shape's range, whose rows launch() holds to the per-frame records
    ref, con, sc, t, fa, k = launch(mods, "N1024_H512", fmt, B, 0, c.frames)
    far = (fa + ((1 << 30) + 1) * B) * hop
    assert max(len(s) for s in con) >= 3 and Scanner.slots(hop, B, far, k * hop) == ((1 << 30) + 1 + fa // B, len(con))
    got = rows_of(sc.waterfall_dev(t, B, n_hist=N - 1, abs0=far, offset=fa * hop, n=k * hop))
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:8]
