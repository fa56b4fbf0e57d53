"""The survey on the GPU (docs/SPEC.md 3.0h: k_scan) where tests/test_gpu_scan.py does not go: hops of N/4 and below (a ring filled by
N/H prologue hops and restaged while N/H - 1 other hops are live; batches of 4 N/H frames), every frame by itself against the model,
stream positions that are no multiple of the loader's vector, Q's edges (the clamp at 2^62, the wrapping sum, shifts 0 and 40, NaN
and infinity, a caller's window), a batch above 8 frames in about a thousand workgroups, and the host streaming form at a small hop.

The only tolerance is 3.0h's: delta = 8 log2(N) 2^-24 sum|w| max|x| on X, |dP| <= 2 |X| delta + delta^2, times 2^shift, plus one
unit for the rounding of Q -- here per FRAME and bin wherever a frame's record can be had alone, so that a defect confined to one
frame of a batch cannot hide in a sum.  Everything that integer sums promise is compared bit for bit.

Largest error observed on an MI355X as a fraction of the per-frame bound: see docs/MEASUREMENTS.md, "Survey"."""
import numpy as np
import pytest

import scan_model as SM
from test_gpu_scan import SHIFT, signal, words
from test_gpu_wide_fmt import conv, dev

pytestmark = pytest.mark.gpu

# N, hop, frames of one call: it crosses the boundary of a batch F = max(8, 4 N / H) except at (4096, 8), one workgroup
SHAPES = {"N1024_H8": (1024, 8, 520), "N1024_H64": (1024, 64, 70), "N1024_H256": (1024, 256, 20),
          "N4096_H8": (4096, 8, 40), "N4096_H64": (4096, 64, 260), "N4096_H1024": (4096, 1024, 20)}
ALL_FORMATS = ("N1024_H8", "N1024_H256", "N4096_H64")
FRAME_CASES = [(s, f) for s in SHAPES for f in ("cf32", "s16", "u8") if f == "cf32" or s in ALL_FORMATS]
M62 = 1 << 62


@pytest.fixture(scope="module")
def mods():
    from p25rx_amd import _lib, Scanner
    from p25rx_amd.frontend import FrontEnd
    return _lib, FrontEnd, Scanner


_CASES, _FRAMES = {}, {}


class Capture:
    """tests/test_gpu_scan.py's signal (seeded noise plus two tones from position 0), long enough for `frames` frames behind the
    first one with all of its history in memory: the raw samples of every format and their converted samples"""

    def __init__(self, N, hop, frames):
        self.N, self.hop, self.frames = N, hop, frames
        x = signal(N, hop, N + hop + frames * hop + 48)
        self.raw = {"cf32": x, "s16": SM.to_s16(x), "u8": SM.to_u8(x)}
        self.cf = {"cf32": x, "s16": conv(self.raw["s16"]), "u8": conv(self.raw["u8"])}
        self.w = SM.window(N)


def case(N, hop, frames):
    if (N, hop, frames) not in _CASES:
        _CASES[(N, hop, frames)] = Capture(N, hop, frames)
    return _CASES[(N, hop, frames)]


def first_frame(c):
    return c.N // c.hop + 1                                          # the first frame with all of its history behind sample N


def gpu_frames(mods, shape, fmt):
    """the GPU's per-frame records of a shape's range, made once: uint64 [frames, N + 1]"""
    if (shape, fmt) not in _FRAMES:
        _lib, FE, Scanner = mods
        c = case(*SHAPES[shape])
        sc = Scanner(FE(), c.N, c.hop, shift=SHIFT)
        _FRAMES[(shape, fmt)] = SM.scan_frames(sc, dev(c.raw[fmt]), first_frame(c), c.frames)
    return _FRAMES[(shape, fmt)]


def within(got, ref, bound):
    """|got - ref| <= bound for every word, compared as Python integers against the bound's doubles -> (ok, largest fraction)"""
    err = np.abs(SM.as_ints(got) - SM.as_ints(ref)).reshape(-1)
    b = np.asarray(bound, dtype=np.float64).reshape(-1)
    return all(int(e) <= v for e, v in zip(err, b)), max(float(e) / v for e, v in zip(err, b))


# ---- 1. every frame by itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,fmt", FRAME_CASES)
def test_every_frame_within_the_bound(mods, shape, fmt):
    """rec_f[f, b] against Q(P_f[b]) of the model for every frame and bin, nothing summed over frames; rec_f[f, N] = 1"""
    c = case(*SHAPES[shape])
    rec = gpu_frames(mods, shape, fmt)
    f0 = first_frame(c)
    X = SM.spectra(c.cf[fmt], c.N, c.hop, c.w, f0 * c.hop, c.frames * c.hop)
    assert rec.shape == (c.frames, c.N + 1) == (X.shape[0], X.shape[1] + 1)
    assert (rec[:, c.N] == 1).all()
    ref = SM.quantise(X, SHIFT)                                      # (below 2^53: exact in double, and so is the difference)
    bound = SM.frame_bound(X, SM.delta(c.N, c.w, c.cf[fmt]), SHIFT)
    err = np.abs(rec[:, :c.N].astype(np.float64) - ref)
    frac = err / bound
    f, b = np.unravel_index(int(frac.argmax()), frac.shape)
    print("%s %s: largest error %.4f of the per-frame bound (frame %d of %d, bin %d: |error| %.0f of %.0f)"
          % (shape, fmt, frac.max(), f, c.frames, b, err[f, b], bound[f, b]))
    assert ref.max() > 2.0 ** 30                                     # the tones are there
    assert (err <= bound).all(), np.argwhere(err > bound)[:8]


@pytest.mark.parametrize("shape,fmt", FRAME_CASES)
def test_a_batch_is_the_sum_of_its_frames(mods, shape, fmt):
    """one call over the whole range equals the wrapping sum of the per-frame records in all 8 (N + 1) bytes: the ring's rotation,
    the prefetch and the staging over a live ring against the path of a call's first frame, at every place in a batch; and the
    u8 and s16 batches equal the cf32 batch on their converted samples"""
    _lib, FE, Scanner = mods
    c = case(*SHAPES[shape])
    rec = gpu_frames(mods, shape, fmt)
    at = first_frame(c) * c.hop
    sc = Scanner(FE(), c.N, c.hop, shift=SHIFT)
    kw = dict(n_hist=c.N - 1, abs0=at, offset=at, n=c.frames * c.hop)
    whole = words(sc.scan_dev(dev(c.raw[fmt]), **kw))
    assert int(whole[c.N]) == c.frames
    assert np.array_equal(whole, SM.wrapping_sum(rec)), np.flatnonzero(whole != SM.wrapping_sum(rec))[:8]
    if fmt != "cf32":
        assert np.array_equal(whole, words(sc.scan_dev(dev(c.cf[fmt]), **kw)))


# ---- 2. positions that are no multiple of the loader's vector -------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["cf32", "s16", "u8"])
@pytest.mark.parametrize("N,hop", [(1024, 64), (1024, 512), (4096, 512)])
def test_odd_stream_positions(mods, N, hop, fmt):
    """abs_first = offset + d with the pointer aligned: the frames lie d samples off the 16-byte vectors (the kernel's sh takes
    every value but 0).  Each record against the model's of the same samples d positions later in a stream, per bin within the
    bound summed over its frames; and equal, bit for bit, to the same range split at cuts that are multiples of 8 in the buffer"""
    _lib, FE, Scanner = mods
    c = case(N, hop, 12)
    sc = Scanner(FE(), N, hop, shift=SHIFT)
    t = dev(c.raw[fmt])
    offset, n = N + 8, 10 * hop + 5
    assert offset + n + 8 <= len(c.cf[fmt])
    dl = SM.delta(N, c.w, c.cf[fmt])
    worst = 0.0
    for d in {"u8": range(1, 8), "s16": range(1, 4), "cf32": range(1, 2)}[fmt]:
        abs0 = offset + d
        got = words(sc.scan_dev(t, n_hist=offset, abs0=abs0, offset=offset, n=n))
        X = SM.spectra(SM.shifted(c.cf[fmt], d), N, hop, c.w, abs0, n, offset)
        assert int(got[N]) == X.shape[0] == 10
        ref = SM.quantise(X, SHIFT).sum(axis=0)                      # (sums below 2^53: exact in double)
        bound = SM.frame_bound(X, dl, SHIFT).sum(axis=0)
        err = np.abs(got[:N].astype(np.float64) - ref)
        worst = max(worst, (err / bound).max())
        assert ref.max() > 2.0 ** 30
        assert (err <= bound).all(), (d, np.flatnonzero(err > bound)[:8])
        for cuts in ((hop + 8,), (8, 3 * hop - 16)):
            acc = None
            edges = (0,) + cuts + (n,)
            for a, b in zip(edges[:-1], edges[1:]):
                assert a % 8 == 0 and (abs0 + a) % 8 == d
                n_hist = N - 1 if len(cuts) == 2 else offset + a     # exactly what continuation needs, or everything there is
                acc = sc.scan_dev(t, n_hist=n_hist, abs0=abs0 + a, offset=offset + a, n=b - a, acc=acc)
            assert np.array_equal(words(acc), got), (d, cuts)
    print("N %d hop %d %s: largest error %.4f of the summed bound" % (N, hop, fmt, worst))


# ---- 3. Q's edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["cf32", "s16", "u8"])
def test_the_clamp_and_the_wrapping_sum(mods, fmt):
    """a caller's window 8 x Hann at shift 40 on the saturating scene (tests/test_scan_abi.py holds its premise: bin 100 is past
    2^62 by more than the bound in every frame, no other bin is within the bound of it): three frames give 3 * 2^62 exactly, four
    wrap to 0 while the frame count says 4; every other bin within the bound, compared as integers"""
    _lib, FE, Scanner = mods
    N, H, B, w = SM.SAT_N, SM.SAT_HOP, SM.SAT_BIN, SM.saturating_window()
    raw = SM.saturating_capture()[fmt]
    cf = raw if fmt == "cf32" else conv(raw)
    sc = Scanner(FE(), N, H, window=w, shift=SM.SAT_SHIFT)
    t = dev(raw)
    X = SM.spectra(cf, N, H, w, N, 4 * H)
    q = SM.as_ints(SM.quantise(X, SM.SAT_SHIFT))
    bound = SM.frame_bound(X, SM.delta(N, w, cf), SM.SAT_SHIFT)
    others = np.arange(N) != B
    for k in (3, 4):
        got = words(sc.scan_dev(t, n_hist=N - 1, abs0=N, offset=N, n=k * H))
        assert int(got[N]) == k
        assert int(got[B]) == (k * M62) % (1 << 64), (k, hex(int(got[B])))
        ok, frac = within(got[:N][others], q[:k].sum(axis=0)[others], bound[:k].sum(axis=0)[others])
        print("%s, %d frames: largest error %.4f of the bound, largest unsaturated sum %.3f x 2^62"
              % (fmt, k, frac, max(int(v) for v in got[:N][others]) / M62))
        assert ok
    assert int(q[:, others].max()) > M62 // 2                        # a clamp one bit low would cut these


def test_the_designed_window_passed_explicitly(mods):
    _lib, FE, Scanner = mods
    c = case(*SHAPES["N1024_H256"])
    fe = FE()
    t = dev(c.raw["cf32"])
    at = c.N + c.hop + 24
    kw = dict(n_hist=at, abs0=at, offset=at, n=c.frames * c.hop)
    a = words(Scanner(fe, c.N, c.hop, shift=SHIFT).scan_dev(t, **kw))
    b = words(Scanner(fe, c.N, c.hop, window=Scanner.design(c.N), shift=SHIFT).scan_dev(t, **kw))
    assert int(a[c.N]) == c.frames and np.array_equal(a, b)


@pytest.mark.parametrize("fmt", ["cf32", "s16", "u8"])
def test_shift_zero(mods, fmt):
    """shift 0: the sums within the bound (which is then little more than the rounding unit per frame), non-zero at the tones'
    bins, and neither the record of shift 16 nor nothing"""
    _lib, FE, Scanner = mods
    c = case(*SHAPES["N1024_H256"])
    fe = FE()
    t = dev(c.raw[fmt])
    at = c.N + c.hop + 24
    kw = dict(n_hist=at, abs0=at, offset=at, n=c.frames * c.hop)
    got = words(Scanner(fe, c.N, c.hop, shift=0).scan_dev(t, **kw))
    X = SM.spectra(c.cf[fmt], c.N, c.hop, c.w, at, c.frames * c.hop)
    assert int(got[c.N]) == c.frames == X.shape[0]
    ref = SM.quantise(X, 0).sum(axis=0)
    bound = SM.frame_bound(X, SM.delta(c.N, c.w, c.cf[fmt]), 0).sum(axis=0)
    err = np.abs(got[:c.N].astype(np.float64) - ref)
    print("%s: largest error %.4f of the bound, largest sum %.0f" % (fmt, (err / bound).max(), ref.max()))
    assert (err <= bound).all(), np.flatnonzero(err > bound)[:8]
    for b in (126, c.N - 38, c.N - 37):                              # 0.1234 N = 126.4 and -37.5
        assert int(got[b]) > 1000
    other = words(Scanner(fe, c.N, c.hop, shift=SHIFT).scan_dev(t, **kw))
    assert got[:c.N].any() and not np.array_equal(got, other)


def _poisoned(mods, value, component, j):
    """the N1024_H256 range's first 12 frames with `value` in one component of the sample at position j of hop f0 + 4, which
    frames 4 .. 7 of the 12 cover -> (the record, the clean per-frame records)"""
    _lib, FE, Scanner = mods
    c = case(*SHAPES["N1024_H256"])
    rec = gpu_frames(mods, "N1024_H256", "cf32")[:12]
    f0 = first_frame(c)
    x = np.array(c.raw["cf32"])
    v = x.view(np.float32).reshape(-1, 2)
    v[(f0 + 4) * c.hop + j, component] = value
    sc = Scanner(FE(), c.N, c.hop, shift=SHIFT)
    got = words(sc.scan_dev(dev(x), n_hist=c.N - 1, abs0=f0 * c.hop, offset=f0 * c.hop, n=12 * c.hop))
    assert int(got[c.N]) == 12
    return got, rec


@pytest.mark.parametrize("j,component", [(37, 0), (0, 1)])
def test_a_nan_empties_its_frames_only(mods, j, component):
    """one NaN component in a sample that exactly N / H = 4 frames of 12 cover: those frames count and add nothing, the record is
    the sum of the clean input's other 8 per-frame records, bit for bit.  j = 0 is where the last of the four frames has the
    window's zero: 0 * NaN is NaN"""
    got, rec = _poisoned(mods, np.nan, component, j)
    clean = SM.wrapping_sum(np.concatenate([rec[:4], rec[8:]]))
    assert np.array_equal(got[:-1], clean[:-1]), np.flatnonzero(got[:-1] != clean[:-1])[:8]
    assert not np.array_equal(got[:-1], SM.wrapping_sum(rec)[:-1])


@pytest.mark.parametrize("value,component", [(np.inf, 0), (-np.inf, 1)])
def test_an_infinity_adds_multiples_of_the_clamp(mods, value, component):
    """an infinite component: every bin of each of the four frames that cover it becomes 0 (NaN) or exactly 2^62; the other 8
    frames are untouched"""
    got, rec = _poisoned(mods, value, component, 37)
    clean = SM.as_ints(SM.wrapping_sum(np.concatenate([rec[:4], rec[8:]])))
    extra = [(int(g) - int(k)) % (1 << 64) for g, k in zip(got[:-1], clean[:-1])]
    assert all(e % M62 == 0 for e in extra), [b for b, e in enumerate(extra) if e % M62][:8]
    print("bins at 0, 1, 2, 3 x 2^62: %s" % [sum(1 for e in extra if e == k * M62) for k in range(4)])


# ---- 4. batches above 8 frames, about a thousand workgroups ------------------------------------------------------------------------
def test_ten_frames_a_batch_in_923_workgroups(mods):
    """9221 frames of N = 1024 at hop 512 in one call (batches of 10, the last workgroup with one frame) equal the same range in
    three calls of 3000, 4000 and 2221 frames (batches of 8, the path the per-frame tests pin), bit for bit"""
    _lib, FE, Scanner = mods
    N, H, frames = 1024, 512, 9221
    raw = np.random.default_rng(9221).integers(0, 256, size=2 * frames * H, dtype=np.uint8)
    t = dev(raw)
    sc = Scanner(FE(), N, H, shift=SHIFT)
    whole = words(sc.scan_dev(t))
    assert int(whole[N]) == frames and whole[:N].all()
    acc = None
    edges = (0, 3000 * H + 8, 7000 * H + 1000, frames * H)
    for a, b in zip(edges[:-1], edges[1:]):
        assert a % 8 == 0 and SM.n_frames(H, a, b - a) <= 8192
        acc = sc.scan_dev(t, n_hist=a, abs0=a, offset=a, n=b - a, acc=acc)
    assert np.array_equal(words(acc), whole)


# ---- 5. the host streaming form at a small hop --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["u8", "cf32"])
def test_host_streaming_at_a_small_hop(mods, fmt):
    """p25fe_scan at N = 1024, hop 64 in chunks of 1, 3, 7, 63, 64, 65, 1000 and 0 samples and the rest equals one p25fe_scan_dev
    over the capture, bit for bit"""
    _lib, FE, Scanner = mods
    c = case(*SHAPES["N1024_H64"])
    sc = Scanner(FE(), c.N, c.hop, shift=SHIFT)
    raw = c.raw[fmt]
    n = len(c.cf[fmt])
    whole = words(sc.scan_dev(dev(raw), n_hist=0, abs0=0, offset=0))
    assert int(whole[c.N]) == n // c.hop
    per = 1 if fmt == "cf32" else 2
    edges = np.concatenate([[0], np.cumsum([1, 3, 7, 63, 64, 65, 1000, 0]), [n]])
    for a, b in zip(edges[:-1], edges[1:]):
        sc.scan(raw[per * a:per * b])
    assert np.array_equal(sc.read(), whole)
