"""The survey on the GPU (docs/SPEC.md 3.0h: k_scan), through the C ABI, against tests/scan_model.py.

The DFT is fp32 and factored, so the sums are compared with the model's within 3.0h's bound; everything that integer sums and a
fixed per-frame sequence of operations promise is compared bit for bit: splits, missing history, the formats, the position, the
host streaming form.  Shapes: N = 1024 at hop 512 with 9 owned frames (two workgroups: a batch is 8 frames), N = 4096 at hop 2048
with 6, and N = 1024 at hop 1024 (no overlap: the whole ring is rewritten per frame) with 9; ranges start 24 samples past a hop's
multiple, so a workgroup's strip starts inside a hop -- but on a 16-byte vector of every format (24 is a multiple of 8 samples):
only the host streaming test puts frames off the loader's vectors here.  Positions that are no multiple of 8, hops of N/4 and below,
every frame by itself and Q's edges: tests/test_gpu_scan_edges.py.

Largest error observed on an MI355X as a fraction of the bound: see docs/MEASUREMENTS.md, "Survey"."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import scan_model as SM
from test_gpu_wide_fmt import affine_table, conv, dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFT = 16
SHAPES = {"N1024_H512": (1024, 512, 9), "N4096_H2048": (4096, 2048, 6), "N1024_H1024": (1024, 1024, 9)}
FMTS = ("cf32", "s16", "u8")


@pytest.fixture(scope="module")
def mods():
    from p25rx_amd import _lib, Scanner
    from p25rx_amd.frontend import FrontEnd, Tuner
    return _lib, FrontEnd, Scanner, Tuner


def signal(N, hop, length):
    """seeded noise plus two tones from position 0, complex64 [length]"""
    rng = np.random.default_rng(N + hop)
    t = np.arange(length, dtype=np.float64)
    x = 0.2 * (rng.standard_normal(len(t)) + 1j * rng.standard_normal(len(t))) / np.sqrt(2.0)
    x += 0.3 * np.exp(2j * np.pi * 0.1234 * t) + 0.25 * np.exp(-2j * np.pi * (37.5 / N) * t + 1.0j)
    return x.astype(np.complex64)


class Case:
    """seeded noise plus two tones from position 0: the raw samples of every format, their converted samples, and the range
    [first, first + n) that owns `frames` frames with all of its history in memory"""

    def __init__(self, N, hop, frames):
        self.N, self.hop, self.frames = N, hop, frames
        self.first = N + hop + 24
        self.n = frames * hop + 16
        assert SM.n_frames(hop, self.first, self.n) == frames and self.first % hop and self.first % 8 == 0
        x = signal(N, hop, self.first + self.n + 8)
        self.raw = {"cf32": x, "s16": SM.to_s16(x), "u8": SM.to_u8(x)}
        self.cf = {"cf32": x, "s16": conv(self.raw["s16"]), "u8": conv(self.raw["u8"])}
        self.w = SM.window(N)
        self._X = {}

    def X(self, fmt):
        if fmt not in self._X:
            self._X[fmt] = SM.spectra(self.cf[fmt], self.N, self.hop, self.w, self.first, self.n)
        return self._X[fmt]


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(*SHAPES[name])
    return _CASES[name]


def words(acc):
    return acc.cpu().numpy().view(np.uint64).copy()


def test_default_u8_numbers_are_the_models():
    spec = json.load(open(os.path.join(ROOT, "tests", "golden", "spec.json")))
    x = np.arange(256, dtype=np.uint8).repeat(2)
    assert np.array_equal(conv(x), SM.convert_u8(x, spec["u8_scale"], spec["u8_offset"]))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_within_the_bound_of_the_spec(mods, shape, fmt):
    """every acc[b] within 3.0h's bound propagated to the power: delta = 8 log2(N) 2^-24 sum|w| max|x| on X, |dP| <= 2 |X| delta +
    delta^2 per frame, times 2^shift, plus one unit per frame for the rounding of Q; acc[N] is the frame count"""
    _lib, FE, Scanner, _TN = mods
    c = case(shape)
    fe = FE()
    sc = Scanner(fe, c.N, c.hop, shift=SHIFT)
    got = words(sc.scan_dev(dev(c.raw[fmt]), n_hist=c.first, abs0=c.first, offset=c.first, n=c.n))
    X = c.X(fmt)
    assert int(got[c.N]) == c.frames == X.shape[0]
    ref = SM.quantise(X, SHIFT).sum(axis=0)                          # (sums below 2^53: exact in double)
    delta = 8.0 * np.log2(c.N) * 2.0 ** -24 * np.abs(c.w.astype(np.float64)).sum() * np.abs(c.cf[fmt].astype(np.complex128)).max()
    bound = ((2.0 * np.abs(X) * delta + delta * delta) * 2.0 ** SHIFT + 1.0).sum(axis=0)
    err = np.abs(got[:c.N].astype(np.float64) - ref)
    print("%s %s: largest error %.4f of the bound (bin %d: |error| %.0f of %.0f, sum %.3e)"
          % (shape, fmt, (err / bound).max(), int((err / bound).argmax()), err[(err / bound).argmax()],
             bound[(err / bound).argmax()], ref.max()))
    assert ref.max() > 2.0 ** 30                                     # the tones are there
    assert (err <= bound).all(), np.flatnonzero(err > bound)[:8]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("shape", ["N1024_H512", "N4096_H2048"])
def test_any_split_gives_the_same_bits(mods, shape, fmt):
    """one call over the range equals two and three calls at cuts that are multiples of 8 and not of the hop; each call's n_hist
    reaches back N - 1 or further"""
    _lib, FE, Scanner, _TN = mods
    c = case(shape)
    fe = FE()
    sc = Scanner(fe, c.N, c.hop, shift=SHIFT)
    t = dev(c.raw[fmt])
    whole = words(sc.scan_dev(t, n_hist=c.first, abs0=c.first, offset=c.first, n=c.n))
    assert int(whole[c.N]) == c.frames
    for cuts in ((c.hop + 8,), (8, 3 * c.hop - 16), (2 * c.hop + 1000, 2 * c.hop + 1008)):
        assert all(k % 8 == 0 and k % c.hop for k in cuts)
        acc = None
        edges = (0,) + cuts + (c.n,)
        for a, b in zip(edges[:-1], edges[1:]):
            n_hist = c.N - 1 if len(cuts) == 2 else c.first + a      # exactly what continuation needs, or everything there is
            acc = sc.scan_dev(t, n_hist=n_hist, abs0=c.first + a, offset=c.first + a, n=b - a, acc=acc)
        assert np.array_equal(words(acc), whole), cuts


@pytest.mark.parametrize("fmt", FMTS)
def test_missing_history_reads_as_zero(mods, fmt):
    """n_hist = 0 at abs_first > 0 equals the same range with a zeroed history in memory; n_hist = 100 likewise; a range shorter
    than one hop that owns no frame adds nothing"""
    import torch
    _lib, FE, Scanner, _TN = mods
    c = case("N1024_H512")
    fe = FE()
    sc = Scanner(fe, c.N, c.hop, shift=SHIFT)
    t = dev(c.raw[fmt])
    full = words(sc.scan_dev(t, n_hist=c.first, abs0=c.first, offset=c.first, n=c.n))
    per = 1 if fmt == "cf32" else 2
    if fmt == "u8":
        # no byte converts to zero with the default numbers: a table with an exact zero at byte 7, for both calls
        lut = affine_table()
        lut[7] = 0.0
        fe_z = FE(u8_lut=lut, specialize=_lib.SPECIALIZE_OFF)
        sc_z, fill = Scanner(fe_z, c.N, c.hop, shift=SHIFT), 7
    else:
        sc_z, fill = sc, 0
    for n_hist in (0, 100):
        z = np.array(c.raw[fmt])
        z[:per * (c.first - n_hist)] = fill
        a = words(sc_z.scan_dev(t, n_hist=n_hist, abs0=c.first, offset=c.first, n=c.n))
        b = words(sc_z.scan_dev(dev(z), n_hist=c.first, abs0=c.first, offset=c.first, n=c.n))
        assert int(a[c.N]) == c.frames and np.array_equal(a, b), n_hist
        assert not np.array_equal(a, full)
    acc = torch.zeros(c.N + 1, dtype=torch.int64, device="cuda")
    at = 3 * c.hop                                                   # the frame ending at 4 hop - 1 lies behind [3 hop, 4 hop - 8)
    sc.scan_dev(t, n_hist=c.N - 1, abs0=at, offset=at, n=c.hop - 8, acc=acc)
    sc.scan_dev(t, n_hist=0, abs0=at, offset=at, n=0, acc=acc)
    assert not words(acc).any()
    sc.scan_dev(t, n_hist=c.N - 1, abs0=at, offset=at, n=c.hop, acc=acc)
    assert int(words(acc)[c.N]) == 1


@pytest.mark.parametrize("shape", ["N1024_H512", "N4096_H2048"])
def test_formats_are_their_converted_samples(mods, shape):
    """the u8 and s16 records equal the cf32 record on the converted samples, bit for bit: the handle's default u8 numbers (the
    table as arithmetic) and a caller's table (looked up)"""
    _lib, FE, Scanner, _TN = mods
    c = case(shape)
    fe = FE()
    sc = Scanner(fe, c.N, c.hop, shift=SHIFT)
    kw = dict(n_hist=c.first, abs0=c.first, offset=c.first, n=c.n)
    for fmt in ("s16", "u8"):
        a = words(sc.scan_dev(dev(c.raw[fmt]), **kw))
        b = words(sc.scan_dev(dev(c.cf[fmt]), **kw))
        assert int(a[c.N]) == c.frames and np.array_equal(a, b), fmt
    lut = (np.sin(np.arange(256) * 0.37) * 0.9).astype(np.float32)   # nothing affine about it
    fe_t = FE(u8_lut=lut, specialize=_lib.SPECIALIZE_OFF)
    sc_t = Scanner(fe_t, c.N, c.hop, shift=SHIFT)
    a = words(sc_t.scan_dev(dev(c.raw["u8"]), **kw))
    b = words(sc_t.scan_dev(dev(conv(c.raw["u8"], lut)), **kw))
    assert np.array_equal(a, b) and not np.array_equal(a, words(sc.scan_dev(dev(c.raw["u8"]), **kw)))


@pytest.mark.parametrize("fmt", FMTS)
def test_position_matters_modulo_the_hop(mods, fmt):
    """abs_first = 2^40 + 3 H + 8 equals the same samples at 3 H + 8, bit for bit; a position 8 further on owns other frames"""
    _lib, FE, Scanner, _TN = mods
    c = case("N1024_H512")
    fe = FE()
    sc = Scanner(fe, c.N, c.hop, shift=SHIFT)
    t = dev(c.raw[fmt])
    off, n = c.N + 8, 5 * c.hop + 40
    a = words(sc.scan_dev(t, n_hist=c.N - 1, abs0=3 * c.hop + 8, offset=off, n=n))
    b = words(sc.scan_dev(t, n_hist=c.N - 1, abs0=(1 << 40) + 3 * c.hop + 8, offset=off, n=n))
    d = words(sc.scan_dev(t, n_hist=c.N - 1, abs0=(1 << 40) + 3 * c.hop + 16, offset=off, n=n))
    assert int(a[c.N]) == 5 and np.array_equal(a, b) and not np.array_equal(a, d)
    # ... and it is the model's record of the stream that begins 3 H + 8 - off samples earlier (same frames, same samples)
    lead = 3 * c.hop + 8 - off
    z = np.concatenate([np.zeros(lead, dtype=np.complex64), c.cf[fmt]])
    X = SM.spectra(z, c.N, c.hop, c.w, 3 * c.hop + 8, n, c.N - 1)
    ref = SM.quantise(X, SHIFT).sum(axis=0)
    assert np.abs(a[:c.N].astype(np.float64) - ref).max() <= 1e-4 * ref.max()


@pytest.mark.parametrize("fmt", ["cf32", "u8", "s16"])
def test_host_streaming_form(mods, fmt):
    """p25fe_scan in uneven chunks with p25fe_scan_read equals one p25fe_scan_dev over the whole capture, bit for bit; read with
    clear zeroes the record; reset starts over; a change of format inside a stream is refused"""
    _lib, FE, Scanner, _TN = mods
    c = case("N4096_H2048")
    fe = FE()
    sc = Scanner(fe, c.N, c.hop, shift=SHIFT)
    raw = c.raw[fmt]
    n = len(c.cf[fmt])
    whole = words(sc.scan_dev(dev(raw), n_hist=0, abs0=0, offset=0))
    assert int(whole[c.N]) == n // c.hop
    per = 1 if fmt == "cf32" else 2
    edges = [0, 1000, 1003, 5096, 5097, 5613, 5613, 13000, n]
    for a, b in zip(edges[:-1], edges[1:]):
        sc.scan(raw[per * a:per * b])
    assert np.array_equal(sc.read(), whole)
    assert np.array_equal(sc.read(clear=True), whole) and not sc.read().any()
    other = c.raw["s16" if fmt != "s16" else "u8"]
    with pytest.raises(_lib.P25feError) as e:
        sc.scan(other[:64])
    assert e.value.status == _lib.ERR_FORMAT
    sc.reset()
    assert not sc.read().any()
    sc.scan(raw)
    assert np.array_equal(sc.read(), whole)
    sc.reset()
    sc.scan(other[:2 * 4096])                                        # after a reset the stream may have another format
    assert int(sc.read()[c.N]) == 2


def test_guard_words_and_adding(mods):
    """the words in front of and behind the record are untouched; a second call adds rather than overwrites"""
    import torch
    _lib, FE, Scanner, _TN = mods
    for shape in ("N1024_H512", "N4096_H2048"):
        c = case(shape)
        fe = FE()
        sc = Scanner(fe, c.N, c.hop, shift=SHIFT)
        t = dev(c.raw["cf32"])
        G = 16
        buf = torch.full((c.N + 1 + 2 * G,), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda")
        buf[G:G + c.N + 1] = 0
        acc = buf[G:G + c.N + 1]
        kw = dict(n_hist=c.first, abs0=c.first, offset=c.first, n=c.n)
        sc.scan_dev(t, acc=acc, **kw)
        one = words(acc)
        sc.scan_dev(t, acc=acc, **kw)
        two = words(acc)
        assert int(one[c.N]) == c.frames and np.array_equal(two, one * np.uint64(2))
        assert bool((buf[:G] == 0x5a5a5a5a5a5a5a5a).all()) and bool((buf[G + c.N + 1:] == 0x5a5a5a5a5a5a5a5a).all())


def test_refusals_on_an_object(mods):
    """with a real object: misaligned pointers, null pointers, an unknown format and positions from 2^62 are P25FE_ERR_ARG and
    leave the record alone"""
    import torch
    _lib, FE, Scanner, _TN = mods
    fe = FE()
    sc = Scanner(fe, 1024, 512)
    L = sc.lib
    t = torch.zeros((4096, 2), dtype=torch.float32, device="cuda")
    acc = torch.zeros(1025 + 1, dtype=torch.int64, device="cuda")
    p, q = t.data_ptr(), acc.data_ptr()
    for d_iq, fmt, n, abs_first, d_acc in ((p + 8, 0, 2048, 0, q), (p, 0, 2048, 0, q + 4), (None, 0, 2048, 0, q), (p, 0, 2048, 0, None),
                                           (p, 3, 2048, 0, q), (p, -1, 2048, 0, q), (p, 0, 2048, 1 << 62, q), (p, 0, 1 << 62, 0, q),
                                           (p + 2, 1, 2048, 0, q), (p + 4, 2, 2048, 0, q)):
        rc = L.p25fe_scan_dev(sc.sc, C.c_void_p(d_iq) if d_iq else None, fmt, 0, n, abs_first, C.c_void_p(d_acc) if d_acc else None, None)
        assert rc == _lib.ERR_ARG, (d_iq, fmt, n, abs_first, d_acc)
    torch.cuda.synchronize()
    assert not words(acc).any()
    assert L.p25fe_scan_read(sc.sc, None, 0) == _lib.ERR_ARG


# ---- end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["u8", "cf32"])
def test_end_to_end(mods, fmt):
    """the scene of tests/scan_model.py: Scanner -> channels gives exactly the raster channels {-33, 0, 11, 12}; the channels
    tuned by Tuner.nco at r * 12500 + offset_hz and run through a four-channel receive chain: every row finds frame syncs and
    decodes its generator's symbols with 0 errors (the CPU model of the same chain -- tests/tune_nco_model.py and the oracle on the
    model's record -- gives 0 in 1168 symbols per row, residuals 20 .. 62 Hz); the residual is at most 150 Hz, against the 600 Hz
    the chain tolerates (3.0f).  Tuned at the bare raster frequencies, the three off-raster rows find no frame."""
    from p25rx_amd.frontend import parse_results
    _lib, FE, Scanner, TN = mods
    x, truths = SM.scene()
    raw = x if fmt == "cf32" else SM.to_u8(x)
    fs = SM.SCENE_FS
    fe1, fe4 = FE(), FE(n_channels=4)
    sc = Scanner(fe1, 4096, 2048, shift=SHIFT)
    t = dev(raw)
    acc = words(sc.scan_dev(t))
    assert int(acc[4096]) == len(x) // 2048
    chans = Scanner.channels(acc, fs)
    found = {int(ch["raster_index"]): ch for ch in chans}
    assert set(found) == set(SM.SCENE_CHANNELS), sorted(found)
    assert (chans["db_over_floor"] >= 35.0).all()
    freqs = []
    for off in SM.TRUE_OFFSETS_HZ:                                   # the sources' order: row k decodes truths[k]
        ch = found[int(round(off / 12500.0))]
        f = ch["centre_hz"] + ch["offset_hz"]
        print("%s: channel %d, %.1f dB over the floor, offset %.1f Hz, residual %.1f Hz"
              % (fmt, ch["raster_index"], ch["db_over_floor"], ch["offset_hz"], f - off))
        assert abs(f - off) <= 150.0
        freqs.append(float(f))
    L, M, T, taps, steps = TN.design_nco(fs, freqs)
    y, no = TN.nco(fe1, L, M, T, taps, steps).tune_dev(t)
    dib, res = fe4.run_dev(y[:, :no])
    for k in range(4):
        r = parse_results(res)[k]
        got = dib[k, :int(r["n_dibits"])].cpu().numpy()
        kk = min(len(got), len(truths[k]) - 24)
        errs = int(np.count_nonzero(got[:kk] != truths[k][24:24 + kk]))
        print("    row %d: %d syncs, %d errors in %d symbols" % (k, int(r["n_sync"]), errs, kk))
        assert int(r["n_sync"]) >= 1 and kk > 1100 and errs == 0, (k, errs, kk)
    bare = [int(round(off / 12500.0)) * 12500.0 for off in SM.TRUE_OFFSETS_HZ]
    L, M, T, taps, steps = TN.design_nco(fs, bare)
    y, no = TN.nco(fe1, L, M, T, taps, steps).tune_dev(t)
    dib, res = fe4.run_dev(y[:, :no])
    assert [int(r["n_dibits"]) for r in parse_results(res)][:3] == [0, 0, 0]
