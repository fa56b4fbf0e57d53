"""u8 and s16 input to the two 2.4 Msps stages: the pre-decimator (docs/SPEC.md 3.0) and the channeliser (3.11).

A wideband u8 or s16 stream IS the cf32 stream of its converted samples, so every case makes the same two comparisons:
(A) the narrow call's output equals, as uint32, the cf32 call's output on the converted samples with the same n_hist / abs0 /
    offset;
(B) where abs0 == offset, it equals the oracle on the converted samples: O.PreDecim bit for bit, O.channelise within SPEC 3.11's
    own bound per output, (2e-6 + 2^-24) * T (tests/chz_model.py; 2^-24 T is the oracle's rounding to fp32), and never more than
    the capture-wide 2e-6 * sum|h| * max|x|.  Tests 1, 2 and 5 hold the cf32 call's output to (B) as well: cf32 is one more
    instantiation of the same kernel body, checked on its own and not only through (A).
The conversions are computed here in float64 and rounded once, which is fma((float)b, scale, offset) exactly (8 x 24 bits and one
addition fit a double), and (float)v * 2^-15, which is exact.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U8_SCALE, U8_OFFSET = np.float32(2.0 / 255.0), np.float32(-1.0)


def conv_s16(x):
    """[..., 2 n] int16 -> [..., n] complex64"""
    return np.ascontiguousarray(np.asarray(x, dtype=np.int16).astype(np.float32) * np.float32(2.0 ** -15)).view(np.complex64)


def affine_table(scale=U8_SCALE, offset=U8_OFFSET):
    b = np.arange(256, dtype=np.float64)
    return (b * np.float64(np.float32(scale)) + np.float64(np.float32(offset))).astype(np.float32)


def conv_u8(x, table=None):
    """[..., 2 n] uint8 -> [..., n] complex64 through the 256-entry table (default: SPEC 3.1's)"""
    t = affine_table() if table is None else np.asarray(table, dtype=np.float32)
    return np.ascontiguousarray(t[np.asarray(x, dtype=np.uint8)]).view(np.complex64)


def conv(x, table=None):
    return conv_u8(x, table) if x.dtype == np.uint8 else conv_s16(x)


def dev(a):
    """[..., 2 n] u8 / s16 or [..., n] complex64 -> device tensor [..., n, 2]"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.complex64:
        return torch.from_numpy(a.view(np.float32).reshape(a.shape + (2,)).copy()).cuda()
    return torch.from_numpy(a.reshape(a.shape[:-1] + (-1, 2)).copy()).cuda()


def same_bits(a, b):
    import torch
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def bits(a):
    return np.ascontiguousarray(a).view(np.float32).view(np.uint32)


def noise(fmt, rng, n):
    """[2 n] random samples of the format with its extreme values spliced in"""
    if fmt == "u8":
        x = rng.integers(0, 256, size=2 * n, dtype=np.int64).astype(np.uint8)
        x[10:14] = (0, 255, 255, 0)
        x[-4:] = (255, 0, 0, 255)
    else:
        x = rng.integers(-32768, 32768, size=2 * n, dtype=np.int64).astype(np.int16)
        x[10:14] = (-32768, 32767, 32767, -32768)
        x[-4:] = (32767, -32768, -32768, 32767)
    return x


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def FE():
    from p25rx_amd.frontend import FrontEnd
    return FrontEnd


def first_out(offset):
    """number of outputs whose instant 10 m + 9 lies before `offset`"""
    return offset // 10


def oracle_predecim(O, cf, offset, n_hist, n):
    """what the oracle gives for the range [offset, offset + n) when only n_hist samples in front of it exist"""
    z = np.array(cf[:offset + n], dtype=np.complex64)
    z[:offset - n_hist] = 0                                          # (a zero sample adds an exact zero to the accumulator)
    y = O.PreDecim().feed(z)
    return y[first_out(offset):]


# ---- 1: one channel from the start of the stream -----------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["u8", "s16"])
def test_predecim_whole_stream(O, FE, fmt):
    """n = 7709: 770 outputs (instants 9, 19 .. 7699) = two workgroups of 384 and a partial sub-tile, n no multiple of 8; extremes of
    the format included"""
    n = 7709
    x = noise(fmt, np.random.default_rng(1), n)
    assert (x.min(), x.max()) == ((0, 255) if fmt == "u8" else (-32768, 32767))
    cf = conv(x)
    fe = FE()
    y, no = fe.predecim_dev(dev(x))
    yc, noc = fe.predecim_dev(dev(cf))
    assert no == noc == 770
    assert same_bits(y[:, :no], yc[:, :no])                          # (A)
    ref = O.PreDecim().feed(cf)
    assert len(ref) == no and np.array_equal(bits(y[0, :no].cpu().numpy()).ravel(), bits(ref).ravel())     # (B)
    assert np.array_equal(bits(yc[0, :no].cpu().numpy()).ravel(), bits(ref).ravel())                       # (B), cf32


# ---- 2: grid and history sweep -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["u8", "s16"])
def test_predecim_grid_and_history_sweep(O, FE, fmt):
    """every o0, both window parities, history shorter than the 79 samples needed, empty and one-output results, tails inside a vector"""
    lens = (1, 7, 9, 10, 1913, 1921, 3847)
    total = 2008 + max(lens)
    x = noise(fmt, np.random.default_rng(2), total)
    cf = conv(x)
    tx, tc = dev(x), dev(cf)
    fe = FE()
    seen_empty = seen_one = False
    for offset in (2000, 2008):
        for n_hist in (0, 8, 72, 79, 80, 96):
            for n in lens:
                ref = oracle_predecim(O, cf, offset, n_hist, n)
                for r in range(10):
                    kw = dict(n_hist=n_hist, abs0=offset + r, offset=offset)
                    y, no = fe.predecim_dev(tx[:offset + n], **kw)
                    yc, noc = fe.predecim_dev(tc[:offset + n], **kw)
                    assert no == noc, (offset, n_hist, n, r)
                    seen_empty |= no == 0
                    seen_one |= no == 1
                    assert same_bits(y[:, :no], yc[:, :no]), (offset, n_hist, n, r)                    # (A)
                    if r == 0:                                                                        # (B)
                        assert no == len(ref), (offset, n_hist, n)
                        assert np.array_equal(bits(y[0, :no].cpu().numpy()).ravel(), bits(ref).ravel()), (offset, n_hist, n)
                        assert np.array_equal(bits(yc[0, :no].cpu().numpy()).ravel(), bits(ref).ravel()), (offset, n_hist, n)
    assert seen_empty and seen_one


# ---- 3: what surrounds the range is never used -------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["u8", "s16"])
def test_surroundings_are_ignored(O, FE, fmt):
    """the range inside a larger buffer of random bytes gives what it gives inside zeros; both stages.  The buffer extends 2000
    samples in front of the range and at least 64 behind it, so every vector the kernels touch lies inside it."""
    offset, back = 2000, 64
    rng = np.random.default_rng(3)
    fe = FE()
    for n_hist in (0, 83):
        for n in (2001, 2003, 2007, 1):                              # n % 8 = 1, 3, 7: the tail ends inside a vector
            x = noise(fmt, rng, offset + n + back)
            z = x.copy()
            z[:2 * (offset - n_hist)] = 0
            z[2 * (offset + n):] = 0
            tx, tz = dev(x), dev(z)
            kw = dict(n_hist=n_hist, abs0=offset, offset=offset)
            y, no = fe.predecim_dev(tx[:offset + n], **kw)
            yz, _ = fe.predecim_dev(tz[:offset + n], **kw)
            assert same_bits(y[:, :no], yz[:, :no]), (n_hist, n)
            ref = oracle_predecim(O, conv(z), offset, n_hist, n)
            assert no == len(ref) and np.array_equal(bits(y[0, :no].cpu().numpy()).ravel(), bits(ref).ravel()), (n_hist, n)
            yc, _ = fe.predecim_dev(dev(conv(z))[:offset + n], **kw)
            assert same_bits(y[:, :no], yc[:, :no]), (n_hist, n)
            c, nc = fe.channelise_dev(tx[:offset + n], **kw)
            cz, _ = fe.channelise_dev(tz[:offset + n], **kw)
            assert same_bits(c[:, :nc], cz[:, :nc]), (n_hist, n)


# ---- 4: the u8 conversions ---------------------------------------------------------------------------------------------------
def _monotone_table():
    rng = np.random.default_rng(44)
    steps = rng.uniform(0.001, 0.02, size=256)
    t = (np.cumsum(steps) - steps.sum() / 2).astype(np.float32)
    assert (np.diff(t) > 0).all() and np.abs(np.diff(t, 2)).max() > 1e-3          # monotone, nowhere near a straight line
    return t


@pytest.mark.parametrize("kind", ["default", "affine", "lut"])
def test_u8_conversions_three_channels(O, FE, kind):
    """the default table, a caller's scale / offset and a table that is not affine (looked up), on three channels whose stride
    (2056 samples) is longer than the range; both stages"""
    from p25rx_amd import _lib
    if kind == "default":
        kw, table = {}, affine_table()
    elif kind == "affine":
        kw = dict(u8_scale=0.0123, u8_offset=-1.57)
        table = affine_table(np.float32(0.0123), np.float32(-1.57))
    else:
        table = _monotone_table()
        kw = dict(u8_lut=table)
    if kw:
        kw["specialize"] = _lib.SPECIALIZE_OFF
    Cn, stride, n = 3, 2056, 2049
    rng = np.random.default_rng(4)
    x = np.stack([noise("u8", rng, stride) for _ in range(Cn)])
    cf = conv_u8(x, table)
    fe = FE(n_channels=Cn, **kw)
    tx, tc = dev(x), dev(cf)
    assert tx.shape == (Cn, stride, 2) and tx.stride(0) == 2 * stride
    y, no = fe.predecim_dev(tx[:, :n])
    yc, noc = fe.predecim_dev(tc[:, :n])
    assert no == noc == 204
    assert same_bits(y[:, :no], yc[:, :no])                                                           # (A)
    for c in range(Cn):                                                                               # (B)
        ref = O.PreDecim().feed(cf[c, :n])
        assert np.array_equal(bits(y[c, :no].cpu().numpy()).ravel(), bits(ref).ravel()), c
    y2, no2 = fe.predecim_dev(tx[:, :n], n_hist=96, abs0=107, offset=96)
    y2c, _ = fe.predecim_dev(tc[:, :n], n_hist=96, abs0=107, offset=96)
    assert no2 > 190 and same_bits(y2[:, :no2], y2c[:, :no2])
    # the channeliser converts with the same handle's numbers (it takes one channel: row 1 of the buffer)
    c1, n1 = fe.channelise_dev(tx[1, :n])
    c1c, _ = fe.channelise_dev(tc[1, :n])
    assert n1 == 204 and same_bits(c1[:, :n1], c1c[:, :n1])


# ---- 5: the channeliser ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["u8", "s16"])
def test_channeliser(O, FE, fmt):
    """n = 2008: 200 instants = three whole 64-instant tiles and a partial one; ranges with history, mixer phases, a bad pointer"""
    n = 2008
    spec = O.load_spec()
    hsum = float(np.abs(np.array(spec["pre_taps"], dtype=np.float64)).sum())
    x = noise(fmt, np.random.default_rng(5), 1504 + n)
    cf = conv(x)
    tol = 2e-6 * hsum * float(np.abs(cf).max())
    tx, tc = dev(x), dev(cf)
    fe = FE()

    import chz_model as CM

    def host(y, no):
        return y[:, :no].cpu().numpy().view(np.complex64)[..., 0]

    def close(y, no, ref, x, n_hist, abs0, what):
        CM.within(host(y, no), x, n_hist, abs0, k=CM.K_SPEC + CM.U, ref=ref, cap=tol, what="%s %s" % (fmt, what))
    y, no = fe.channelise_dev(tx[:n])
    yc, _ = fe.channelise_dev(tc[:n])
    assert no == 200 and same_bits(y[:, :no], yc[:, :no])
    ref = O.channelise(cf[:n])
    close(y, no, ref, cf[:n], 0, 0, "whole")
    close(yc, no, ref, cf[:n], 0, 0, "whole, cf32")                                                   # cf32
    for offset, n_hist in ((1000, 80), (1048, 96), (1504, 1504)):
        kw = dict(n_hist=n_hist, abs0=offset, offset=offset)
        y, no = fe.channelise_dev(tx[:offset + n], **kw)
        yc, noc = fe.channelise_dev(tc[:offset + n], **kw)
        assert no == noc and no >= 200 and same_bits(y[:, :no], yc[:, :no]), offset                   # (A)
        ref = O.channelise(cf[offset - n_hist:offset + n], n_hist=n_hist, abs0=offset)
        assert ref.shape[1] == no
        close(y, no, ref, cf[offset - n_hist:offset + n], n_hist, offset, "offset %d" % offset)       # (B)
        close(yc, no, ref, cf[offset - n_hist:offset + n], n_hist, offset, "offset %d, cf32" % offset)     # (B), cf32
        for k, r in ((1, 0), (1, 1), (3, 7), (5, 9), (1 << 20, 101), (7, 191)):                       # the mixer phase moves
            kw = dict(n_hist=n_hist, abs0=offset + 192 * k + r, offset=offset)
            y, no = fe.channelise_dev(tx[:offset + n], **kw)
            yc, noc = fe.channelise_dev(tc[:offset + n], **kw)
            assert no == noc and same_bits(y[:, :no], yc[:, :no]), (offset, k, r)
    # a pointer off the 16-byte grid is P25FE_ERR_ARG, also where it is still 4- or 8-byte aligned
    from p25rx_amd._lib import P25feError, ERR_ARG
    bps = 2 if fmt == "u8" else 4
    tried = set()
    for off in (1, 2, 3, 4, 6):
        if off * bps % 16 == 0:
            continue
        tried.add(off * bps % 16)
        for call in (fe.channelise_dev, fe.predecim_dev):
            with pytest.raises(P25feError) as ei:
                call(tx, n_hist=0, abs0=off, offset=off)
            assert ei.value.status == ERR_ARG, (off, call)
    assert {4, 8, 12} <= tried


# ---- 5b: stream positions past 2^31, 2^32, 2^40 and 2^56 ---------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["u8", "s16"])
def test_large_positions(O, FE, fmt):
    """Both stages at positions no 32-bit index holds: (A) against the cf32 call at the same position, and -- a range at position P
    computes what the same samples compute at any P' congruent to P modulo the stage's grid (10; 10 and 192 for the channeliser,
    docs/SPEC.md section 4) -- bit for bit against the narrow call at P mod 960.  2^62 and beyond is P25FE_ERR_ARG."""
    from p25rx_amd._lib import P25feError, ERR_ARG
    offset, n_hist, n = 1048, 96, 2008
    x = noise(fmt, np.random.default_rng(6), offset + n)
    tx, tc = dev(x), dev(conv(x))
    fe = FE()
    for big in (1 << 31, 1 << 32, 1 << 40, 1 << 56, (1 << 62) - 4000):
        for r in (0, 3, 7, 191, 957):
            P = big + r
            for call in (fe.predecim_dev, fe.channelise_dev):
                y, no = call(tx, n_hist=n_hist, abs0=P, offset=offset)
                yc, noc = call(tc, n_hist=n_hist, abs0=P, offset=offset)
                ys, nos = call(tx, n_hist=n_hist, abs0=P % 960, offset=offset)
                assert no == noc == nos and no >= 200, (P, call)
                assert same_bits(y[:, :no], yc[:, :no]), (P, call)
                assert same_bits(y[:, :no], ys[:, :no]), (P, call)
    for call in (fe.predecim_dev, fe.channelise_dev):
        for P in (1 << 62, (1 << 64) - 1):
            with pytest.raises(P25feError) as ei:
                call(tx, n_hist=n_hist, abs0=P, offset=offset)
            assert ei.value.status == ERR_ARG


# ---- 6: end to end -----------------------------------------------------------------------------------------------------------
def test_config3_from_u8(O, FE):
    """BASELINE.json config 3 from an RTL-SDR style capture: tests/test_gpu_parity.py's wideband capture (C4FM channel x 10 plus an
    interferer 300 kHz away) scaled by 0.5 and rounded to u8 -> predecim_dev(u8) -> run_dev = the oracle's dibits = the generator's"""
    from scipy import signal as sps
    from p25rx_amd import c4fm
    from p25rx_amd.frontend import parse_results
    iq, truth, _ = c4fm.synth(0.5, seed=12, snr_db=25.0)
    wide = sps.resample_poly(iq.astype(np.complex128), 10, 1)
    t = np.arange(len(wide)) / 2.4e6
    wide = (wide + 0.8 * np.exp(2j * np.pi * 300e3 * t)).astype(np.complex64)
    u8 = c4fm.to_u8(0.5 * wide)
    assert 0 < u8.min() and u8.max() < 255                           # nothing clipped
    cf = conv_u8(u8)
    x240 = O.PreDecim().feed(cf)
    ref = O.run_cf32(x240)
    k = min(len(ref), len(truth) - 24)
    assert k > 2300 and np.array_equal(ref[:k], truth[24:24 + k])    # 8 bits and the interferer: the symbols survive
    fe = FE()
    y, no = fe.predecim_dev(dev(u8))
    assert no == len(x240)
    assert np.array_equal(bits(y[0, :no].cpu().numpy()).ravel(), bits(x240).ravel())
    dib, res = fe.run_dev(y[:, :no])
    assert np.array_equal(dib[0, :int(parse_results(res)[0]["n_dibits"])].cpu().numpy(), ref)


def test_channeliser_end_to_end_from_s16(O, FE):
    """three C4FM carriers on raster slots of one 2.4 Msps capture, delivered as int16 -> channeliser -> the 192-channel front
    end: each carrier's dibits equal the generator's truth, idle slots never lock"""
    from p25rx_amd import c4fm
    from p25rx_amd.frontend import parse_results
    carriers = {5: (31, 1.0), 100: (32, 0.6), 190: (33, 0.8)}
    wide, truth = c4fm.synth_wideband(0.5, carriers, snr_db=22.0, seed=3)
    peak = float(max(np.abs(wide.real).max(), np.abs(wide.imag).max()))
    s16 = c4fm.to_s16(wide, full_scale=int(0.9 * 32767 / peak))     # scaled into range: the peak at 0.9 of full scale
    assert np.abs(s16.astype(np.int32)).max() < 32767
    fe = FE()
    yc, nc = fe.channelise_dev(dev(s16))
    fe192 = FE(n_channels=192)
    dib, res = fe192.run_dev(yc[:, :nc])
    r = parse_results(res)
    for c in range(192):
        nd = int(r["n_dibits"][c])
        if c in carriers:
            got = dib[c, :nd].cpu().numpy()
            k = min(len(got), len(truth[c]) - 24)
            assert k > 2000 and np.array_equal(got[:k], truth[c][24:24 + k]), c
        elif min(abs(c - k) if abs(c - k) <= 96 else 192 - abs(c - k) for k in carriers) > 1:
            assert int(r["n_sync"][c]) == 0, c                          # idle slot (adjacent slots see the skirt)
