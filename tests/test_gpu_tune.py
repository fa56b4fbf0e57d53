"""The tuner (docs/SPEC.md 3.0c, k_tune) on the GPU: bit for bit against tests/tune_model.py, against the resampler where it IS the
resampler, within SPEC 3.11's bound against the channeliser's oracle where it is the channeliser, and against itself across channel
counts, formats, ranges, positions and chunkings.

As in tests/test_gpu_resample.py the bit-exact cases use random, ASYMMETRIC tables, and the sizes are the smallest at which tiling
can go wrong: a sub-tile holds at most 256 outputs and a workgroup four sub-tiles, so >= 2400 outputs per row cover two full
workgroups and a partial one at every ratio.  The rotator tables come from the library's getter, which defines them."""
from math import gcd

import numpy as np
import pytest

import resample_model as RM
import tune_model as TM
from test_gpu_wide_fmt import _monotone_table, bits, conv, conv_u8, dev, noise, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def mods():
    from p25rx_amd import _lib
    from p25rx_amd.frontend import FrontEnd, Resampler, Tuner
    return _lib, FrontEnd, Resampler, Tuner


def rand_taps(rng, L, T):
    return (rng.standard_normal(L * T) * 0.1).astype(np.float32)


def cnoise(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def host(y, no, k):
    return y[k, :no].cpu().numpy().view(np.complex64)[..., 0]


_ROT = {}


def rot(TN, den):
    if den not in _ROT:
        _ROT[den] = TN.rotator(den)
    return _ROT[den]


def model(TN, x, L, M, T, taps, freqs):
    """[K, n_out] of the whole stream x from position 0"""
    return np.stack([TM.tune(x, L, M, T, taps, num, den, *rot(TN, den)) for num, den in freqs])


def check_rows(y, no, ref, what=None):
    assert no == ref.shape[1], (what, no, ref.shape)
    for k in range(ref.shape[0]):
        got = host(y, no, k)
        bad = np.flatnonzero((bits(got) != bits(ref[k])).reshape(no, 2).any(axis=1))
        assert bad.size == 0, (what, k, bad[:8], got[bad[:4]], ref[k][bad[:4]])


# the ranges' case: one capture and its whole-stream model rows, computed once and shared (never modified)
R_L, R_M, R_T, R_N = 12, 125, 84, 40003
R_FREQS = ((11, 200), (-37, 200), (0, 1))
R_GRID = 1000                                                        # lcm(M, den)


@pytest.fixture(scope="module")
def stream(mods):
    TN = mods[3]
    rng = np.random.default_rng(30)
    taps = rand_taps(rng, R_L, R_T)
    x = cnoise(rng, R_N)
    y = model(TN, x, R_L, R_M, R_T, taps, R_FREQS)
    y.setflags(write=False)
    x.setflags(write=False)
    return taps, x, y


# ---- 1: model parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(12, 125, 84, 40003, ((-37, 200), (11, 200), (0, 1))),
                                   (15, 128, 69, 33001, ((-825, 4096), (25, 8192), (0, 1), (1, 2))),
                                   (3, 250, 667, 200003, ((-399, 800), (241, 800), (0, 1))),
                                   (24, 25, 9, 4099, ((-7, 25), (12, 25), (0, 1)))], ids=lambda s: "%d_%d_%d" % s[:3])
def test_model_parity(mods, shape):
    """whole streams from position 0 (3840, 3867, 2400 and 3935 outputs per row): a negative, a positive and the zero frequency per
    ratio; rotators in LDS (den 200, 25, 2) and gathered (den 800, 4096, 8192)"""
    _lib, FE, RS, TN = mods
    L, M, T, n, freqs = shape
    rng = np.random.default_rng(20 + L)
    taps, x = rand_taps(rng, L, T), cnoise(rng, n)
    ref = model(TN, x, L, M, T, taps, freqs)
    fe = FE()
    tn = TN(fe, L, M, T, taps, freqs)
    y, no = tn.tune_dev(dev(x))
    assert no == RM.n_resample(L, M, 0, n) == int(fe.L.p25fe_n_resample(L, M, 0, n)) == tn.n_out(0, n) and no >= 2400
    assert tuple(y.shape[:1]) == (len(freqs),)
    check_rows(y, no, ref, shape[:3])


# ---- 2: channel count ---------------------------------------------------------------------------------------------------------
def test_channel_counts(mods):
    """K = 1 and K = 256 at 24/25, every row against the model (the kernel has no channel blocks: a channel is a workgroup).  The
    256 frequencies are (k - 100) / 200 reduced, wrapped into [-1/2, 1/2): 201 distinct ones, rows 201 .. 255 repeat rows 1 .. 55."""
    _lib, FE, RS, TN = mods
    L, M, T, n = 24, 25, 9, 4099
    rng = np.random.default_rng(60)
    taps, x = rand_taps(rng, L, T), cnoise(rng, n)
    freqs = []
    for k in range(256):
        num = (k % 200) - 100
        g = gcd(abs(num), 200)
        freqs.append((num // g, 200 // g))
    assert len(set(freqs)) == 200 and freqs[0] == (-1, 2) and freqs[100] == (0, 1) and freqs[1] == (-99, 200)
    ref = model(TN, x, L, M, T, taps, freqs)
    fe = FE()
    tx = dev(x)
    y, no = TN(fe, L, M, T, taps, freqs).tune_dev(tx)
    assert no == 3935
    check_rows(y, no, ref, "K=256")
    for k in (0, 1, 100, 255):
        y1, n1 = TN(fe, L, M, T, taps, [freqs[k]]).tune_dev(tx)
        assert tuple(y1.shape[:1]) == (1,)
        check_rows(y1, n1, ref[k:k + 1], "K=1 of row %d" % k)


# ---- 3: it is the resampler / the channeliser ---------------------------------------------------------------------------------
def test_is_the_resampler(mods, stream):
    _lib, FE, RS, TN = mods
    taps, x, y = stream
    fe = FE()
    tx = dev(x)
    g, no = TN(fe, R_L, R_M, R_T, taps, R_FREQS).tune_dev(tx)
    r, nr = RS(fe, R_L, R_M, R_T, taps).resample_dev(tx)
    assert no == nr and same_bits(g[2, :no], r[0, :nr])
    assert not same_bits(g[0, :no], r[0, :nr])


def test_is_the_channeliser(O, mods):
    """1/10, 80 taps, SPEC 3.0's table and c / 192 reduced: SPEC 3.11's formula in a fixed fp32 order, within 3.11's bound of its
    double-precision oracle"""
    _lib, FE, RS, TN = mods
    spec = O.load_spec()
    taps = np.array(spec["pre_taps"], dtype=np.float32)
    n = 7709
    x = cnoise(np.random.default_rng(1), n)
    ref = O.channelise(x)
    chans = (0, 5, 100)
    freqs = [(0, 1), (5, 192), (-23, 48)]                            # 100 / 192 is -92 / 192
    fe = FE()
    y, no = TN(fe, 1, 10, 80, taps, freqs).tune_dev(dev(x))
    assert no == ref.shape[1] == 770
    bound = 2e-6 * float(np.abs(taps.astype(np.float64)).sum()) * float(np.abs(x).max())
    for k, c in enumerate(chans):
        err = float(np.abs(host(y, no, k).astype(np.complex128) - ref[c].astype(np.complex128)).max())
        print("channel %d: max error %.3e, bound %.3e" % (c, err, bound))
        assert err <= bound, (c, err, bound)


# ---- 4: ranges ----------------------------------------------------------------------------------------------------------------
def test_ranges(mods, stream):
    """tests/test_gpu_resample.py::test_ranges for two mixed channels and the centre: ranges in the middle of the capture at odd
    positions that are multiples of neither M, L, den nor the 16-byte vector, each in a buffer of its own -- [junk | n_hist samples
    of history | the range] -- with its position as abs_first"""
    import torch
    _lib, FE, RS, TN = mods
    taps, x, y = stream
    L, M, T = R_L, R_M, R_T
    K = len(R_FREQS)
    fe = FE()
    tn = TN(fe, L, M, T, taps, R_FREQS)
    tx = dev(x)
    junk = cnoise(np.random.default_rng(31), 2) * 1000

    def call(a, n, n_hist):
        lead = (n_hist + 1) // 2 * 2
        buf = np.concatenate([junk[:lead - n_hist], x[a - n_hist:a + n]])
        g, no = tn.tune_dev(dev(buf), n_hist=n_hist, abs0=a, offset=lead)
        return np.stack([host(g, no, k) for k in range(K)])
    for a, n in ((5007, 3001), (12347, 20001), (127, 1)):
        assert a % M and a % L and a % 2 and a % 200
        first, cnt = a * L // M, RM.n_resample(L, M, a, n)
        for n_hist in (T - 1, T + 13, a):
            g = call(a, n, n_hist)
            assert g.shape == (K, cnt) and np.array_equal(bits(g), bits(y[:, first:first + cnt])), (a, n, n_hist)
        z = np.array(x[:a + n])
        for n_hist in (0, 40):                                       # less history than T - 1: what is missing reads as zero
            z[:a] = x[:a]
            z[:a - n_hist] = 0
            g = call(a, n, n_hist)
            want = model(TN, z, L, M, T, taps, R_FREQS)[:, first:first + cnt]
            assert g.shape == (K, cnt) and np.array_equal(bits(g), bits(want)), (a, n, n_hist)
    a, n = 5006, 3001                                                # in place: abs_first == offset
    first, cnt = a * L // M, RM.n_resample(L, M, a, n)
    for n_hist in (T - 1, T + 13, a):
        g, no = tn.tune_dev(tx[:a + n], n_hist=n_hist, abs0=a, offset=a)
        check_rows(g, no, y[:, first:first + cnt], n_hist)
    # three consecutive ranges of odd lengths: the whole stream
    cuts = (0, 13339, 13339 + 11111, R_N)
    assert all((b - a) % 2 == 1 for a, b in zip(cuts, cuts[1:]))
    parts = [call(a, b - a, min(a, T - 1)) for a, b in zip(cuts, cuts[1:])]
    assert np.array_equal(bits(np.concatenate(parts, axis=1)), bits(y))
    # a range that owns no output: count 0, nothing written
    a, n = 5012, 8
    assert RM.n_resample(L, M, a, n) == 0
    out = torch.full((K, 16, 2), -7.5, device="cuda")
    g, no = tn.tune_dev(tx[:a + n], n_hist=T - 1, abs0=a, offset=a, out=out)
    assert no == 0 and bool((out == -7.5).all())
    # a pointer off the 16-byte grid
    with pytest.raises(_lib.P25feError) as ei:
        tn.tune_dev(tx[:6000], n_hist=T - 1, abs0=5007, offset=5007)
    assert ei.value.status == _lib.ERR_ARG


# ---- 5: guards ----------------------------------------------------------------------------------------------------------------
def test_guards(mods, stream):
    """rows with a stride larger than needed, a guard value everywhere: nothing is written from n_out on, nor between the rows;
    out_stride < n_out is an argument error and writes nothing"""
    import torch
    _lib, FE, RS, TN = mods
    taps, x, y = stream
    K, n = len(R_FREQS), 8995
    fe = FE()
    tn = TN(fe, R_L, R_M, R_T, taps, R_FREQS)
    tx = dev(x[:n])
    cnt = RM.n_resample(R_L, R_M, 0, n)
    sentinel = -123456.75
    out = torch.full((K, cnt + 37, 2), sentinel, device="cuda")
    g, no = tn.tune_dev(tx, out=out)
    assert no == cnt and g.data_ptr() == out.data_ptr()
    assert bool((out[:, cnt:] == sentinel).all())
    check_rows(out, cnt, y[:, :cnt])
    small = torch.full((K, cnt - 1, 2), sentinel, device="cuda")
    with pytest.raises(_lib.P25feError) as ei:
        tn.tune_dev(tx, out=small)
    assert ei.value.status == _lib.ERR_ARG and bool((small == sentinel).all())


# ---- 6: formats ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [(12, 125, 84, ((11, 200), (-37, 200), (0, 1), (1, 3))),
                                   (15, 128, 69, ((-825, 4096), (7, 16), (0, 1), (1, 2), (-2, 5)))],
                         ids=lambda r: "%d_%d" % r[:2])
@pytest.mark.parametrize("kind", ["u8", "u8_lut", "s16"])
def test_formats(mods, kind, ratio):
    """u8 with the default affine table, u8 with a table that is not affine and s16, the formats' extremes spliced in: bit for bit
    the cf32 call on the converted samples with the same n_hist / abs_first / offset, and the model where it applies.  Denominators
    below the samples per 16-byte vector (2, 3, 5 against 4 or 8) are among the channels."""
    _lib, FE, RS, TN = mods
    L, M, T, freqs = ratio
    rng = np.random.default_rng(50)
    taps = rand_taps(rng, L, T)
    n = 12003
    fmt = "s16" if kind == "s16" else "u8"
    table = _monotone_table() if kind == "u8_lut" else None
    fe = FE(u8_lut=table, specialize=_lib.SPECIALIZE_OFF) if table is not None else FE()
    tn = TN(fe, L, M, T, taps, freqs)
    x = noise(fmt, rng, n)
    cf = conv_u8(x, table) if fmt == "u8" else conv(x)
    tx, tc = dev(x), dev(cf)
    ref = model(TN, cf, L, M, T, taps, freqs)
    for kw in (dict(), dict(n_hist=T - 1, abs0=2008, offset=2008), dict(n_hist=96, abs0=7 * M + 5, offset=1048),
               dict(n_hist=8, abs0=3, offset=8)):
        y, no = tn.tune_dev(tx, **kw)
        yc, nc = tn.tune_dev(tc, **kw)
        assert no == nc and no > 950 and same_bits(y[:, :no], yc[:, :nc]), (kind, kw)      # (959 at 12/125 from 2008 on)
        if kw.get("abs0", 0) == kw.get("offset", 0) and kw.get("n_hist", 0) in (0, T - 1):
            first = kw.get("abs0", 0) * L // M
            check_rows(y, no, ref[:, first:first + no], (kind, kw))


# ---- 7: positions -------------------------------------------------------------------------------------------------------------
def test_large_positions(mods, stream):
    """abs_first = q lcm(M, den) + r with the multiple just past 2^31, 2^32, 2^40 and 2^56: the bits and the count of position r;
    2^62 and beyond is P25FE_ERR_ARG; a position congruent mod M but not mod den changes the mixed rows and not the centre's"""
    _lib, FE, RS, TN = mods
    taps, x, _ = stream
    L, M, T = R_L, R_M, R_T
    fe = FE()
    tn = TN(fe, L, M, T, taps, R_FREQS)
    offset, n_hist = 1048, 96
    tx = dev(x[:offset + 6007])
    for r in (0, 1, 7, 77, 124, 199):
        ys, ns = tn.tune_dev(tx, n_hist=n_hist, abs0=r, offset=offset)
        for two in (31, 32, 40, 56):
            q = ((1 << two) // R_GRID + 1) * R_GRID
            y, no = tn.tune_dev(tx, n_hist=n_hist, abs0=q + r, offset=offset)
            assert no == ns == RM.n_resample(L, M, q + r, 6007) and no > 570, (two, r)
            assert same_bits(y[:, :no], ys[:, :ns]), (two, r)
        ym, nm = tn.tune_dev(tx, n_hist=n_hist, abs0=(1 << 40) // R_GRID * R_GRID + R_GRID + M + r, offset=offset)
        assert nm == ns and same_bits(ym[2, :nm], ys[2, :ns]), r
        assert not same_bits(ym[0, :nm], ys[0, :ns]) and not same_bits(ym[1, :nm], ys[1, :ns]), r
    y, no = tn.tune_dev(tx, n_hist=n_hist, abs0=(1 << 62) - 1, offset=offset)
    assert no == RM.n_resample(L, M, (1 << 62) - 1, 6007)
    for P in (1 << 62, (1 << 64) - 1):
        with pytest.raises(_lib.P25feError) as ei:
            tn.tune_dev(tx, n_hist=n_hist, abs0=P, offset=offset)
        assert ei.value.status == _lib.ERR_ARG


# ---- 8: host streaming form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["cf32", "u8", "s16"])
def test_host_streaming(mods, stream, fmt):
    """one call = five chunks of uneven sizes = tune_dev; a cap too small is P25FE_ERR_CAPACITY and changes nothing; reset restarts
    at position 0; another format within a stream is P25FE_ERR_FORMAT"""
    import ctypes as C
    _lib, FE, RS, TN = mods
    taps, xs, ys = stream
    L, M, T = R_L, R_M, R_T
    K, n = len(R_FREQS), 20011
    if fmt == "cf32":
        x, unit = np.array(xs[:n]), 1
        ref = ys[:, :RM.n_resample(L, M, 0, n)]
    else:
        x, unit = noise(fmt, np.random.default_rng(70), n), 2
        ref = model(TN, conv(x), L, M, T, taps, R_FREQS)
    fe = FE()
    tn = TN(fe, L, M, T, taps, R_FREQS)
    one = tn.tune(x)
    assert one.shape == ref.shape and np.array_equal(bits(one), bits(ref))
    yd, nd = tn.tune_dev(dev(x))
    check_rows(yd, nd, one)
    tn.reset()
    cuts = (0, 1, 50, 8007, 8010, n)                                 # 1, 49 (both shorter than the history), 7957, 3, 12001
    parts = [tn.tune(x[unit * a:unit * b]) for a, b in zip(cuts, cuts[1:])]
    assert parts[0].shape == (K, 0) and np.array_equal(bits(np.concatenate(parts, axis=1)), bits(one))
    # capacity
    tn.reset()
    head = tn.tune(x[:unit * 9001])
    need = RM.n_resample(L, M, 9001, n - 9001)
    out = np.full((K, need), np.complex64(-3.25), dtype=np.complex64)
    no = C.c_size_t(0)
    tail = np.ascontiguousarray(x[unit * 9001:])
    rc = fe.L.p25fe_tune(tn.tn, tail.ctypes.data_as(C.c_void_p), {"cf32": 0, "u8": 1, "s16": 2}[fmt], n - 9001,
                         out.ctypes.data_as(C.c_void_p), need - 1, C.byref(no))
    assert rc == _lib.ERR_CAPACITY and no.value == need and (out == np.complex64(-3.25)).all()
    rest = tn.tune(tail)
    assert np.array_equal(bits(np.concatenate([head, rest], axis=1)), bits(one))
    # another format in the same stream
    other = np.zeros(16, dtype=np.int16) if fmt != "s16" else np.zeros(16, dtype=np.uint8)
    with pytest.raises(_lib.P25feError) as ei:
        tn.tune(other)
    assert ei.value.status == _lib.ERR_FORMAT
    tn.reset()
    assert np.array_equal(bits(tn.tune(x[:unit * 5000])), bits(one[:, :RM.n_resample(L, M, 0, 5000)]))


# ---- 9: end to end ------------------------------------------------------------------------------------------------------------
def test_end_to_end(O, mods):
    """four C4FM sources in one 2.5 Msps capture (two of them adjacent 12.5 kHz channels), the designed table, the tuner, a
    four-channel handle's receive chain on its rows: the oracle's dibits on the model's rows, bit for bit, and the generators'
    symbols without an error"""
    from p25rx_amd.frontend import parse_results
    _lib, FE, RS, TN = mods
    fs, offsets = 2500000, (-412500, 137500, 150000, 0)
    wide, truths = TM.site_capture(fs, 125, 12, offsets)
    L, M, T, taps, freqs = TN.design(fs, offsets)
    assert (L, M, T) == (12, 125, 84) and freqs == [(-33, 200), (11, 200), (3, 50), (0, 1)]
    rows = model(TN, wide, L, M, T, taps, freqs)
    fe1, fe4 = FE(), FE(n_channels=4)
    y, no = TN(fe1, L, M, T, taps, freqs).tune_dev(dev(wide))
    check_rows(y, no, rows)
    dib, res = fe4.run_dev(y[:, :no])
    for k in range(4):
        ref = O.run_cf32(rows[k])
        got = dib[k, :int(parse_results(res)[k]["n_dibits"])].cpu().numpy()
        kk = min(len(ref), len(truths[k]) - 24)
        assert kk > 1100 and np.array_equal(got, ref), k
        assert np.array_equal(got[:kk], truths[k][24:24 + kk]), k


# ---- 10: lifetimes ------------------------------------------------------------------------------------------------------------
def test_destroy_after_the_handle(mods, stream):
    """p25fe_tuner_destroy after p25fe_destroy of its handle (a garbage collector's order) neither fails nor leaves an error behind
    for the next call of the thread"""
    _lib, FE, RS, TN = mods
    taps, x, y = stream
    for _ in range(3):
        fe = FE()
        tn = TN(fe, R_L, R_M, R_T, taps, R_FREQS)
        fe.close()                                                   # the handle first
        junk = [FE() for _ in range(2)]                              # its memory is handed out again
        tn.close()
        del junk
        fe2 = FE()
        tn2 = TN(fe2, R_L, R_M, R_T, taps, R_FREQS)
        g, no = tn2.tune_dev(dev(x[:4001]))
        assert no == RM.n_resample(R_L, R_M, 0, 4001)
        check_rows(g, no, y[:, :no])
        assert np.array_equal(bits(tn2.tune(np.array(x[:4001]))), bits(y[:, :no]))
