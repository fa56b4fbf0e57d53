"""The tuner's NCO channels (docs/SPEC.md 3.0d, k_tune_nco) on the GPU: bit for bit against tests/tune_nco_model.py, against the
resampler where a channel IS the resampler, against the rational tuner where it IS one of its channels, and against itself across
channel counts, formats, ranges, positions and chunkings.

Sizes and tables are tests/test_gpu_tune.py's: random, ASYMMETRIC tables and >= 2400 outputs per row, which are two full workgroups
and a partial one at every ratio.  The rotator table comes from the library's getter, which defines it."""
import numpy as np
import pytest

import resample_model as RM
import tune_model as TM
import tune_nco_model as NM
from test_gpu_tune import cnoise, host, rand_taps
from test_gpu_wide_fmt import _monotone_table, bits, conv, conv_u8, dev, noise, same_bits

pytestmark = pytest.mark.gpu

OFF_A, OFF_B = 232387521, -3527459                                   # two steps off every raster (135 268.1 Hz and -2 053.3 Hz at 2.5 Msps)
STEPS = (0, 1, -1, 0x7fffffff, -(1 << 31), 11 << 24, OFF_A, OFF_B)
GRID32 = 125 << 32                                                   # lcm(M, 2^32) at M = 125


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def mods():
    from p25rx_amd import _lib
    from p25rx_amd.frontend import FrontEnd, Resampler, Tuner
    return _lib, FrontEnd, Resampler, Tuner


@pytest.fixture(scope="module")
def rot(mods):
    return mods[3].rotator(256)


def model(rot, x, L, M, T, taps, steps):
    """[K, n_out] of the whole stream x from position 0"""
    return np.stack([NM.tune_nco(x, L, M, T, taps, st, *rot) for st in steps])


def check_rows(y, no, ref, what=None):
    assert no == ref.shape[1], (what, no, ref.shape)
    for k in range(ref.shape[0]):
        got = host(y, no, k)
        bad = np.flatnonzero((bits(got) != bits(ref[k])).reshape(no, 2).any(axis=1))
        assert bad.size == 0, (what, k, bad[:8], got[bad[:4]], ref[k][bad[:4]])


# the ranges' case: one capture and its whole-stream model rows, computed once and shared (never modified)
R_L, R_M, R_T, R_N = 12, 125, 84, 40003
R_STEPS = (OFF_A, OFF_B, 0)


@pytest.fixture(scope="module")
def stream(rot):
    rng = np.random.default_rng(30)
    taps = rand_taps(rng, R_L, R_T)
    x = cnoise(rng, R_N)
    y = model(rot, x, R_L, R_M, R_T, taps, R_STEPS)
    y.setflags(write=False)
    x.setflags(write=False)
    return taps, x, y


# ---- 1: model parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(12, 125, 84, 40003), (15, 128, 69, 33001)], ids=lambda s: "%d_%d" % s[:2])
def test_model_parity(mods, rot, shape):
    """whole streams from position 0 (3840 and 3867 outputs per row): the centre, the smallest steps, the largest, Nyquist, a
    step on the table's raster (residual 0) and two off every raster"""
    _lib, FE, RS, TN = mods
    L, M, T, n = shape
    rng = np.random.default_rng(20 + L)
    taps, x = rand_taps(rng, L, T), cnoise(rng, n)
    ref = model(rot, x, L, M, T, taps, STEPS)
    fe = FE()
    tn = TN.nco(fe, L, M, T, taps, STEPS)
    y, no = tn.tune_dev(dev(x))
    assert no == RM.n_resample(L, M, 0, n) == tn.n_out(0, n) and no >= 2400
    assert tuple(y.shape[:1]) == (len(STEPS),)
    check_rows(y, no, ref, shape[:3])


# ---- 2: it is the resampler / the rational tuner ------------------------------------------------------------------------------
def test_is_the_resampler(mods, stream):
    _lib, FE, RS, TN = mods
    taps, x, y = stream
    fe = FE()
    tx = dev(x)
    g, no = TN.nco(fe, R_L, R_M, R_T, taps, R_STEPS).tune_dev(tx)
    r, nr = RS(fe, R_L, R_M, R_T, taps).resample_dev(tx)
    assert no == nr and same_bits(g[2, :no], r[0, :nr])
    assert not same_bits(g[0, :no], r[0, :nr])


def test_is_the_rational_tuner(mods, stream):
    """step = num 2^24 is the rational channel num / 256, at position 0 and at an odd position past 2^40"""
    _lib, FE, RS, TN = mods
    taps, x, _ = stream
    nums = (1, -37, 55, 127, -127)
    fe = FE()
    a = TN.nco(fe, R_L, R_M, R_T, taps, [v << 24 for v in nums])
    b = TN(fe, R_L, R_M, R_T, taps, [(v, 256) for v in nums])
    offset, n_hist = 1048, 96
    tx = dev(x[:offset + 6007])
    for pos in (0, 12345, (1 << 40) + 77):
        ya, na = a.tune_dev(tx, n_hist=n_hist, abs0=pos, offset=offset)
        yb, nb = b.tune_dev(tx, n_hist=n_hist, abs0=pos, offset=offset)
        assert na == nb and na > 570 and same_bits(ya[:, :na], yb[:, :nb]), pos
    ya, na = a.tune_dev(dev(x))
    yb, nb = b.tune_dev(dev(x))
    assert na == nb == 3840 and same_bits(ya[:, :na], yb[:, :nb])


# ---- 3: channel count ---------------------------------------------------------------------------------------------------------
def test_channel_counts(mods, rot):
    """K = 1, 3, 64 and 256 at 24/25, every row against the model (a channel is a workgroup): 256 distinct steps, the centre among
    them; the smaller objects take rows of the largest"""
    _lib, FE, RS, TN = mods
    L, M, T, n = 24, 25, 9, 4099
    rng = np.random.default_rng(60)
    taps, x = rand_taps(rng, L, T), cnoise(rng, n)
    steps = [int(s) for s in rng.integers(-(1 << 31), 1 << 31, size=256)]
    steps[100] = 0
    ref = model(rot, x, L, M, T, taps, steps)
    fe = FE()
    tx = dev(x)
    for K, rows in ((256, range(256)), (64, range(64, 128)), (3, (99, 100, 255)), (1, (0,)), (1, (100,))):
        rows = list(rows)
        y, no = TN.nco(fe, L, M, T, taps, [steps[k] for k in rows]).tune_dev(tx)
        assert no == 3935 and tuple(y.shape[:1]) == (K,)
        check_rows(y, no, ref[rows], "K=%d" % K)


# ---- 4: ranges ----------------------------------------------------------------------------------------------------------------
def test_ranges(mods, rot, stream):
    """tests/test_gpu_tune.py::test_ranges for two mixed channels and the centre: ranges in the middle of the capture at odd
    positions that are multiples of neither M, L nor the 16-byte vector, each in a buffer of its own -- [junk | n_hist samples of
    history | the range] -- with its position as abs_first; n_hist below and above T - 1"""
    import torch
    _lib, FE, RS, TN = mods
    taps, x, y = stream
    L, M, T = R_L, R_M, R_T
    K = len(R_STEPS)
    fe = FE()
    tn = TN.nco(fe, L, M, T, taps, R_STEPS)
    tx = dev(x)
    junk = cnoise(np.random.default_rng(31), 2) * 1000

    def call(a, n, n_hist):
        lead = (n_hist + 1) // 2 * 2
        buf = np.concatenate([junk[:lead - n_hist], x[a - n_hist:a + n]])
        g, no = tn.tune_dev(dev(buf), n_hist=n_hist, abs0=a, offset=lead)
        return np.stack([host(g, no, k) for k in range(K)])
    for a, n in ((5007, 3001), (12347, 20001), (127, 1)):
        assert a % M and a % L and a % 2
        first, cnt = a * L // M, RM.n_resample(L, M, a, n)
        for n_hist in (T - 1, T + 13, a):
            g = call(a, n, n_hist)
            assert g.shape == (K, cnt) and np.array_equal(bits(g), bits(y[:, first:first + cnt])), (a, n, n_hist)
        z = np.array(x[:a + n])
        for n_hist in (0, 40):                                       # less history than T - 1: what is missing reads as zero
            z[:a] = x[:a]
            z[:a - n_hist] = 0
            g = call(a, n, n_hist)
            want = model(rot, z, L, M, T, taps, R_STEPS)[:, first:first + cnt]
            assert g.shape == (K, cnt) and np.array_equal(bits(g), bits(want)), (a, n, n_hist)
    a, n = 5006, 3001                                                # in place: abs_first == offset
    first, cnt = a * L // M, RM.n_resample(L, M, a, n)
    for n_hist in (T - 1, T + 13, a):
        g, no = tn.tune_dev(tx[:a + n], n_hist=n_hist, abs0=a, offset=a)
        check_rows(g, no, y[:, first:first + cnt], n_hist)
    # three consecutive ranges of odd lengths: the whole stream
    cuts = (0, 13339, 13339 + 11111, R_N)
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
    K, n = len(R_STEPS), 8995
    fe = FE()
    tn = TN.nco(fe, R_L, R_M, R_T, taps, R_STEPS)
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
@pytest.mark.parametrize("ratio", [(12, 125, 84), (15, 128, 69)], ids=lambda r: "%d_%d" % r[:2])
@pytest.mark.parametrize("kind", ["u8", "u8_lut", "s16"])
def test_formats(mods, rot, kind, ratio):
    """u8 with the default affine table, u8 with a table that is not affine and s16, the formats' extremes spliced in: bit for bit
    the cf32 call on the converted samples with the same n_hist / abs_first / offset, and the model where it applies.  The element
    offsets 2008, 1048 and 8 with positions 2008, 7 M + 5 and 3 put the window at every alignment of a 4- and an 8-sample vector."""
    _lib, FE, RS, TN = mods
    L, M, T = ratio
    steps = (OFF_A, OFF_B, 0, -(1 << 31), 1)
    rng = np.random.default_rng(50)
    taps = rand_taps(rng, L, T)
    n = 12003
    fmt = "s16" if kind == "s16" else "u8"
    table = _monotone_table() if kind == "u8_lut" else None
    fe = FE(u8_lut=table, specialize=_lib.SPECIALIZE_OFF) if table is not None else FE()
    tn = TN.nco(fe, L, M, T, taps, steps)
    x = noise(fmt, rng, n)
    cf = conv_u8(x, table) if fmt == "u8" else conv(x)
    tx, tc = dev(x), dev(cf)
    ref = model(rot, cf, L, M, T, taps, steps)
    for kw in (dict(), dict(n_hist=T - 1, abs0=2008, offset=2008), dict(n_hist=96, abs0=7 * M + 5, offset=1048),
               dict(n_hist=8, abs0=3, offset=8)):
        y, no = tn.tune_dev(tx, **kw)
        yc, nc = tn.tune_dev(tc, **kw)
        assert no == nc and no > 950 and same_bits(y[:, :no], yc[:, :nc]), (kind, kw)
        if kw.get("abs0", 0) == kw.get("offset", 0) and kw.get("n_hist", 0) in (0, T - 1):
            first = kw.get("abs0", 0) * L // M
            check_rows(y, no, ref[:, first:first + no], (kind, kw))


# ---- 7: positions -------------------------------------------------------------------------------------------------------------
def test_straddles_two_to_the_32(mods, rot, stream):
    """a range whose positions run through 2^32, against the model at those positions (the phase wraps with the register): the
    model's stream starts on the output grid, at the multiple of M below the history, with zeros up to it"""
    _lib, FE, RS, TN = mods
    taps, x, _ = stream
    L, M, T = R_L, R_M, R_T
    n, a0 = 11000, (1 << 32) - 5001                                  # the range starts below 2^32 and ends above it
    xs = np.array(x[:T - 1 + n])                                     # T - 1 samples of history, then the range
    s0 = (a0 - (T - 1)) // M * M
    pad = a0 - (T - 1) - s0
    z = np.concatenate([np.zeros(pad, dtype=np.complex64), xs])
    want = np.stack([RM.resample(NM.mix_nco(z, st, s0, *rot), L, M, T, taps) for st in R_STEPS])
    a_loc = pad + T - 1
    first, cnt = a_loc * L // M, RM.n_resample(L, M, a0, n)
    assert cnt == RM.n_resample(L, M, a_loc, n) and cnt > 1000
    fe = FE()
    tn = TN.nco(fe, L, M, T, taps, R_STEPS)
    buf = np.concatenate([np.full(1, 1000 + 1000j, dtype=np.complex64), xs])     # one sample of junk: owned sample 0 is 16-byte aligned
    assert (T - 1) % 2 == 1
    g, no = tn.tune_dev(dev(buf), n_hist=T - 1, abs0=a0, offset=T)
    check_rows(g, no, want[:, first:first + cnt], "2^32")


def test_large_positions(mods, stream):
    """abs_first = q lcm(M, 2^32) + r with the multiple just past 2^40 and 2^56 (at 15/128, where the grid is 2^32, also just past
    2^32): the bits and the count of position r; a position congruent mod M alone changes the mixed rows and not the step-0 row;
    2^62 and beyond is P25FE_ERR_ARG"""
    _lib, FE, RS, TN = mods
    taps, x, _ = stream
    L, M, T = R_L, R_M, R_T
    fe = FE()
    tn = TN.nco(fe, L, M, T, taps, R_STEPS)
    offset, n_hist = 1048, 96
    tx = dev(x[:offset + 6007])
    for r in (0, 1, 7, 77, 124, 199):
        ys, ns = tn.tune_dev(tx, n_hist=n_hist, abs0=r, offset=offset)
        for two in (40, 56):
            q = ((1 << two) // GRID32 + 1) * GRID32
            y, no = tn.tune_dev(tx, n_hist=n_hist, abs0=q + r, offset=offset)
            assert no == ns == RM.n_resample(L, M, q + r, 6007) and no > 570, (two, r)
            assert same_bits(y[:, :no], ys[:, :ns]), (two, r)
        ym, nm = tn.tune_dev(tx, n_hist=n_hist, abs0=(1 << 40) // M * M + M + r, offset=offset)
        assert nm == ns and same_bits(ym[2, :nm], ys[2, :ns]), r
        assert not same_bits(ym[0, :nm], ys[0, :ns]) and not same_bits(ym[1, :nm], ys[1, :ns]), r
    y, no = tn.tune_dev(tx, n_hist=n_hist, abs0=(1 << 62) - 1, offset=offset)
    assert no == RM.n_resample(L, M, (1 << 62) - 1, 6007)
    for P in (1 << 62, (1 << 64) - 1):
        with pytest.raises(_lib.P25feError) as ei:
            tn.tune_dev(tx, n_hist=n_hist, abs0=P, offset=offset)
        assert ei.value.status == _lib.ERR_ARG
    # 15/128: lcm(M, 2^32) = 2^32
    L2, M2, T2 = 15, 128, 69
    taps2 = rand_taps(np.random.default_rng(71), L2, T2)
    t2 = TN.nco(fe, L2, M2, T2, taps2, R_STEPS)
    for r in (0, 77, 127):
        ys, ns = t2.tune_dev(tx, n_hist=n_hist, abs0=r, offset=offset)
        for q in (1 << 32, (1 << 40) + (1 << 32), (1 << 56) + (1 << 32)):
            y, no = t2.tune_dev(tx, n_hist=n_hist, abs0=q + r, offset=offset)
            assert no == ns and no > 700 and same_bits(y[:, :no], ys[:, :ns]), (q, r)


# ---- 8: host streaming form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["cf32", "u8", "s16"])
def test_host_streaming(mods, rot, stream, fmt):
    """one call = five chunks of uneven sizes = tune_dev; a cap too small is P25FE_ERR_CAPACITY and changes nothing; reset restarts
    at position 0; another format within a stream is P25FE_ERR_FORMAT"""
    import ctypes as C
    _lib, FE, RS, TN = mods
    taps, xs, ys = stream
    L, M, T = R_L, R_M, R_T
    K, n = len(R_STEPS), 20011
    if fmt == "cf32":
        x, unit = np.array(xs[:n]), 1
        ref = ys[:, :RM.n_resample(L, M, 0, n)]
    else:
        x, unit = noise(fmt, np.random.default_rng(70), n), 2
        ref = model(rot, conv(x), L, M, T, taps, R_STEPS)
    fe = FE()
    tn = TN.nco(fe, L, M, T, taps, R_STEPS)
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
E_FS, E_OFFSETS = 2500000, (-412500 + 1871.3, 137500 - 2210.7, 150000 - 2411.6, 733.1)


@pytest.fixture(scope="module")
def site():
    """four C4FM sources a crystal's few ppm off the 12.5 kHz raster in one 2.5 Msps capture, and the generators' symbols"""
    wide, truths = TM.site_capture(E_FS, 125, 12, E_OFFSETS)
    wide.setflags(write=False)
    return wide, truths


def test_end_to_end(O, mods, rot, site):
    """the designed table, the NCO tuner at the exact offsets, a four-channel handle's receive chain on its rows: the model's rows
    bit for bit, the oracle's dibits on the model's rows, and the generators' symbols without an error"""
    from p25rx_amd.frontend import parse_results
    _lib, FE, RS, TN = mods
    wide, truths = site
    L, M, T, taps, steps = TN.design_nco(E_FS, E_OFFSETS)
    assert (L, M, T) == (12, 125, 84) and all(s % (1 << 24) for s in steps)
    rows = model(rot, wide, L, M, T, taps, steps)
    fe1, fe4 = FE(), FE(n_channels=4)
    y, no = TN.nco(fe1, L, M, T, taps, steps).tune_dev(dev(wide))
    check_rows(y, no, rows)
    dib, res = fe4.run_dev(y[:, :no])
    for k in range(4):
        ref = O.run_cf32(rows[k])
        got = dib[k, :int(parse_results(res)[k]["n_dibits"])].cpu().numpy()
        kk = min(len(ref), len(truths[k]) - 24)
        assert kk > 1100 and np.array_equal(got, ref), k
        assert np.array_equal(got[:kk], truths[k][24:24 + kk]), k


def test_replay_tunes_off_the_raster(site, tmp_path):
    """p25fe_replay -r 2500000 -F 135289.3 decodes the capture's second source; on the raster beside it (-f 137500) it finds no
    frame; -f and -F together are a usage error"""
    import os
    import subprocess
    wide, truths = site
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "p25fe_replay")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    src, out, out2 = tmp_path / "cap.cf32", tmp_path / "dib.out", tmp_path / "dib2.out"
    np.asarray(wide).tofile(src)
    assert abs(E_OFFSETS[1] - 135289.3) < 1e-6
    r = subprocess.run([exe, "-r", str(E_FS), "-F", "135289.3", "cf32", str(src), str(out)], capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stderr[-1000:]
    got = np.fromfile(out, dtype=np.uint8)
    kk = min(len(got), len(truths[1]) - 24)
    assert kk > 1100 and np.array_equal(got[:kk], truths[1][24:24 + kk])
    r = subprocess.run([exe, "-r", str(E_FS), "-f", "137500", "cf32", str(src), str(out2)], capture_output=True, text=True, timeout=100)
    assert r.returncode == 0 and len(np.fromfile(out2, dtype=np.uint8)) == 0, r.stderr[-1000:]
    r = subprocess.run([exe, "-r", str(E_FS), "-f", "137500", "-F", "135289.3", "cf32", str(src), str(out2)], capture_output=True, text=True)
    assert r.returncode != 0 and "usage" in r.stderr


# ---- 10: lifetimes ------------------------------------------------------------------------------------------------------------
def test_destroy_after_the_handle(mods, stream):
    """p25fe_tuner_destroy of an NCO tuner after p25fe_destroy of its handle neither fails nor leaves an error behind for the next
    call of the thread"""
    _lib, FE, RS, TN = mods
    taps, x, y = stream
    for _ in range(3):
        fe = FE()
        tn = TN.nco(fe, R_L, R_M, R_T, taps, R_STEPS)
        fe.close()                                                   # the handle first
        junk = [FE() for _ in range(2)]                              # its memory is handed out again
        tn.close()
        del junk
        fe2 = FE()
        tn2 = TN.nco(fe2, R_L, R_M, R_T, taps, R_STEPS)
        g, no = tn2.tune_dev(dev(x[:4001]))
        assert no == RM.n_resample(R_L, R_M, 0, 4001)
        check_rows(g, no, y[:, :no])
        assert np.array_equal(bits(tn2.tune(np.array(x[:4001]))), bits(y[:, :no]))
