"""The rational resampler (docs/SPEC.md 3.0b, k_resample) on the GPU: bit for bit against tests/resample_model.py, against K0 where
it IS K0, and against itself across formats, ranges, positions and chunkings.

The bit-exact cases use random, ASYMMETRIC tables: a designed prototype is symmetric and would hide a reversed tap or phase order.
A sub-tile of the kernel holds at most 256 outputs and a workgroup at most four sub-tiles.  No case of THIS file reaches that: what
the launch makes of its ratios is 180 outputs per sub-tile at 12/125 and 15/128, 17 at 3/250, 192 at 24/25 and 1/10, 128 at 2/25, so
the parity sizes below -- 2400 to 3935 outputs -- cover at least two full workgroups and a partial one at every ratio here.  The
256-output sub-tile, every other launch plan the shape limits admit (lane counts, outputs per lane, tiles down to one output) and
the tap loop's short paths are run by tests/test_gpu_resample_shapes.py on tests/resample_shapes.py's table."""
import numpy as np
import pytest

import resample_model as RM
from test_gpu_wide_fmt import _monotone_table, bits, conv, conv_u8, dev, noise, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def mods():
    from p25rx_amd import _lib
    from p25rx_amd.frontend import FrontEnd, Resampler
    return _lib, FrontEnd, Resampler


def rand_taps(rng, L, T):
    return (rng.standard_normal(L * T) * 0.1).astype(np.float32)


def cnoise(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def host(y, no, c=0):
    return y[c, :no].cpu().numpy().view(np.complex64)[..., 0]


# the ranges' ratio: one capture and its whole-stream model output, computed once and shared (never modified)
R_L, R_M, R_T, R_N = 12, 125, 84, 40003


@pytest.fixture(scope="module")
def stream():
    rng = np.random.default_rng(30)
    taps = rand_taps(rng, R_L, R_T)
    x = cnoise(rng, R_N)
    y = RM.resample(x, R_L, R_M, R_T, taps)
    y.setflags(write=False)
    x.setflags(write=False)
    return taps, x, y


# ---- 1: with L / M / T = 1 / 10 / 80 and SPEC 3.0's taps it is K0 --------------------------------------------------------------
def test_is_k0(O, mods):
    _lib, FE, RS = mods
    spec = O.load_spec()
    taps = np.array(spec["pre_taps"], dtype=np.float32)
    n = 7709
    fe = FE()
    rs = RS(fe, 1, 10, 80, taps)
    x = cnoise(np.random.default_rng(1), n)
    y, no = rs.resample_dev(dev(x))
    yk, nk = fe.predecim_dev(dev(x))
    ref = O.PreDecim().feed(x)
    assert no == nk == len(ref) == 770 == rs.n_out(0, n)
    assert same_bits(y[:, :no], yk[:, :no])
    assert np.array_equal(bits(host(y, no)), bits(ref))
    for fmt in ("u8", "s16"):
        xn = noise(fmt, np.random.default_rng(2), n)
        yn, nn = rs.resample_dev(dev(xn))
        yc, nc = rs.resample_dev(dev(conv(xn)))
        assert nn == nc == 770 and same_bits(yn[:, :nn], yc[:, :nc]), fmt
        assert np.array_equal(bits(host(yn, nn)), bits(O.PreDecim().feed(conv(xn)))), fmt


# ---- 2: model parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(12, 125, 84, 40003), (15, 128, 69, 33001), (3, 250, 667, 200003), (24, 25, 9, 4099),
                                   (2, 25, 100, 30011)], ids=lambda s: "%d_%d_%d" % s[:3])
def test_model_parity(mods, shape):
    """whole streams from position 0: the count, every output's bits, every phase in use.  Sizes: see the module's docstring (3840,
    3867, 2400, 3935 and 2400 outputs: at least two full workgroups and a partial one)."""
    _lib, FE, RS = mods
    L, M, T, n = shape
    rng = np.random.default_rng(20 + L)
    taps, x = rand_taps(rng, L, T), cnoise(rng, n)
    ref = RM.resample(x, L, M, T, taps)
    fe = FE()
    rs = RS(fe, L, M, T, taps)
    y, no = rs.resample_dev(dev(x))
    assert no == len(ref) == RM.n_resample(L, M, 0, n) == int(fe.L.p25fe_n_resample(L, M, 0, n)) and no >= 2400
    assert set(RM.phases(L, M, no).tolist()) == set(range(L))
    got = host(y, no)
    bad = np.flatnonzero((bits(got) != bits(ref)).reshape(no, 2).any(axis=1))
    assert bad.size == 0, (bad[:8], got[bad[:4]], ref[bad[:4]])


# ---- 3: ranges ----------------------------------------------------------------------------------------------------------------
def test_ranges(mods, stream):
    """Ranges in the middle of the capture.  d_iq has to be 16-byte aligned (two cf32 samples), so a range whose position is odd
    cannot sit at that offset of the capture's own buffer: `call` gives it a buffer of its own -- [junk | n_hist samples of history |
    the range] with the range on an even index -- and passes its position as abs_first; the junk in front of the history must not
    be read.  The positions are no multiple of M, of L or of the 16-byte vector, the lengths are odd.  One range runs in the capture's
    own buffer with abs_first == offset (even), and an odd offset there is refused (at the end)."""
    _lib, FE, RS = mods
    taps, x, y = stream
    L, M, T = R_L, R_M, R_T
    fe = FE()
    rs = RS(fe, L, M, T, taps)
    tx = dev(x)
    junk = cnoise(np.random.default_rng(31), 2) * 1000

    def call(a, n, n_hist):
        lead = (n_hist + 1) // 2 * 2
        buf = np.concatenate([junk[:lead - n_hist], x[a - n_hist:a + n]])
        g, no = rs.resample_dev(dev(buf), n_hist=n_hist, abs0=a, offset=lead)
        return host(g, no).copy()
    for a, n in ((5007, 3001), (12347, 20001), (127, 1)):
        assert a % M and a % L and a % 2
        first, cnt = a * L // M, RM.n_resample(L, M, a, n)
        for n_hist in (T - 1, T + 13, a):
            g = call(a, n, n_hist)
            assert len(g) == cnt and np.array_equal(bits(g), bits(y[first:first + cnt])), (a, n, n_hist)
        z = np.array(x[:a + n])
        for n_hist in (0, 40):                                       # less history than T - 1: what is missing reads as zero
            z[:a] = x[:a]
            z[:a - n_hist] = 0
            g = call(a, n, n_hist)
            assert len(g) == cnt and np.array_equal(bits(g), bits(RM.resample(z, L, M, T, taps)[first:first + cnt])), (a, n, n_hist)
    a, n = 5006, 3001                                                # in place: abs_first == offset
    first, cnt = a * L // M, RM.n_resample(L, M, a, n)
    for n_hist in (T - 1, T + 13, a):
        g, no = rs.resample_dev(tx[:a + n], n_hist=n_hist, abs0=a, offset=a)
        assert no == cnt and np.array_equal(bits(host(g, no)), bits(y[first:first + cnt])), n_hist
    # three consecutive ranges of odd lengths: the whole stream
    cuts = (0, 13339, 13339 + 11111, R_N)
    assert all((b - a) % 2 == 1 for a, b in zip(cuts, cuts[1:]))
    parts = [call(a, b - a, min(a, T - 1)) for a, b in zip(cuts, cuts[1:])]
    assert np.array_equal(bits(np.concatenate(parts)), bits(y))
    # a range shorter than M / L that owns no output: count 0, nothing written
    import torch
    a, n = 5012, 8                                                   # outputs sit at inputs 5010, 5020: none in [5012, 5020)
    assert RM.n_resample(L, M, a, n) == 0
    out = torch.full((1, 16, 2), -7.5, device="cuda")
    g, no = rs.resample_dev(tx[:a + n], n_hist=T - 1, abs0=a, offset=a, out=out)
    assert no == 0 and bool((out == -7.5).all())
    # a pointer off the 16-byte grid
    with pytest.raises(_lib.P25feError) as ei:
        rs.resample_dev(tx[:6000], n_hist=T - 1, abs0=5007, offset=5007)
    assert ei.value.status == _lib.ERR_ARG


# ---- 4: guards ----------------------------------------------------------------------------------------------------------------
def test_guards_and_three_channels(mods):
    """nothing is written from n_out on, nor in the padding between rows; three channels with strides larger than needed each equal
    their own single-channel run; out_stride < n_out is an argument error"""
    import torch
    _lib, FE, RS = mods
    L, M, T = R_L, R_M, R_T
    rng = np.random.default_rng(40)
    taps = rand_taps(rng, L, T)
    Cn, stride, n = 3, 9008, 8995
    x = np.stack([cnoise(rng, stride) for _ in range(Cn)])
    tx = dev(x)
    fe3, fe1 = FE(n_channels=Cn), FE()
    rs3, rs1 = RS(fe3, L, M, T, taps), RS(fe1, L, M, T, taps)
    cnt = RM.n_resample(L, M, 0, n)
    sentinel = -123456.75
    out = torch.full((Cn, cnt + 37, 2), sentinel, device="cuda")
    g, no = rs3.resample_dev(tx[:, :n], out=out)
    assert no == cnt and g.data_ptr() == out.data_ptr()
    assert bool((out[:, cnt:] == sentinel).all())
    for c in range(Cn):
        g1, n1 = rs1.resample_dev(tx[c, :n].contiguous())
        assert n1 == cnt and same_bits(out[c, :cnt], g1[0, :cnt]), c
        assert np.array_equal(bits(host(out, cnt, c)), bits(RM.resample(x[c, :n], L, M, T, taps))), c
    # a range with history and a position off the grid, three channels
    g, no = rs3.resample_dev(tx[:, :n], n_hist=96, abs0=1000 * M + 77, offset=96)
    for c in range(Cn):
        g1, n1 = rs1.resample_dev(tx[c, :n].contiguous(), n_hist=96, abs0=77, offset=96)
        assert n1 == no and same_bits(g[c, :no], g1[0, :no]), c
    small = torch.full((Cn, cnt - 1, 2), sentinel, device="cuda")
    with pytest.raises(_lib.P25feError) as ei:
        rs3.resample_dev(tx[:, :n], out=small)
    assert ei.value.status == _lib.ERR_ARG and bool((small == sentinel).all())


# ---- 5: formats ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "u8_lut", "s16"])
def test_formats(mods, kind):
    """u8 with the default affine table, u8 with a table that is not affine (looked up in LDS) and s16, the formats' extremes spliced
    in: bit for bit the cf32 call on the converted samples with the same n_hist / abs_first / offset"""
    _lib, FE, RS = mods
    L, M, T = 15, 128, 69
    rng = np.random.default_rng(50)
    taps = rand_taps(rng, L, T)
    n = 12003
    fmt = "s16" if kind == "s16" else "u8"
    table = _monotone_table() if kind == "u8_lut" else None
    fe = FE(u8_lut=table, specialize=_lib.SPECIALIZE_OFF) if table is not None else FE()
    rs = RS(fe, L, M, T, taps)
    x = noise(fmt, rng, n)
    cf = conv_u8(x, table) if fmt == "u8" else conv(x)
    tx, tc = dev(x), dev(cf)
    ref = RM.resample(cf, L, M, T, taps)
    for kw in (dict(), dict(n_hist=T - 1, abs0=2008, offset=2008), dict(n_hist=96, abs0=7 * M + 5, offset=1048),
               dict(n_hist=8, abs0=3, offset=8)):
        y, no = rs.resample_dev(tx, **kw)
        yc, nc = rs.resample_dev(tc, **kw)
        assert no == nc and no > 1000 and same_bits(y[:, :no], yc[:, :nc]), (kind, kw)
        if kw.get("abs0", 0) == kw.get("offset", 0) and kw.get("n_hist", 0) in (0, T - 1):
            first = kw.get("abs0", 0) * L // M
            assert np.array_equal(bits(host(y, no)), bits(ref[first:first + no])), (kind, kw)


# ---- 6: positions -------------------------------------------------------------------------------------------------------------
def test_large_positions(mods, stream):
    """abs_first = k M + r with k M just past 2^31, 2^32, 2^40 and 2^56: the bits and the count of position r (the grid is M);
    2^62 and beyond is P25FE_ERR_ARG"""
    _lib, FE, RS = mods
    taps, x, _ = stream
    L, M, T = R_L, R_M, R_T
    fe = FE()
    rs = RS(fe, L, M, T, taps)
    offset, n_hist = 1048, 96
    tx = dev(x[:offset + 6007])
    for r in (0, 1, 7, 77, 124):
        ys, ns = rs.resample_dev(tx, n_hist=n_hist, abs0=r, offset=offset)
        for two in (31, 32, 40, 56):
            kM = ((1 << two) // M + 1) * M
            y, no = rs.resample_dev(tx, n_hist=n_hist, abs0=kM + r, offset=offset)
            assert no == ns == RM.n_resample(L, M, kM + r, 6007) and no > 570, (two, r)
            assert same_bits(y[:, :no], ys[:, :ns]), (two, r)
    y, no = rs.resample_dev(tx, n_hist=n_hist, abs0=(1 << 62) - 1, offset=offset)
    assert no == RM.n_resample(L, M, (1 << 62) - 1, 6007)
    for P in (1 << 62, (1 << 64) - 1):
        with pytest.raises(_lib.P25feError) as ei:
            rs.resample_dev(tx, n_hist=n_hist, abs0=P, offset=offset)
        assert ei.value.status == _lib.ERR_ARG


# ---- 7: host streaming form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["cf32", "u8", "s16"])
def test_host_streaming(mods, stream, fmt):
    """one call = five chunks of uneven sizes = resample_dev; a cap too small is P25FE_ERR_CAPACITY and changes nothing; reset
    restarts at position 0; another format within a stream is P25FE_ERR_FORMAT"""
    import ctypes as C
    _lib, FE, RS = mods
    taps, xs, ys = stream
    L, M, T = R_L, R_M, R_T
    n = 20011
    if fmt == "cf32":
        x, cf, unit = np.array(xs[:n]), xs[:n], 1
        ref = ys[:RM.n_resample(L, M, 0, n)]
    else:
        x, unit = noise(fmt, np.random.default_rng(70), n), 2
        cf = conv(x)
        ref = RM.resample(cf, L, M, T, taps)
    fe = FE()
    rs = RS(fe, L, M, T, taps)
    one = rs.resample(x)
    assert np.array_equal(bits(one), bits(ref))
    yd, nd = rs.resample_dev(dev(x))
    assert nd == len(one) and np.array_equal(bits(host(yd, nd)), bits(one))
    # the stream goes on where the call left it: the next chunk continues at position n
    rs.reset()
    cuts = (0, 1, 50, 8007, 8010, n)                                 # 1, 49 (both shorter than the history), 7957, 3, 12001
    parts = [rs.resample(x[unit * a:unit * b]) for a, b in zip(cuts, cuts[1:])]
    assert len(parts[0]) == 0 and np.array_equal(bits(np.concatenate(parts)), bits(one))
    # capacity
    rs.reset()
    head = rs.resample(x[:unit * 9001])
    need = RM.n_resample(L, M, 9001, n - 9001)
    out = np.full(need, np.complex64(-3.25), dtype=np.complex64)
    no = C.c_size_t(0)
    tail = np.ascontiguousarray(x[unit * 9001:])
    rc = fe.L.p25fe_resample(rs.rs, tail.ctypes.data_as(C.c_void_p), {"cf32": 0, "u8": 1, "s16": 2}[fmt], n - 9001,
                             out.ctypes.data_as(C.c_void_p), need - 1, C.byref(no))
    assert rc == _lib.ERR_CAPACITY and no.value == need and (out == np.complex64(-3.25)).all()
    rest = rs.resample(tail)
    assert np.array_equal(bits(np.concatenate([head, rest])), bits(one))
    # another format in the same stream
    other = np.zeros(16, dtype=np.int16) if fmt != "s16" else np.zeros(16, dtype=np.uint8)
    with pytest.raises(_lib.P25feError) as ei:
        rs.resample(other)
    assert ei.value.status == _lib.ERR_FORMAT
    rs.reset()
    assert np.array_equal(bits(rs.resample(x[:unit * 5000])), bits(one[:RM.n_resample(L, M, 0, 5000)]))


# ---- 8: end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up,down,fs", [(125, 12, 2500000), (128, 15, 2048000), (25, 2, 3000000)])
def test_end_to_end(O, mods, up, down, fs):
    """a C4FM channel resampled to the tuner's rate, an interferer 300 kHz away added, the designed filter, the resampler, the
    receive chain: the oracle's dibits on the model's output, bit for bit, and the generator's symbols without an error"""
    from scipy import signal as sps
    from p25rx_amd import c4fm
    from p25rx_amd.frontend import parse_results
    _lib, FE, RS = mods
    iq, truth, _ = c4fm.synth(0.25, seed=12, snr_db=25.0)
    wide = sps.resample_poly(iq.astype(np.complex128), up, down)
    t = np.arange(len(wide)) / float(fs)
    wide = (wide + 0.8 * np.exp(2j * np.pi * 300e3 * t)).astype(np.complex64)
    L, M, T, taps = RS.design(fs)
    assert (L, M) == (down, up)
    x240 = RM.resample(wide, L, M, T, taps)
    ref = O.run_cf32(x240)
    k = min(len(ref), len(truth) - 24)
    assert k > 1100 and np.array_equal(ref[:k], truth[24:24 + k])
    fe = FE()
    rs = RS(fe, L, M, T, taps)
    y, no = rs.resample_dev(dev(wide))
    assert no == len(x240) and np.array_equal(bits(host(y, no)), bits(x240))
    dib, res = fe.run_dev(y[:, :no])
    got = dib[0, :int(parse_results(res)[0]["n_dibits"])].cpu().numpy()
    assert np.array_equal(got, ref)
    assert np.array_equal(got[:k], truth[24:24 + k])


@pytest.mark.parametrize("mode", ["u8", "s16"])
def test_replay_resamples(O, mods, tmp_path, mode):
    """p25fe_replay -r 2048000 u8|s16 (the resampler alone in front of the cf32 mode's path) on test_end_to_end's 2.048 Msps capture,
    one 32768-byte buffer's worth per call and the default batch: the oracle's dibits on the model's output for the converted
    capture, bit for bit.  The capture is scaled to the formats' range first: channel plus interferer reach 1.4."""
    import os
    import subprocess
    from scipy import signal as sps
    from p25rx_amd import c4fm
    _lib, FE, RS = mods
    up, down, fs = 128, 15, 2048000
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "p25fe_replay")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    iq, truth, _ = c4fm.synth(0.25, seed=12, snr_db=25.0)
    wide = sps.resample_poly(iq.astype(np.complex128), up, down)
    t = np.arange(len(wide)) / float(fs)
    wide = (0.5 * (wide + 0.8 * np.exp(2j * np.pi * 300e3 * t))).astype(np.complex64)
    raw = c4fm.to_u8(wide) if mode == "u8" else c4fm.to_s16(wide)
    L, M, T, taps = RS.design(fs)
    assert (L, M) == (down, up)
    ref = O.run_cf32(RM.resample(conv(raw), L, M, T, taps))
    k = min(len(ref), len(truth) - 24)
    assert k > 1100 and np.array_equal(ref[:k], truth[24:24 + k])
    src, out = tmp_path / ("cap." + mode), tmp_path / "dibits.out"
    raw.tofile(src)
    for batch in (["-b", "1"], []):
        r = subprocess.run([exe] + batch + ["-r", str(fs), mode, str(src), str(out)], capture_output=True, text=True, timeout=100)
        assert r.returncode == 0, r.stderr[-1000:]
        assert np.array_equal(np.fromfile(out, dtype=np.uint8), ref), batch


# ---- 9: lifetimes -------------------------------------------------------------------------------------------------------------
def test_destroy_after_the_handle(mods, stream):
    """A garbage collector may finalise the handle before the resampler made from it (both sit in one reference cycle as soon as a
    caught exception's traceback holds the frame): p25fe_resampler_destroy then must not read the handle -- nothing it does may
    fail or leave an error behind for the next call of the thread."""
    _lib, FE, RS = mods
    taps, x, y = stream
    for _ in range(3):
        fe = FE()
        rs = RS(fe, R_L, R_M, R_T, taps)
        fe.close()                                                   # the handle first
        junk = [FE() for _ in range(2)]                              # its memory is handed out again
        rs.close()
        del junk
        fe2 = FE()
        rs2 = RS(fe2, R_L, R_M, R_T, taps)
        g, no = rs2.resample_dev(dev(x[:4001]))
        assert no == RM.n_resample(R_L, R_M, 0, 4001) and np.array_equal(bits(host(g, no)), bits(y[:no]))
        assert np.array_equal(bits(rs2.resample(np.array(x[:4001]))), bits(y[:no]))
