"""AFC on the GPU (docs/SPEC.md 3.0e: k_tune_nco's ph0 and p25fe_afc_set_step; 3.0f: k_afc_measure), through the C ABI, bit for bit
against tests/afc_model.py.

Retune: a fresh object IS 3.0d; after p25fe_afc_set_step every range equals the model with the channel's new (step, ph0), the
history mixed with them too.  Shapes: 12/125 with T = 84 (a sub-tile is 180 outputs, a workgroup 720) and the short-table rate
24/25 with T = 9 (192 and 768): one partial sub-tile, more than RS_SUBS sub-tiles (two workgroups per channel), and no output.
Measure: a tile holds 180 (D 10, T 240), 255 (D 3, T 7) and 23 (D 64, T 512) products; the counts sit on both sides of a tile."""
import numpy as np
import pytest

import afc_model as AM
import resample_model as RM
import tune_model as TM
import tune_nco_model as NM
from test_gpu_tune import cnoise, host, rand_taps
from test_gpu_wide_fmt import bits, conv, dev, noise

pytestmark = pytest.mark.gpu

OFF_A, OFF_B = 232387521, -3527459
STEPS = (0, OFF_A, OFF_B)
MASK = (1 << 32) - 1


@pytest.fixture(scope="module")
def mods():
    from p25rx_amd import _lib
    from p25rx_amd.frontend import Afc, FrontEnd, Tuner
    return _lib, FrontEnd, Tuner, Afc


@pytest.fixture(scope="module")
def rot(mods):
    return mods[2].rotator(256)


# ---- retune -------------------------------------------------------------------------------------------------------------------
def model_range(rot, xs, n_hist, a0, L, M, T, taps, params):
    """xs = [n_hist samples of history | the range], a0 = the position of the range's first sample, params = [(step, ph0)] ->
    [K, count]: the model's stream starts on the output grid, at the multiple of M below the history, with zeros up to it"""
    s0 = (a0 - n_hist) // M * M
    pad = a0 - n_hist - s0
    z = np.concatenate([np.zeros(pad, dtype=np.complex64), xs])
    a_loc = pad + n_hist
    first, cnt = a_loc * L // M, RM.n_resample(L, M, a0, len(xs) - n_hist)
    assert cnt == RM.n_resample(L, M, a_loc, len(xs) - n_hist)
    return np.stack([RM.resample(AM.mix_nco(z, st, ph0, s0, *rot), L, M, T, taps)[first:first + cnt] for st, ph0 in params])


def check_rows(y, no, ref, what=None):
    assert no == ref.shape[1], (what, no, ref.shape)
    for k in range(ref.shape[0]):
        got = host(y, no, k)
        bad = np.flatnonzero((bits(got) != bits(ref[k])).reshape(no, 2).any(axis=1)) if no else np.zeros(0, dtype=np.int64)
        assert bad.size == 0, (what, k, bad[:8], got[bad[:4]], ref[k][bad[:4]])


@pytest.mark.parametrize("fmt", ["cf32", "s16", "u8"])
@pytest.mark.parametrize("ratio", [(12, 125, 84, 1000, 8400, 240), (24, 25, 9, 104, 880, 48)], ids=lambda r: "%d_%d" % r[:2])
def test_retune(mods, rot, ratio, fmt):
    """K = 3 at steps (0, 232387521, -3527459); range 1 = [P - n1, P) on a fresh object, p25fe_afc_set_step on every channel at
    abs_at = P (two calls on the last one: they compose; the second channel goes to step 0 and keeps a phase offset), then from P:
    more than RS_SUBS sub-tiles, one partial sub-tile, and a range that owns no output, every one into rows with guard bands.
    P = 5000, 2^32 + 77 and 2^40 + 3."""
    import torch
    _lib, FE, TN, _ = mods
    L, M, T, n1, n2, n_small = ratio
    K, hist, sentinel = len(STEPS), 96, -123456.75
    rng = np.random.default_rng(40 + L)
    taps = rand_taps(rng, L, T)
    raw = cnoise(rng, hist + n1 + n2) if fmt == "cf32" else noise(fmt, rng, hist + n1 + n2)
    x = raw if fmt == "cf32" else conv(raw)
    tx = dev(raw)
    fe = FE()
    for P in (5000, (1 << 32) + 77, (1 << 40) + 3):
        tn = TN.nco(fe, L, M, T, taps, STEPS)
        params = [(st, 0) for st in STEPS]
        assert [tn.get_step(k) for k in range(K)] == params
        # a fresh object is 3.0d (every ph0 is 0)
        y, no = tn.tune_dev(tx[:hist + n1], n_hist=hist, abs0=P - n1, offset=hist)
        ref = model_range(rot, x[:hist + n1], hist, P - n1, L, M, T, taps, params)
        check_rows(y, no, ref, ("fresh", P))
        # retune every channel at P
        new = (1234567, 0, OFF_B + 5000)
        for k in (0, 1):
            tn.set_step(k, new[k], P)
            params[k] = AM.set_step(*params[k], new[k], P)
        tn.set_step(2, 77777777, P - 13)                              # two calls before one launch compose
        tn.set_step(2, new[2], P)
        params[2] = AM.set_step(*AM.set_step(*params[2], 77777777, P - 13), new[2], P)
        assert [tn.get_step(k) for k in range(K)] == params
        assert params[1][0] == 0 and params[1][1] != 0 and all(p[1] != 0 for p in params)
        o2 = hist + n1                                                # range 2 starts here: a multiple of 8 samples
        assert o2 % 8 == 0
        n_none = next(n for n in (3, 2, 1, 0) if RM.n_resample(L, M, P, n) == 0)
        for what, n in (("two workgroups", n2), ("partial sub-tile", n_small), ("no output", n_none)):
            cnt = RM.n_resample(L, M, P, n)
            if what == "two workgroups":
                tile = min((64 - 64 % L) * 4, 1 + (2040 - T) * L // M)
                tile = tile if tile < 64 - 64 % L else tile // (64 - 64 % L) * (64 - 64 % L)
                assert 4 * tile < cnt <= 8 * tile, (cnt, tile)
            elif what == "partial sub-tile":
                assert 0 < cnt < 60
            else:
                assert cnt == 0
            out = torch.full((K, cnt + 38, 2), sentinel, device="cuda")
            g, no = tn.tune_dev(tx[:o2 + n], n_hist=T - 1, abs0=P, offset=o2, out=out)
            assert no == cnt and bool((out[:, cnt:] == sentinel).all()), (what, P)
            if cnt:
                ref = model_range(rot, x[o2 - (T - 1):o2 + n], T - 1, P, L, M, T, taps, params)
                check_rows(out, cnt, ref, (what, P))
        # back to the first steps at the same index: the offsets return to zero and the object is 3.0d again
        tn.set_step(0, STEPS[0], P)
        tn.set_step(1, STEPS[1], P)
        tn.set_step(2, 77777777, P)
        tn.set_step(2, STEPS[2], P - 13)
        assert [tn.get_step(k) for k in range(K)] == [(st, 0) for st in STEPS]
        g, no = tn.tune_dev(tx[:o2 + n_small], n_hist=T - 1, abs0=P, offset=o2)
        check_rows(g, no, model_range(rot, x[o2 - (T - 1):o2 + n_small], T - 1, P, L, M, T, taps, [(st, 0) for st in STEPS]), ("back", P))
        tn.close()


def test_retune_one_channel_of_several(mods, rot):
    """p25fe_afc_set_step on ONE channel leaves the others as p25fe_nco_create made them, ph0 = 0 on the device as on the host.
    24/25 with T = 9, K = 3 at steps (232387521, -3527459, 0), cf32, P = 5000 and 2^32 + 77: range 1 = [P - 104, P) on a fresh
    object, set_step(1, 1234567, P) alone, range 2 = 880 samples from P with n_hist = T - 1 into rows with guard bands.  Channel 1
    equals the model with its new (step, ph0), channels 0 and 2 the model with (step, 0), channel 2 the resampler's output of the
    same range, all bit for bit, and get_step says the same.  Then the host form: p25fe_tune with K = 2, p25fe_afc_set_step with a
    null stream on channel 0, channel 1 (step 0) untouched."""
    import torch
    from p25rx_amd.frontend import Resampler
    _lib, FE, TN, _ = mods
    L, M, T, n1, n2 = 24, 25, 9, 104, 880
    steps, hist, sentinel = (OFF_A, OFF_B, 0), 96, -123456.75
    K, o2 = len(steps), hist + n1
    rng = np.random.default_rng(47)
    taps, x = rand_taps(rng, L, T), cnoise(rng, o2 + n2)
    tx = dev(x)
    fe = FE()
    rs = Resampler(fe, L, M, T, taps)
    for P in (5000, (1 << 32) + 77):
        tn = TN.nco(fe, L, M, T, taps, steps)
        params = [(st, 0) for st in steps]
        y, no = tn.tune_dev(tx[:o2], n_hist=hist, abs0=P - n1, offset=hist)
        check_rows(y, no, model_range(rot, x[:o2], hist, P - n1, L, M, T, taps, params), ("fresh", P))
        tn.set_step(1, 1234567, P)
        params[1] = AM.set_step(*params[1], 1234567, P)
        assert params[1][1] != 0 and [tn.get_step(k) for k in range(K)] == params
        cnt = RM.n_resample(L, M, P, n2)
        out = torch.full((K, cnt + 38, 2), sentinel, device="cuda")
        g, no = tn.tune_dev(tx, n_hist=T - 1, abs0=P, offset=o2, out=out)
        assert no == cnt and cnt > 800 and bool((out[:, cnt:] == sentinel).all()), P
        check_rows(out, cnt, model_range(rot, x[o2 - (T - 1):], T - 1, P, L, M, T, taps, params), ("one retuned", P))
        r, nr = rs.resample_dev(tx, n_hist=T - 1, abs0=P, offset=o2)
        assert nr == cnt and np.array_equal(bits(host(out, cnt, 2)), bits(host(r, nr, 0))), P
        tn.close()
    # the host form, from position 0: the chunks are [0, n1) and [n1, n1 + n2)
    xs = x[:n1 + n2]
    tn = TN.nco(fe, L, M, T, taps, [OFF_A, 0])
    a = tn.tune(xs[:n1])
    assert np.array_equal(bits(a), bits(model_range(rot, xs[:n1], 0, 0, L, M, T, taps, [(OFF_A, 0), (0, 0)])))
    assert fe.L.p25fe_afc_set_step(tn.tn, 0, 1234567, n1, None) == _lib.OK
    params = [AM.set_step(OFF_A, 0, 1234567, n1), (0, 0)]
    assert params[0][1] != 0 and [tn.get_step(k) for k in range(2)] == params
    b = tn.tune(xs[n1:])
    assert b.shape[1] == RM.n_resample(L, M, n1, n2)
    assert np.array_equal(bits(b), bits(model_range(rot, xs[n1 - (T - 1):], T - 1, n1, L, M, T, taps, params)))
    rs.resample(xs[:n1])
    assert np.array_equal(bits(b[1]), bits(rs.resample(xs[n1:])))


def test_retune_host_streaming_and_refusals(mods, rot):
    """p25fe_tune after p25fe_afc_set_step with a null stream (the handle's): the chunk equals the model with the new numbers;
    p25fe_tuner_reset leaves steps and offsets alone; a rational tuner, a channel outside the range and a refused position are
    P25FE_ERR_ARG and change nothing"""
    import ctypes as C
    _lib, FE, TN, _ = mods
    L, M, T = 12, 125, 84
    rng = np.random.default_rng(45)
    taps, x = rand_taps(rng, L, T), cnoise(rng, 6000)
    fe = FE()
    tn = TN.nco(fe, L, M, T, taps, [OFF_A])
    a = tn.tune(x[:2500])
    assert np.array_equal(bits(a), bits(model_range(rot, x[:2500], 0, 0, L, M, T, taps, [(OFF_A, 0)])))
    assert fe.L.p25fe_afc_set_step(tn.tn, 0, OFF_A + 9999, 2500, None) == _lib.OK
    par = AM.set_step(OFF_A, 0, OFF_A + 9999, 2500)
    assert tn.get_step(0) == par and par[1] != 0
    b = tn.tune(x[2500:])
    assert np.array_equal(bits(b), bits(model_range(rot, x[2500 - (T - 1):], T - 1, 2500, L, M, T, taps, [par])))
    tn.reset()
    assert tn.get_step(0) == par
    c = tn.tune(x[:2500])
    assert np.array_equal(bits(c), bits(model_range(rot, x[:2500], 0, 0, L, M, T, taps, [par])))
    for k, at in ((1, 0), (-1, 0), (0, 1 << 62), (0, (1 << 64) - 1)):
        assert fe.L.p25fe_afc_set_step(tn.tn, k, 5, at, None) == _lib.ERR_ARG
    assert tn.get_step(0) == par
    st, ph = C.c_int32(0), C.c_uint32(0)
    assert fe.L.p25fe_afc_get_step(tn.tn, 1, C.byref(st), C.byref(ph)) == _lib.ERR_ARG
    assert fe.L.p25fe_afc_get_step(tn.tn, 0, None, C.byref(ph)) == _lib.ERR_ARG
    rat = TN(fe, L, M, T, taps, [(11, 200)])
    assert fe.L.p25fe_afc_set_step(rat.tn, 0, 5, 0, None) == _lib.ERR_ARG
    assert fe.L.p25fe_afc_get_step(rat.tn, 0, C.byref(st), C.byref(ph)) == _lib.ERR_ARG


# ---- measure ------------------------------------------------------------------------------------------------------------------
SHAPES = {(10, 240): 180, (3, 7): 255, (64, 512): 23}               # (D, T) -> products per tile


def _rec(t):
    return tuple(int(v) for v in t)


class Stream:
    """K rows of unit noise through a low-pass prefilter, and the model's products of every row at three shifts (computed once)"""

    def __init__(self, Afc, D, T, K):
        self.D, self.T, self.K, self.P = D, T, K, SHAPES[(D, T)]
        rng = np.random.default_rng(1000 * D + T + K)
        self.g = Afc.design(D, T, 240000.0 / D / 8.0)
        self.n = (2 * self.P + 5) * D + 3
        self.x = np.stack([cnoise(rng, self.n) for _ in range(K)])
        self.raw = [AM.raw_products(self.x[k], D, T, self.g) for k in range(K)]
        self.prod = {sh: [AM.quantise(r, sh) for r in self.raw] for sh in (0, 24, 40)}
        self.x.setflags(write=False)

    def records(self, first, count, shift=24):
        return [AM.record(self.prod[shift][k], first, count) for k in range(self.K)]


_STREAMS = {}


@pytest.fixture(params=[(D, T, K) for (D, T) in SHAPES for K in (1, 3)], ids=lambda p: "D%d_T%d_K%d" % p)
def S(request, mods):
    if request.param not in _STREAMS:
        _STREAMS[request.param] = Stream(mods[3], *request.param)
    return _STREAMS[request.param]


def guarded(K, init=None):
    """K records between two guard records on the device"""
    import torch
    buf = torch.full((K + 2, 32), 0x5a, dtype=torch.uint8, device="cuda")
    buf[1:K + 1] = 0
    if init is not None:
        buf[1:K + 1] = torch.from_numpy(np.frombuffer(init.tobytes(), dtype=np.uint8).reshape(K, 32).copy()).cuda()
    return buf, buf[1:K + 1]


def read(mods, buf, K):
    assert bool((buf[0] == 0x5a).all()) and bool((buf[K + 1] == 0x5a).all()), "guard records touched"
    r = mods[3].records(buf[1:K + 1])
    return [_rec(r[k]) for k in range(K)]


def test_measure_counts(mods, S):
    """decimated counts 0, 1, exactly one tile, one tile + 1 and three workgroups, from position 0 with no history; shifts 0, 24
    and 40 (at 40 most products clamp)"""
    _lib, FE, TN, Afc = mods
    D, T, K, P = S.D, S.T, S.K, S.P
    fe = FE()
    afc = Afc(fe, K, D, T, taps=S.g)
    tx = dev(S.x)
    for c in (0, 1, P, P + 1, 2 * P + 5):
        n = c * D + (D - 1 if c == 0 else 0)
        assert RM.n_resample(1, D, 0, n) == c
        for shift in (0, 24, 40):
            buf, acc = guarded(K)
            afc.measure(tx, n=n, shift=shift, acc=acc)
            assert read(mods, buf, K) == S.records(0, c, shift), (c, shift)
    assert any(abs(int(v)) == 2147483520 for v in S.prod[40][0][2]) and not any(abs(int(v)) >= 2147483520 for v in S.prod[24][0][2])


def test_measure_splits_and_history(mods, S):
    """a stream split at odd places with n_hist = T - 1 + D sums to the whole-range record exactly, each part equals the model's
    part; n_hist = 0 in the middle of the stream equals the model of the zero-extended stream"""
    _lib, FE, TN, Afc = mods
    D, T, K, P = S.D, S.T, S.K, S.P
    fe = FE()
    afc = Afc(fe, K, D, T, taps=S.g)
    tx = dev(S.x)
    keep = T - 1 + D
    cuts = (0, 7, 7 + D * P + 3, 7 + D * P + 3 + 1, S.n - D - 1, S.n)
    buf, acc = guarded(K)
    for a, b in zip(cuts, cuts[1:]):
        part_buf, part = guarded(K)
        for target in (acc, part):
            afc.measure(tx, n_hist=min(a, keep), abs0=a, offset=a, n=b - a, acc=target)
        first, cnt = a // D, b // D - a // D
        assert read(mods, part_buf, K) == S.records(first, cnt), (a, b)
    assert read(mods, buf, K) == S.records(0, S.n // D)
    a = 7 + D * P + 3
    z = np.array(S.x)
    z[:, :a] = 0
    buf, acc = guarded(K)
    afc.measure(tx, n_hist=0, abs0=a, offset=a, acc=acc)
    want = [AM.record(AM.products(z[k], D, T, S.g, 24), a // D, S.n // D - a // D) for k in range(K)]
    assert read(mods, buf, K) == want and want != S.records(a // D, S.n // D - a // D)


def test_measure_positions(mods, S):
    """abs_first matters modulo D: 2^32 + 7 is position (2^32 + 7) mod D; 2^62 is refused"""
    _lib, FE, TN, Afc = mods
    D, T, K = S.D, S.T, S.K
    fe = FE()
    afc = Afc(fe, K, D, T, taps=S.g)
    tx = dev(S.x)
    pos = (1 << 32) + 7
    r = pos % D
    assert r != 0
    z = np.concatenate([np.zeros((K, r), dtype=np.complex64), S.x], axis=1)
    cnt = RM.n_resample(1, D, pos, S.n)
    want = [AM.record(AM.products(z[k], D, T, S.g, 24), 0, cnt) for k in range(K)]
    assert cnt == (r + S.n) // D and want != S.records(0, cnt)
    buf, acc = guarded(K)
    afc.measure(tx, abs0=pos, acc=acc)
    assert read(mods, buf, K) == want
    with pytest.raises(_lib.P25feError) as ei:
        afc.measure(tx, abs0=1 << 62, acc=acc)
    assert ei.value.status == _lib.ERR_ARG
    for shift in (-1, 41):
        with pytest.raises(_lib.P25feError) as ei:
            afc.measure(tx, shift=shift, acc=acc)
        assert ei.value.status == _lib.ERR_ARG
    assert read(mods, buf, K) == want


def test_measure_extremes(mods, S):
    """a row of magnitude 1e6 (Q clamps at shift 24), a row with NaN and +-Inf samples (NaN -> 0, Inf clamps), and accumulation
    onto re = pow = 2^63 - 5, which wraps"""
    _lib, FE, TN, Afc = mods
    D, T, K = S.D, S.T, S.K
    fe = FE()
    afc = Afc(fe, K, D, T, taps=S.g)
    big = (np.array(S.x) * np.float32(1e6)).astype(np.complex64)
    odd = np.array(S.x)
    odd[:, 5 * D] = np.nan
    odd[:, 17 * D + 1] = complex(np.inf, 1.0)
    odd[:, 31 * D + 2] = complex(2.0, -np.inf)
    odd[:, -3] = complex(np.nan, np.inf)
    for name, rows in (("1e6", big), ("nan inf", odd)):
        prods = [AM.products(rows[k], D, T, S.g, 24) for k in range(K)]
        want = [AM.record(p) for p in prods]
        if name == "1e6":
            assert all(np.count_nonzero(np.abs(p[2]) == 2147483520) > len(p[2]) // 2 for p in prods)
        buf, acc = guarded(K)
        afc.measure(dev(rows), acc=acc)
        assert read(mods, buf, K) == want, name
    whole = S.records(0, S.n // D)
    assert all(w[0] > 5 and w[2] > 5 for w in whole)                 # low-passed noise: the lag-1 product's real part is positive
    init = np.zeros(K, dtype=_lib.AFC_ACC_DTYPE)
    init["re"], init["pow"], init["im"], init["n"] = (1 << 63) - 5, (1 << 63) - 5, -77, (1 << 64) - 2
    buf, acc = guarded(K, init)
    afc.measure(dev(S.x), acc=acc)
    want = [(AM.wrap64((1 << 63) - 5 + w[0]), w[1] - 77, AM.wrap64((1 << 63) - 5 + w[2]), ((1 << 64) - 2 + w[3]) % (1 << 64)) for w in whole]
    assert all(w[0] < 0 and w[2] < 0 for w in want)
    assert read(mods, buf, K) == want


def test_measure_refuses_bad_pointers(mods):
    """a misaligned row pointer or record pointer and a null pointer are P25FE_ERR_ARG and write nothing"""
    import ctypes as C
    import torch
    _lib, FE, TN, Afc = mods
    fe = FE()
    afc = Afc(fe, 1, 3, 7, taps=Afc.design(3, 7, 10000.0))
    rows = torch.zeros((1, 64, 2), device="cuda")
    buf, acc = guarded(1)
    f = fe.L.p25fe_afc_measure_dev
    for rp, ap in ((rows.data_ptr() + 4, acc.data_ptr()), (rows.data_ptr(), acc.data_ptr() + 4), (0, acc.data_ptr()), (rows.data_ptr(), 0)):
        assert f(afc.afc, C.c_void_p(rp), 64, 0, 60, 0, 24, C.c_void_p(ap), None) == _lib.ERR_ARG
    assert read(mods, buf, 1) == [(0, 0, 0, 0)]


# ---- end to end ---------------------------------------------------------------------------------------------------------------
E_FS, E_OFFSETS = 2500000, (-412500 + 1871.3, 137500 - 2210.7, 150000 - 2411.6, 733.1)


@pytest.fixture(scope="module")
def site():
    wide, truths = TM.site_capture(E_FS, 125, 12, E_OFFSETS)
    wide.setflags(write=False)
    return wide, truths


def test_end_to_end(mods, rot, site):
    """the site capture through Tuner.nco at the RASTER frequencies: the rows decode nothing.  Afc.measure over the first 50 ms
    (the model's record bit for bit), set_step by the estimate at sample 125000, the rest of the capture through the retuned object
    and a four-channel handle's receive chain: every row locks on the frame sync inside the rest and decodes the generator's symbols
    from there to the end without an error"""
    from p25rx_amd.frontend import parse_results
    _lib, FE, TN, Afc = mods
    wide, truths = site
    raster = [int(round(o / 12500.0)) * 12500 for o in E_OFFSETS]
    L, M, T, taps, steps = TN.design_nco(E_FS, raster)
    cut = 125000
    fe1, fe4 = FE(), FE(n_channels=4)
    tn = TN.nco(fe1, L, M, T, taps, steps)
    tw = dev(wide)
    y, no = tn.tune_dev(tw)
    dib, res = fe4.run_dev(y[:, :no])
    assert [int(r["n_dibits"]) for r in parse_results(res)] == [0, 0, 0, 0]
    D, Tg, fc = Afc.DEFAULT
    afc = Afc(fe1, 4)
    head, nh = tn.tune_dev(tw[:cut])
    assert nh == 12000
    rec = Afc.records(afc.measure(head, n=nh))
    g = Afc.design(D, Tg, fc)
    for k in range(4):
        row = NM.tune_nco(wide[:cut], L, M, T, taps, steps[k], *rot)
        assert _rec(rec[k]) == AM.measure(row, D, Tg, g, 24), k
        hz, coh = Afc.hz(rec[k], D)
        print("offset %.1f: estimate %.1f Hz, true %.1f, coherence %.3f" % (E_OFFSETS[k], hz, E_OFFSETS[k] - raster[k], coh))
        assert abs(hz - (E_OFFSETS[k] - raster[k])) <= 150.0
        tn.set_step(k, steps[k] + TN.nco_step(E_FS, hz), cut)
    y2, n2 = tn.tune_dev(tw, n_hist=T - 1, abs0=cut, offset=cut)
    assert n2 == no - nh
    dib, res = fe4.run_dev(y2[:, :n2])
    for k in range(4):
        got = dib[k, :int(parse_results(res)[k]["n_dibits"])].cpu().numpy()
        kk = min(len(got), len(truths[k]) - 888)
        assert kk >= 290 and np.array_equal(got[:kk], truths[k][888:888 + kk]), (k, kk)


def test_replay_measures_and_corrects(site, tmp_path):
    """p25fe_replay -r 2500000 -F 137500 -a 50: tuned at the raster beside the capture's second source it measures 50 ms, retunes
    once and decodes from the next frame sync on; the estimate is in the JSON events; without -a it finds no frame; -a without -F
    is a usage error"""
    import json
    import os
    import subprocess
    wide, truths = site
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "p25fe_replay")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    src, out, out2, js = tmp_path / "cap.cf32", tmp_path / "dib.out", tmp_path / "dib2.out", tmp_path / "ev.jsonl"
    np.asarray(wide).tofile(src)
    r = subprocess.run([exe, "-j", str(js), "-r", str(E_FS), "-F", "137500", "-a", "50", "cf32", str(src), str(out)],
                       capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stderr[-1000:]
    got = np.fromfile(out, dtype=np.uint8)
    kk = min(len(got), len(truths[1]) - 888)
    assert kk >= 290 and np.array_equal(got[:kk], truths[1][888:888 + kk])
    ev = [json.loads(line) for line in open(js) if '"afc"' in line]
    assert len(ev) == 1 and ev[0]["event"] == "afc" and ev[0]["at"] == 125000 and ev[0]["products"] == 1200
    assert abs(ev[0]["hz"] - (-2210.7)) <= 150.0
    r = subprocess.run([exe, "-r", str(E_FS), "-F", "137500", "cf32", str(src), str(out2)], capture_output=True, text=True, timeout=100)
    assert r.returncode == 0 and len(np.fromfile(out2, dtype=np.uint8)) == 0, r.stderr[-1000:]
    r = subprocess.run([exe, "-r", str(E_FS), "-f", "137500", "-a", "50", "cf32", str(src), str(out2)], capture_output=True, text=True)
    assert r.returncode != 0 and "usage" in r.stderr
