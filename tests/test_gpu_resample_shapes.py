"""resample_body (k_resample, k_tune, k_tune_nco, k_tune_cuts) at every launch plan the shape limits of docs/SPEC.md 3.0b admit: the
designed rates the other files do not run and the corners of the limits (tests/resample_shapes.py's table; what it covers is
asserted on the CPU by tests/test_resample_shapes_model.py).  Every comparison is on bits: no tolerance anywhere in this file.

Per shape: random ASYMMETRIC taps and random input, seeded by the shape; size_for's n owns 9 tile + 3 outputs from position 0, which
are two full workgroups, one more full sub-tile and a partial one of 3 -- at a tile of 1 that is 12 outputs on three workgroups, and
that is the edge.  The models' rows of a shape are computed once (data()) and never modified.

Wall time of the whole file on the MI355X: docs/MEASUREMENTS.md, "Resampler and tuners, every launch plan"."""
import ctypes as C

import numpy as np
import pytest

import afc_model as AM
import resample_model as RM
import tune_cuts_model as CM
import tune_model as TM
from resample_shapes import RS_SUBS, SHAPES, outputs_for, plan, shape_id, size_for
from test_gpu_resample import cnoise, rand_taps
from test_gpu_tune import host
from test_gpu_tune_cuts import OFF_A, POISON, check_cuts, lead_of, len_for, reference_tuner, rows_of
from test_gpu_tune_nco import check_rows
from test_gpu_wide_fmt import _monotone_table, bits, conv, conv_u8, dev, noise, same_bits

pytestmark = pytest.mark.gpu

FREQS = ((0, 1), (11, 200), (-825, 4096))                            # the centre, a rotator in LDS, a gathered one
PAIRS = ((0, 0), (0x7fffffff, 0), (OFF_A, 0x9abcdef1), (-4507, 0))   # (step, ph0): no product, the largest step, off every raster, small
STREAMED = ((1, 2, 1), (1, 128, 1024), (32, 33, 128), (13, 1024, 315))
CHUNKS = (1, 500, 1023, 1024, 3000, 0, 7)                            # then the rest
N_STREAMED = sum(CHUNKS) + 1002
JUNK = {np.dtype(np.complex64): 1000 + 1000j, np.dtype(np.uint8): 255, np.dtype(np.int16): 32767}
shapes = pytest.mark.parametrize("shape", SHAPES, ids=shape_id)


@pytest.fixture(scope="module")
def mods():
    from p25rx_amd import _lib
    from p25rx_amd.frontend import Cuts, FrontEnd, Resampler, Tuner
    return _lib, FrontEnd, Resampler, Tuner, Cuts


@pytest.fixture(scope="module")
def fe(mods):
    return mods[1]()


@pytest.fixture(scope="module")
def fe_lut(mods):
    return mods[1](u8_lut=_monotone_table(), specialize=mods[0].SPECIALIZE_OFF)


@pytest.fixture(scope="module")
def rots(mods):
    """den -> (C, S): the library's getter defines the tables"""
    return {den: mods[3].rotator(den) for den in (200, 4096, 256)}


_DATA, _ROWS = {}, {}


def data(shape):
    """(taps, x, y, n, a, ln) of a shape: the capture, its whole-stream model output, size_for's n, and the range [a, a + ln) of the
    range tests -- a about a third into the capture (behind the first T - 1 samples at every shape), odd, no multiple of M; ln odd.
    The shapes that are streamed have a longer capture, of which the others use the first n samples."""
    if shape not in _DATA:
        L, M, T = shape
        rng = np.random.default_rng(100000 * L + 100 * M + T)
        n = size_for(L, M, T)
        taps, x = rand_taps(rng, L, T), cnoise(rng, max(n, N_STREAMED) if shape in STREAMED else n)
        y = RM.resample(x, L, M, T, taps)
        a = max(n // 3, T + 8) | 1
        while a % M == 0:
            a += 2
        ln = (n // 2) | 1
        assert a % 2 and a % M and a % 8 not in (0, 4) and ln % 2 and a >= T - 1 and a + ln <= n
        for v in (taps, x, y):
            v.setflags(write=False)
        _DATA[shape] = (taps, x, y, n, a, ln)
    return _DATA[shape]


def rows(shape, kind, rots):
    """the model's rows of the whole capture from position 0: kind "rational" (FREQS) or "nco" (PAIRS)"""
    if (shape, kind) not in _ROWS:
        L, M, T = shape
        taps, x = data(shape)[:2]
        if kind == "rational":
            r = np.stack([TM.tune(x, L, M, T, taps, num, den, *rots.get(den, (None, None))) for num, den in FREQS])
        else:
            r = np.stack([AM.tune(x, L, M, T, taps, st, ph, *rots[256]) for st, ph in PAIRS])
        r.setflags(write=False)
        _ROWS[(shape, kind)] = r
    return _ROWS[(shape, kind)]


def framed(x, a, ln, n_hist, lead):
    """[junk | n_hist samples of history | the range [a, a + ln)] of a capture in any format, the range at index `lead` -- a buffer of
    its own, as tests/test_gpu_resample.py::test_ranges::call builds it: the junk in front of the history must not be read as data"""
    unit = 1 if x.dtype == np.complex64 else 2
    assert lead >= n_hist and a >= n_hist
    junk = np.full(unit * (lead - n_hist), JUNK[x.dtype], dtype=x.dtype)
    return np.concatenate([junk, x[unit * (a - n_hist):unit * (a + ln)]])


def first_of(L, M, a):
    return a * L // M


# ---- a: the resampler, a whole stream from position 0 -----------------------------------------------------------------------------------
@shapes
def test_whole_stream(mods, fe, shape):
    _lib, FE, RS, TN, CT = mods
    L, M, T = shape
    taps, x, y, n, _a, _ln = data(shape)
    rs = RS(fe, L, M, T, taps)
    g, no = rs.resample_dev(dev(x[:n]))
    assert no == outputs_for(L, M, T) == RM.n_resample(L, M, 0, n) == int(fe.L.p25fe_n_resample(L, M, 0, n))
    check_rows(g, no, y[None, :no], shape)


# ---- b: the resampler, a range in the middle --------------------------------------------------------------------------------------------
@shapes
def test_a_range(mods, fe, shape):
    """with T - 1 samples of history the slice of the whole stream's output, with none the model of the stream zeroed before a (at
    T = 1 the two coincide); the output goes to a poisoned buffer with a stride larger than the count, and nothing outside
    [0, cnt) changes"""
    import torch
    _lib, FE, RS, TN, CT = mods
    L, M, T = shape
    taps, x, y, n, a, ln = data(shape)
    rs = RS(fe, L, M, T, taps)
    first, cnt = first_of(L, M, a), RM.n_resample(L, M, a, ln)
    z = np.array(x[:a + ln])
    z[:a] = 0
    zeroed = RM.resample(z, L, M, T, taps)[first:first + cnt]
    if T == 1:
        assert np.array_equal(bits(zeroed), bits(y[first:first + cnt]))
    for n_hist, want in ((T - 1, y[first:first + cnt]), (0, zeroed)):
        lead = lead_of(T) if n_hist else 0
        out = torch.full((1, cnt + 37, 2), POISON, device="cuda")
        g, no = rs.resample_dev(dev(framed(x, a, ln, n_hist, lead)), n_hist=n_hist, abs0=a, offset=lead, out=out)
        assert no == cnt > 0 and g.data_ptr() == out.data_ptr()
        check_rows(out, cnt, want[None], (shape, n_hist))
        assert bool((out[:, cnt:] == POISON).all()), (shape, n_hist)


# ---- c: formats -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["s16", "u8", "u8_lut"])
@shapes
def test_formats(mods, fe, fe_lut, shape, kind):
    """s16, u8 with the default affine table and u8 with a table that is not affine (looked up in LDS), the formats' extremes spliced
    in, at the cf32 cases' n: bit for bit the cf32 run of the converted samples, and the model of them, from position 0 and from
    the odd a of the range test with T - 1 samples of history.  `lead` is a multiple of 8, so the range starts on a 16-byte boundary
    in every format and its position a alone sets the loader's alignment case."""
    _lib, FE, RS, TN, CT = mods
    L, M, T = shape
    taps, _x, _y, n, a, ln = data(shape)
    fmt = "s16" if kind == "s16" else "u8"
    table = _monotone_table() if kind == "u8_lut" else None
    f = fe_lut if kind == "u8_lut" else fe
    rs = RS(f, L, M, T, taps)
    raw = noise(fmt, np.random.default_rng(7 * L + M + T + len(kind)), n)
    cf = conv_u8(raw, table) if fmt == "u8" else conv(raw)
    ref = RM.resample(cf, L, M, T, taps)
    g, no = rs.resample_dev(dev(raw))
    gc, nc = rs.resample_dev(dev(cf))
    assert no == nc == outputs_for(L, M, T) and same_bits(g[:, :no], gc[:, :nc]), (shape, kind)
    check_rows(g, no, ref[None], (shape, kind))
    lead = lead_of(T)
    fr = framed(raw, a, ln, T - 1, lead)
    frc = conv_u8(fr, table) if fmt == "u8" else conv(fr)
    kw = dict(n_hist=T - 1, abs0=a, offset=lead)
    g, no = rs.resample_dev(dev(fr), **kw)
    gc, nc = rs.resample_dev(dev(frc), **kw)
    first, cnt = first_of(L, M, a), RM.n_resample(L, M, a, ln)
    assert no == nc == cnt and same_bits(g[:, :no], gc[:, :nc]), (shape, kind, a)
    check_rows(g, no, ref[None, first:first + cnt], (shape, kind, a))


# ---- d: the rational tuner --------------------------------------------------------------------------------------------------------------
@shapes
def test_rational_tuner(mods, fe, rots, shape):
    _lib, FE, RS, TN, CT = mods
    L, M, T = shape
    taps, x, _y, n, a, ln = data(shape)
    ref = rows(shape, "rational", rots)
    tn = TN(fe, L, M, T, taps, FREQS)
    g, no = tn.tune_dev(dev(x[:n]))
    assert no == outputs_for(L, M, T)
    check_rows(g, no, ref[:, :no], shape)
    lead = lead_of(T)
    first, cnt = first_of(L, M, a), RM.n_resample(L, M, a, ln)
    g, no = tn.tune_dev(dev(framed(x, a, ln, T - 1, lead)), n_hist=T - 1, abs0=a, offset=lead)
    check_rows(g, no, ref[:, first:first + cnt], (shape, a))


# ---- e: the NCO tuner -------------------------------------------------------------------------------------------------------------------
@shapes
def test_nco_tuner(mods, fe, rots, shape):
    """the whole stream from position 0 against tests/afc_model.py; the same samples as ONE stream that straddles 2^32 -- it starts
    at an odd position n / 2 below 2^32 with no history -- against tests/tune_cuts_model.py's row at a position"""
    _lib, FE, RS, TN, CT = mods
    L, M, T = shape
    taps, x, _y, n, _a, _ln = data(shape)
    ref = rows(shape, "nco", rots)
    tn = reference_tuner(TN, fe, L, M, T, taps, PAIRS)
    tx = dev(x[:n])
    g, no = tn.tune_dev(tx)
    assert no == outputs_for(L, M, T)
    check_rows(g, no, ref[:, :no], shape)
    a0 = ((1 << 32) - n // 2) | 1
    assert a0 < (1 << 32) < a0 + n
    want = np.stack([CM.cut_row(x[:n], a0, L, M, T, taps, (a0, n, st, ph), *rots[256]) for st, ph in PAIRS])
    g, no = tn.tune_dev(tx, abs0=a0)
    assert no == RM.n_resample(L, M, a0, n) > 0
    check_rows(g, no, want, (shape, a0))


# ---- f: cuts on that NCO tuner ----------------------------------------------------------------------------------------------------------
def host_per(_lib, tn, L, M):
    """outputs per workgroup as p25fe_cuts_create counts them: the largest count of one cut for which 2^31 - 1 workgroups hold it.
    Found by bisection over the refusal, without a launch."""
    lib = _lib.load()
    out_p = C.c_void_p()

    def accepted(cnt):
        c = np.array([(0, -(-cnt * M // L), 1, 0)], dtype=_lib.CUT_DTYPE)
        rc = lib.p25fe_cuts_create(tn.tn, c.ctypes.data_as(C.c_void_p), 1, None, None, C.byref(out_p))
        assert rc in (_lib.OK, _lib.ERR_ARG)
        if rc == _lib.OK:
            lib.p25fe_cuts_destroy(out_p)
        return rc == _lib.OK
    W = (1 << 31) - 1
    lo, hi = 0, 2048 * W                                             # accepted(lo), not accepted(hi)
    assert accepted(1) and not accepted(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if accepted(mid) else (lo, mid)
    assert lo % W == 0
    return lo // W


@shapes
def test_cuts(mods, fe, rots, shape):
    """five cuts in one launch -- an odd start and 701 samples, exactly one workgroup's outputs, one output more, no output, the whole
    range -- each the slice of the NCO tuner's row, which test_nco_tuner ties to the model.  The workgroup counts come from plan();
    the host's own outputs per workgroup, read off p25fe_cuts_create's refusal of more than 2^31 - 1 workgroups, is plan()'s."""
    _lib, FE, RS, TN, CT = mods
    L, M, T = shape
    taps, x, _y, n, a, _ln = data(shape)
    ref = rows(shape, "nco", rots)
    tn = reference_tuner(TN, fe, L, M, T, taps, PAIRS)
    per = plan(L, M, T)[3] * RS_SUBS
    assert host_per(_lib, tn, L, M) == per == CM.tile(L, M, T) * CM.RS_SUBS
    a1 = a
    while RM.n_resample(L, M, a1, 701) == 0:                         # (M near 1024: the cut has to reach an output)
        a1 += 2
    none = next(d for d in range(a, a + 2 * M) if RM.n_resample(L, M, d, 1) == 0)
    cuts = [(a1, 701, 2), (3, len_for(L, M, 3, per), 1), (10, len_for(L, M, 10, per + 1), 3), (none, 1, 0), (0, n, 2)]
    assert a1 % 2 and all(c[0] + c[1] <= n for c in cuts)
    cnt = outputs_for(L, M, T)
    assert CM.wg_counts(L, M, T, cuts) == [1, 1, 2, 0, -(-cnt // per)] and -(-cnt // per) == 3
    ct = CT(tn, [(c[0], c[1], PAIRS[c[2]][0], PAIRS[c[2]][1]) for c in cuts])
    assert ct.counts == [RM.n_resample(L, M, c[0], c[1]) for c in cuts] and ct.counts[1:] == [per, per + 1, 0, cnt]
    out = ct.tune_dev(dev(x[:n]))
    check_cuts(rows_of(out, ct.counts), ref[:, :cnt], L, M, 0, cuts, [c[2] for c in cuts], shape)
    for j, c in enumerate(ct.counts):                                # zero-initialised rows: the tail stays zero
        assert not bool(out[j, c:].any()), (shape, j)
    ct.close()


# ---- g: host streaming ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["cf32", "u8"])
@pytest.mark.parametrize("shape", STREAMED, ids=shape_id)
def test_host_streaming(mods, fe, rots, shape, fmt):
    """T = 1 (no history buffer at all), T = 1024 (1023 samples kept, chunks shorter than that: the history moves up inside itself),
    L = 32 and a tile of 22: the chunks' outputs in a row are the one-call result, which is the device call's and, in cf32, the
    model's; after reset the same chunks give the same bits"""
    _lib, FE, RS, TN, CT = mods
    L, M, T = shape
    taps, xc, y = data(shape)[:3]
    n = len(xc)
    assert n >= sum(CHUNKS) + 1000
    x, unit = (np.array(xc), 1) if fmt == "cf32" else (noise(fmt, np.random.default_rng(70 + T), n), 2)
    edges = np.concatenate([[0], np.cumsum(CHUNKS), [n]])
    rs = RS(fe, L, M, T, taps)
    tn = reference_tuner(TN, fe, L, M, T, taps, PAIRS)
    tx = dev(x)
    for obj, call, dev_call in ((rs, rs.resample, rs.resample_dev), (tn, tn.tune, tn.tune_dev)):
        one = np.atleast_2d(call(x))
        g, no = dev_call(tx)
        assert one.shape[1] == no == RM.n_resample(L, M, 0, n)
        check_rows(g, no, one, (shape, fmt))
        if fmt == "cf32":
            want = y[None] if obj is rs else rows(shape, "nco", rots)
            assert np.array_equal(bits(one), bits(want)), (shape, obj is rs)
        for again in range(2):
            obj.reset()
            parts = [np.atleast_2d(call(x[unit * a:unit * b])) for a, b in zip(edges, edges[1:])]
            assert [p.shape[1] for p in parts] == [RM.n_resample(L, M, a, b - a) for a, b in zip(edges, edges[1:])]
            assert np.array_equal(bits(np.concatenate(parts, axis=1)), bits(one)), (shape, fmt, obj is rs, again)
