"""The tuner's cuts (docs/SPEC.md 3.0j, k_tune_cuts) on the GPU: many pieces of one capture in ONE launch, each bit for bit the slice
of the row p25fe_tune_dev writes for an NCO channel with the cut's (step, ph0) over the call's whole range -- and, so that the
reference is not only the library's other kernel, bit for bit tests/tune_cuts_model.py's row.  No tolerance anywhere in this file.

Every test runs on both designed tables: 2.5 Msps is L / M = 12 / 125 with T = 84 (180 outputs per sub-tile, three per lane: the
R > 1 branch of the host plan), 10 Msps is 3 / 125 with T = 334 (41 outputs per sub-tile: R = 1, tile < gl)."""
import ctypes as C

import numpy as np
import pytest

import resample_model as RM
import tune_cuts_model as CM
from test_gpu_tune import cnoise, host
from test_gpu_wide_fmt import bits, dev, noise

pytestmark = pytest.mark.gpu

RATES = (2500000, 10000000)
OFF_A = 232387521                                                    # a step off every raster (135 268.1 Hz at 2.5 Msps)
# the (step, ph0) pairs of the reference's channels: the centre (no product), the centre with a phase offset, a few thousand either
# way, the largest step, Nyquist, a step on the coarse table's raster (residual 0), off every raster with a phase offset
PAIRS = ((0, 0), (0, 0x12345678), (3001, 0), (-4507, 0), (0x7fffffff, 0), (-(1 << 31), 0), (5 << 24, 0), (OFF_A, 0x9abcdef1))
POISON = -123456.75


@pytest.fixture(scope="module")
def mods():
    from p25rx_amd import _lib
    from p25rx_amd.frontend import Cuts, FrontEnd, Tuner
    return _lib, FrontEnd, Tuner, Cuts


@pytest.fixture(scope="module")
def rot(mods):
    return mods[2].rotator(256)


@pytest.fixture(scope="module")
def tables(mods):
    """fs -> (L, M, T, taps) of the designed tables"""
    out = {}
    for fs in RATES:
        L, M, T, taps, _ = mods[2].design_nco(fs, [0.0])
        taps.setflags(write=False)
        out[fs] = (L, M, T, taps)
    assert out[2500000][:3] == (12, 125, 84) and out[10000000][:3] == (3, 125, 334)
    assert CM.tile(12, 125, 84) == 180 > 60 and CM.tile(3, 125, 334) == 41 < 63
    return out


def reference_tuner(TN, fe, L, M, T, taps, pairs):
    """an NCO tuner whose channel k has the pair pairs[k]: ph0 != 0 is reached through p25fe_afc_set_step(k, step, abs_at = ph0)
    from step + 1, which adds ((step + 1) - step) * ph0 to a phase offset of 0"""
    assert all(s < 0x7fffffff for s, p in pairs if p)
    tn = TN.nco(fe, L, M, T, taps, [s + 1 if p else s for s, p in pairs])
    for k, (s, p) in enumerate(pairs):
        if p:
            tn.set_step(k, s, p)
        assert tn.get_step(k) == (s, p), (k, tn.get_step(k))
    return tn


def len_for(L, M, a, cnt):
    """the smallest n for which a cut at a owns cnt outputs"""
    n = max(cnt * M // L - M, 0)
    while RM.n_resample(L, M, a, n) < cnt:
        n += 1
    assert RM.n_resample(L, M, a, n) == cnt
    return n


def lead_of(T):
    return (T - 1 + 7) // 8 * 8                                       # owned sample 0 on a 16-byte boundary in every format


def buffer_of(fmt, rng, T, n):
    """random samples of a format, [lead | n], as tests/test_gpu_wide_fmt.py's dev() takes them"""
    total = lead_of(T) + n
    return cnoise(rng, total) if fmt == "cf32" else noise(fmt, rng, total)


def rows_of(out, counts):
    return [host(out, c, j) for j, c in enumerate(counts)]


def check_cuts(got, ref_rows, L, M, a0, cuts, pair_of, what=None):
    """row j of the cuts' output is the slice of the reference's row of its pair"""
    for j, (c, g) in enumerate(zip(cuts, got)):
        m0, cnt = CM.slice_of(L, M, a0, c[0], c[1])
        want = ref_rows[pair_of[j]][m0:m0 + cnt]
        assert len(g) == cnt == len(want), (what, j, c, len(g), cnt, len(want))
        bad = np.flatnonzero((bits(g) != bits(want)).reshape(cnt, 2).any(axis=1))
        assert bad.size == 0, (what, j, c, bad[:8], g[bad[:4]], want[bad[:4]])


def cut_list(L, M, T, a0, n):
    """about 24 cuts of [a0, a0 + n) as (abs_first, n, pair index): see test_a_cut_is_the_slice"""
    per = CM.tile(L, M, T) * CM.RS_SUBS
    rel = []
    for r in range(8):                                               # start offsets of every residue mod 8
        rel.append((1000 + 8 * 37 * r + r, 700 + 131 * r))
    rel += [(5003, 0), (5004, 1), (6001, M - 1)]                     # lengths 0, 1 and M - 1
    rel += [(7002, len_for(L, M, a0 + 7002, per)), (7005, len_for(L, M, a0 + 7005, per + 1))]   # one workgroup's outputs, one more
    rel += [(0, n), (n - 5003, 5003)]                                # the whole range, a cut ending at n
    rel += [(20001, 9000), (24007, 9000)]                            # two overlapping cuts (different steps below)
    rel += [(30005, 4001), (30005, 4001)]                            # two identical cuts
    rel += [(40000 + 3 * k, 2000 + 17 * k) for k in range(4)]
    cuts = [(a0 + a, ln, k % len(PAIRS)) for k, (a, ln) in enumerate(rel)]
    cuts[18] = cuts[17]                                              # the identical ones: the same pair too
    assert {c[0] % 8 for c in cuts[:8]} == {(a0 + r) % 8 for r in range(8)} and len(cuts) == 23
    assert cuts[15][2] != cuts[16][2] and cuts[17] == cuts[18]
    assert {c[2] for c in cuts} == set(range(len(PAIRS)))
    assert all(a0 <= c[0] and c[0] + c[1] <= a0 + n for c in cuts)
    return cuts


# ---- 1: a cut is the slice -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["cf32", "s16", "u8"])
@pytest.mark.parametrize("fs", RATES)
def test_a_cut_is_the_slice(mods, tables, fs, fmt):
    """48 000 random samples at three positions, with no history and with T - 1 samples of it; 23 cuts in one launch: start offsets
    of every residue mod 8 (the three formats' vector alignments), lengths 0, 1 and M - 1, the lengths that give exactly one
    workgroup's outputs and one more, the whole range, a cut ending at n, two overlapping cuts with different steps, two identical
    cuts, every pair of PAIRS.  The reference is p25fe_tune_dev over the whole range on an NCO tuner with those pairs."""
    _lib, FE, TN, CT = mods
    L, M, T, taps = tables[fs]
    n, lead = 48000, lead_of(T)
    fe = FE()
    ref = reference_tuner(TN, fe, L, M, T, taps, PAIRS)
    raw = buffer_of(fmt, np.random.default_rng(fs % 1000 + len(fmt)), T, n)
    tx = dev(raw)
    per = CM.tile(L, M, T) * CM.RS_SUBS
    for a0 in (0, (1 << 32) - 20011, (1 << 40) + 3):
        cuts = cut_list(L, M, T, a0, n)
        ct = CT(ref, [(a, ln, PAIRS[p][0], PAIRS[p][1]) for a, ln, p in cuts])
        want_counts = [CM.slice_of(L, M, a0, a, ln)[1] for a, ln, _p in cuts]
        assert ct.counts == want_counts and ct.max_count == max(want_counts) == RM.n_resample(L, M, a0, n)
        assert want_counts[8] == 0 and want_counts[11] == per and want_counts[12] == per + 1
        assert CM.wg_counts(L, M, T, cuts)[11:13] == [1, 2]
        for n_hist in (0, T - 1):
            y, no = ref.tune_dev(tx, n_hist=n_hist, abs0=a0, offset=lead)
            ref_rows = [host(y, no, k) for k in range(len(PAIRS))]
            out = ct.tune_dev(tx, n_hist=n_hist, abs0=a0, offset=lead)
            assert out.shape[0] == len(cuts) and out.shape[1] % 2 == 0 and out.data_ptr() % 16 == 0
            check_cuts(rows_of(out, ct.counts), ref_rows, L, M, a0, cuts, [c[2] for c in cuts], (fs, fmt, a0, n_hist))
            for j, c in enumerate(ct.counts):                        # zero-initialised rows: the tail stays zero
                assert not bool(out[j, c:].any()), j
        ct.close()


# ---- 2: against the model --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", RATES)
def test_against_the_model(mods, rot, tables, fs):
    """cf32, the model's rows (tests/tune_cuts_model.py: tests/afc_model.py's mixer, tests/resample_model.py's resampler) bit for bit,
    at position 0 and past 2^40 with no history: cuts at odd places, the whole range, both kinds of pair"""
    _lib, FE, TN, CT = mods
    L, M, T, taps = tables[fs]
    n = 30011
    x = cnoise(np.random.default_rng(21), n)
    fe = FE()
    tn = TN.nco(fe, L, M, T, taps, [0])
    for a0 in (0, (1 << 40) + 3):
        cuts = [(a0, n, OFF_A, 0x9abcdef1), (a0 + 4999, 8001, -4507, 0), (a0 + 12346, 17000, 0, 0x12345678), (a0 + 29000, 1011, 0, 0),
                (a0 + 77, 3001, -(1 << 31), 0), (a0 + 5, 2500 * 8, 0x7fffffff, 7)]
        ct = CT(tn, cuts)
        buf = np.concatenate([np.full(2, 1000 + 1000j, dtype=np.complex64), x])      # junk in front of owned sample 0: never read as data
        out = ct.tune_dev(dev(buf), n_hist=0, abs0=a0, offset=2)
        for j, c in enumerate(cuts):
            want = CM.cut_row(x, a0, L, M, T, taps, c, *rot)
            got = host(out, ct.counts[j], j)
            assert ct.counts[j] == len(want) > 20 and np.array_equal(bits(got), bits(want)), (fs, a0, j)


# ---- 3: guards -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", RATES)
def test_guards(mods, tables, fs):
    """a poisoned output with a stride larger than any count: every word outside [0, cnt_j) of row j keeps its poison, the stride gap
    included, and so does the whole row of a cut without outputs"""
    import torch
    _lib, FE, TN, CT = mods
    L, M, T, taps = tables[fs]
    n, lead, a0 = 20000, lead_of(T), 12345
    fe = FE()
    ref = reference_tuner(TN, fe, L, M, T, taps, PAIRS[:3])
    tx = dev(cnoise(np.random.default_rng(31), lead + n))
    d = next(d for d in range(8, 200) if RM.n_resample(L, M, a0 + d, 2) == 0)           # two samples that own no output
    cuts = [(a0 + d, 2, 0), (a0 + 1001, 7001, 1), (a0, n, 2), (a0 + 3000, 0, 1), (a0 + n - 1, 1, 2), (a0 + 15000, 4999, 0), (a0 + n, 0, 0)]
    ct = CT(ref, [(a, ln, PAIRS[p][0], PAIRS[p][1]) for a, ln, p in cuts])
    assert ct.counts[0] == ct.counts[3] == ct.counts[6] == 0 and ct.counts[4] in (0, 1) and ct.max_count == ct.counts[2]
    stride = ct.max_count + 38
    out = torch.full((len(cuts), stride, 2), POISON, device="cuda")
    got = ct.tune_dev(tx, n_hist=T - 1, abs0=a0, offset=lead, out=out)
    assert got.data_ptr() == out.data_ptr()
    y, no = ref.tune_dev(tx, n_hist=T - 1, abs0=a0, offset=lead)
    check_cuts(rows_of(out, ct.counts), [host(y, no, k) for k in range(3)], L, M, a0, cuts, [c[2] for c in cuts], fs)
    for j, c in enumerate(ct.counts):
        assert bool((out[j, c:] == POISON).all()), (j, c)


# ---- 4: the workgroup map --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", RATES)
def test_4096_cuts_of_one_workgroup(mods, tables, fs):
    """4096 cuts of 300 samples at a stride of 11 samples: one workgroup each, the search at its full depth (12 halvings)"""
    _lib, FE, TN, CT = mods
    L, M, T, taps = tables[fs]
    lead, a0 = lead_of(T), (1 << 32) - 20011
    J = CM.CUTS_MAX
    n = 11 * (J - 1) + 300
    pairs = PAIRS[2:4] + PAIRS[6:8]
    cuts = [(a0 + 11 * j, 300, j % 4) for j in range(J)]
    assert CM.wg_counts(L, M, T, cuts) == [1] * J                     # the premise
    fe = FE()
    ref = reference_tuner(TN, fe, L, M, T, taps, pairs)
    tx = dev(cnoise(np.random.default_rng(41), lead + n))
    ct = CT(ref, [(a, ln, pairs[p][0], pairs[p][1]) for a, ln, p in cuts])
    out = ct.tune_dev(tx, n_hist=T - 1, abs0=a0, offset=lead)
    y, no = ref.tune_dev(tx, n_hist=T - 1, abs0=a0, offset=lead)
    ref_rows = [host(y, no, k) for k in range(4)]
    g = out.cpu().numpy().view(np.complex64)[..., 0]
    assert min(ct.counts) >= 300 * L // M - 1 > 0
    check_cuts([g[j, :c] for j, c in enumerate(ct.counts)], ref_rows, L, M, a0, cuts, [c[2] for c in cuts], fs)


@pytest.mark.parametrize("fs", RATES)
def test_cuts_of_one_two_and_three_workgroups(mods, tables, fs):
    """cuts that take 1, 2, 3, 1, 2, 3 ... workgroups, with cuts without outputs scattered among them and at both ends: a workgroup
    finds its cut and its place inside it by the prefix of the counts"""
    _lib, FE, TN, CT = mods
    L, M, T, taps = tables[fs]
    per = CM.tile(L, M, T) * CM.RS_SUBS
    lead, a0 = lead_of(T), (1 << 40) + 3
    want = [0, 1, 2, 3, 0, 0, 1, 2, 3, 0, 1, 2, 0, 3, 1, 2, 3, 0]
    cuts, at = [], a0 + 3
    for k, w in enumerate(want):
        cnt = 0 if w == 0 else (w * per if k % 2 else (w - 1) * per + 1 + 7 * k)    # full last workgroups and nearly empty ones
        ln = len_for(L, M, at, cnt) if w else (0 if k % 3 else 1)
        if w == 0 and ln == 1:
            while RM.n_resample(L, M, at, 1):                        # a cut of one sample that owns no output
                at += 1
        cuts.append((at, ln, k % len(PAIRS)))
        at += 1501 + 13 * k                                          # the cuts overlap in time
    n = max(a + ln for a, ln, _p in cuts) - a0 + 5
    assert CM.wg_counts(L, M, T, cuts) == want                        # the premise
    fe = FE()
    ref = reference_tuner(TN, fe, L, M, T, taps, PAIRS)
    tx = dev(cnoise(np.random.default_rng(42), lead + n))
    ct = CT(ref, [(a, ln, PAIRS[p][0], PAIRS[p][1]) for a, ln, p in cuts])
    out = ct.tune_dev(tx, n_hist=T - 1, abs0=a0, offset=lead)
    y, no = ref.tune_dev(tx, n_hist=T - 1, abs0=a0, offset=lead)
    check_cuts(rows_of(out, ct.counts), [host(y, no, k) for k in range(len(PAIRS))], L, M, a0, cuts, [c[2] for c in cuts], fs)


# ---- 5: an offset past 2^31 in the buffer ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", RATES)
def test_an_offset_past_two_to_the_31(mods, tables, fs):
    """u8, a zeroed buffer of 2^31 + 65 536 samples with random data in the last 65 536; one cut starts at sample 2^31 + 5: the
    smallest shape at which a 32-bit offset into the buffer goes wrong.  The reference is p25fe_tune_dev on the pointer advanced by
    2^31 samples with n_hist = T - 1 (the taps reach no further back)"""
    import torch
    _lib, FE, TN, CT = mods
    if torch.cuda.mem_get_info()[0] < 6 << 30:
        pytest.skip("needs 6 GB of free device memory")
    L, M, T, taps = tables[fs]
    big, tail, a0 = 1 << 31, 65536, 7
    buf = torch.zeros((big + tail, 2), dtype=torch.uint8, device="cuda")
    buf[big:] = torch.from_numpy(noise("u8", np.random.default_rng(51), tail).reshape(tail, 2)).cuda()
    fe = FE()
    ref = reference_tuner(TN, fe, L, M, T, taps, PAIRS[7:])
    cut = (a0 + big + 5, 60001, PAIRS[7][0], PAIRS[7][1])
    ct = CT(ref, [cut])
    out = ct.tune_dev(buf, n_hist=0, abs0=a0)
    y, no = ref.tune_dev(buf, n_hist=T - 1, abs0=a0 + big, offset=big)
    m0, cnt = CM.slice_of(L, M, a0 + big, cut[0], cut[1])
    assert ct.counts == [cnt] and cnt > 1400 and m0 + cnt <= no
    got, want = host(out, cnt, 0), host(y, no, 0)[m0:m0 + cnt]
    assert np.array_equal(bits(got), bits(want))
    assert len(np.unique(bits(got))) > cnt                            # data, not the conversion of a zeroed buffer


# ---- 6: splitting ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", RATES)
def test_splitting(mods, tables, fs):
    """one cut split at a sample inside one call, and across two calls -- on one stream and on two --, the second call with
    n_hist = T - 1: the concatenation is the unsplit cut"""
    import torch
    _lib, FE, TN, CT = mods
    L, M, T, taps = tables[fs]
    lead, a0, n = lead_of(T), (1 << 32) - 20011, 40000
    fe = FE()
    tn = TN.nco(fe, L, M, T, taps, [0])
    x = cnoise(np.random.default_rng(61), lead + n)
    tx = dev(x)
    st, ph = PAIRS[7]
    a, ln = a0 + 3001, 30003
    whole_ct = CT(tn, [(a, ln, st, ph)])
    whole = host(whole_ct.tune_dev(tx, n_hist=T - 1, abs0=a0, offset=lead), whole_ct.counts[0], 0)
    assert len(whole) == RM.n_resample(L, M, a, ln) > 700
    for s in (1, 12345, 12346, ln - 1, M, 8 * M + 3):
        ct = CT(tn, [(a, s, st, ph), (a + s, ln - s, st, ph)])
        out = ct.tune_dev(tx, n_hist=T - 1, abs0=a0, offset=lead)
        both = np.concatenate(rows_of(out, ct.counts))
        assert sum(ct.counts) == len(whole) and np.array_equal(bits(both), bits(whole)), s
    # two calls: [a0, a0 + c1) and [a0 + c1, a0 + n), the second in a buffer of its own with T - 1 samples of history
    for c1 in (3001 + 12345, 3001 + 16):
        s = c1 - 3001
        first, second = CT(tn, [(a, s, st, ph)]), CT(tn, [(a + s, ln - s, st, ph)])
        lead2 = lead
        buf2 = np.concatenate([np.full(lead2 - (T - 1), 1000 + 1000j, dtype=np.complex64), x[lead + c1 - (T - 1):]])
        tx1, tx2 = dev(x[:lead + c1]), dev(buf2)
        for streams in (1, 2):
            s2 = torch.cuda.Stream() if streams == 2 else torch.cuda.current_stream()
            o1 = first.tune_dev(tx1, n_hist=T - 1, abs0=a0, offset=lead)
            s2.wait_stream(torch.cuda.current_stream())              # (the inputs were uploaded on the current stream)
            with torch.cuda.stream(s2):
                o2 = second.tune_dev(tx2, n_hist=T - 1, abs0=a0 + c1, offset=lead2)
            torch.cuda.synchronize()
            both = np.concatenate([host(o1, first.counts[0], 0), host(o2, second.counts[0], 0)])
            assert np.array_equal(bits(both), bits(whole)), (c1, streams)


# ---- 7: refusals on an object ----------------------------------------------------------------------------------------------------------
def test_refusals(mods, tables):
    """every P25FE_ERR_ARG of p25fe_cuts_create and p25fe_cuts_dev with a live tuner; after each refused launch the poisoned
    output is untouched"""
    import torch
    _lib, FE, TN, CT = mods
    L, M, T, taps = tables[2500000]
    lib = _lib.load()
    fe = FE()
    tn = TN.nco(fe, L, M, T, taps, [5])
    out_p, mx = C.c_void_p(1), C.c_size_t(7)

    def create(tuner, cuts, n=None):
        c = np.array(cuts, dtype=_lib.CUT_DTYPE)
        out_p.value = 1
        rc = lib.p25fe_cuts_create(tuner, c.ctypes.data_as(C.c_void_p), len(c) if n is None else n, None, C.byref(mx), C.byref(out_p))
        assert rc == _lib.OK or not out_p.value
        return rc
    one = [(100, 5000, 12345, 0)]
    rational = TN(fe, L, M, T, taps, [(11, 200)])
    assert create(rational.tn, one) == _lib.ERR_ARG and create(None, one) == _lib.ERR_ARG
    assert create(tn.tn, one, n=0) == _lib.ERR_ARG and create(tn.tn, one * 4097) == _lib.ERR_ARG
    for bad in ((1 << 62, 1, 0, 0), (5, 1 << 62, 0, 0)):
        assert create(tn.tn, one + [bad]) == _lib.ERR_ARG, bad
    # more than 2^31 - 1 workgroups in total: 720 outputs each at 12 / 125
    assert create(tn.tn, [(0, (1 << 31) * 720 * 125 // 12 + 125, 1, 0)]) == _lib.ERR_ARG
    assert create(tn.tn, [(0, (1 << 30) * 720 * 125 // 12, 1, 0)] * 2 + [(0, 7500, 1, 0)]) == _lib.ERR_ARG
    assert create(tn.tn, [(0, (1 << 30) * 720 * 125 // 12, 1, 0), (0, ((1 << 30) - 1) * 720 * 125 // 12, 1, 0)]) == _lib.OK
    lib.p25fe_cuts_destroy(out_p)
    assert create(tn.tn, one * 4096) == _lib.OK and mx.value == RM.n_resample(L, M, 100, 5000)
    lib.p25fe_cuts_destroy(out_p)

    # the launch: cuts in [a0 + 100, a0 + 9000) of a call [a0, a0 + 10000)
    a0, n, lead = 12345, 10000, lead_of(T)
    ct = CT(tn, [(a0 + 100, 5000, 12345, 0), (a0 + 4000, 5000, -777, 9)])
    tx = dev(cnoise(np.random.default_rng(71), lead + n))
    stride = ct.max_count + 10
    out = torch.full((2, stride, 2), POISON, device="cuda")
    p_in, p_out = tx.data_ptr() + 8 * lead, out.data_ptr()

    def launch(ctp=None, d_iq=p_in, fmt=_lib.FMT_CF32, n_hist=T - 1, n_=n, a=a0, d_out=p_out, st=stride):
        rc = lib.p25fe_cuts_dev(ct.ct if ctp is None else ctp, C.c_void_p(d_iq), fmt, n_hist, n_, a, C.c_void_p(d_out), st, None)
        torch.cuda.synchronize()
        assert bool((out == POISON).all())
        return rc
    assert launch(ctp=C.c_void_p(None)) == _lib.ERR_ARG
    assert launch(d_iq=None) == _lib.ERR_ARG and launch(d_out=None) == _lib.ERR_ARG
    assert launch(d_iq=p_in + 8) == _lib.ERR_ARG and launch(d_out=p_out + 4) == _lib.ERR_ARG
    assert launch(fmt=3) == _lib.ERR_ARG and launch(fmt=-1) == _lib.ERR_ARG
    assert launch(a=1 << 62) == _lib.ERR_ARG and launch(a=(1 << 64) - 1) == _lib.ERR_ARG
    assert launch(st=ct.max_count - 1) == _lib.ERR_ARG and launch(st=0) == _lib.ERR_ARG and launch(st=1 << 50) == _lib.ERR_ARG
    # a cut not inside [abs_first, abs_first + n): the range too short, begun too late, somewhere else altogether
    assert launch(n_=8999) == _lib.ERR_ARG and launch(n_=0) == _lib.ERR_ARG
    assert launch(a=a0 + 101) == _lib.ERR_ARG and launch(a=a0 + 20000) == _lib.ERR_ARG and launch(a=0) == _lib.ERR_ARG
    # and the call that is right writes
    assert lib.p25fe_cuts_dev(ct.ct, C.c_void_p(p_in), _lib.FMT_CF32, T - 1, 9000, a0, C.c_void_p(p_out), stride, None) == _lib.OK
    torch.cuda.synchronize()
    assert bool((out[:, :ct.counts[0]] != POISON).all()) and bool((out[:, ct.max_count:] == POISON).all())


def test_destroy_after_the_tuner(mods, tables):
    """p25fe_cuts_destroy after the tuner and its handle are gone neither fails nor leaves an error behind for the thread's next call"""
    _lib, FE, TN, CT = mods
    L, M, T, taps = tables[2500000]
    x = dev(cnoise(np.random.default_rng(81), 5000))
    fe = FE()
    tn = TN.nco(fe, L, M, T, taps, [5])
    ct = CT(tn, [(10, 4000, 5, 0)])
    first = host(ct.tune_dev(x), ct.counts[0], 0)
    tn.close()
    fe.close()
    ct.close()
    fe2 = FE()
    tn2 = TN.nco(fe2, L, M, T, taps, [5])
    ct2 = CT(tn2, [(10, 4000, 5, 0)])
    assert np.array_equal(bits(host(ct2.tune_dev(x), ct2.counts[0], 0)), bits(first))


# ---- 8: end to end ---------------------------------------------------------------------------------------------------------------------
def symbols_compared(src, n_wide):
    """the truth symbol one slot before the keying's end: symbol s of a source sits at sample 50 (s + 4) of its 240 ksps stream"""
    end = n_wide if src[3] is None else src[3]
    return ((end - CM.SCENE_SLOT) * CM.SCENE_DOWN // CM.SCENE_UP) // 50 - 4


def place_of(dib, truth):
    """where the first 48 dibits are found in the truth"""
    return [p for p in range(len(truth) - 48) if np.array_equal(truth[p:p + 48], dib[:48])]


def test_end_to_end(mods, rot, tables):
    """capture -> waterfall -> keys -> cuts -> the K-row receive chain, on tests/tune_cuts_model.py's gated scene (five keyings on
    four raster channels, two of them neighbours, sources with a frame sync every 216 dibits).  The keys are the truth's intervals
    (tests/waterfall_model.py's +- 1 slot rule); every GPU row is the model's cut bit for bit; every row's dibits and sync
    positions are the oracle's on that zero-padded row; the dibits from each row's first sync on are found at exactly one place in
    the source's truth, and from there to the truth symbol one slot before the keying's end no symbol differs.  The CPU chain alone
    (model cut -> oracle) gives 0 errors in 1148, 323, 536, 556 and 456 compared symbols (docs/MEASUREMENTS.md, "Tuner, cuts"): the
    bound is 0."""
    from oracle import oracle as O
    from p25rx_amd.frontend import parse_results
    from p25rx_amd.scan import Scanner
    _lib, FE, TN, CT = mods
    x, truths = CM.gated_scene()
    N, hop, B, fs = CM.SCENE_N, CM.SCENE_HOP, CM.SCENE_B, CM.SCENE_FS
    L, M, T, taps = tables[fs]
    fe = FE()
    tx = dev(x)
    sc = Scanner(fe, N, hop, shift=CM.SCENE_SHIFT)
    rows = sc.waterfall_dev(tx, B)
    rows = (rows[0] if isinstance(rows, tuple) else rows).cpu().numpy().view(np.uint64)
    keys = Scanner.keys(rows, fs)
    truth = CM.gated_truth()
    assert len(keys) == len(truth) == 5 and len({t[0] for t in truth}) == 4
    for k, (r, a, b, _off, _src) in zip(keys, truth):
        assert int(k["raster_index"]) == r and abs(int(k["first_slot"]) - a) <= 1, (k, r, a)
        assert abs(int(k["first_slot"]) + int(k["n_slots"]) - 1 - b) <= 1 and int(k["n_slots"]) >= 20, (k, b)
    cuts = CT.from_keys(keys, N, hop, B, fs, margin=N, range_first=0, range_n=len(x))
    assert len(cuts) == 5 and [tuple(int(v) for v in c) for c in cuts] == CM.from_keys(
        [(int(k["raster_index"]), int(k["first_slot"]), int(k["n_slots"]), float(k["centre_hz"]), float(k["offset_hz"])) for k in keys],
        N, hop, B, fs, N, 0, len(x))
    tn = TN.nco(fe, L, M, T, taps, [0])
    ct = CT(tn, cuts)
    out = ct.tune_dev(tx)
    assert out.shape[1] % 2 == 0 and out.shape[1] >= ct.max_count and out.data_ptr() % 16 == 0
    padded = []
    for j, c in enumerate(cuts):
        want = CM.cut_row(x, 0, L, M, T, taps, tuple(int(v) for v in c), *rot)
        got = host(out, out.shape[1], j)
        assert ct.counts[j] == len(want) and np.array_equal(bits(got[:len(want)]), bits(want)) and not got[len(want):].any(), j
        padded.append(got)
    feJ = FE(n_channels=len(cuts))
    dib, res = feJ.run_dev(out)
    res = parse_results(res)
    bb, nb = feJ.demod_dev(out)
    _d2, _r2, spos, sdib = feJ.slice_dev(bb, nb, sync_cap=64)
    for j, (r, _a, _b, _off, src) in enumerate(truth):
        ref = O.run_cf32(padded[j])
        got = dib[j, :int(res[j]["n_dibits"])].cpu().numpy()
        assert np.array_equal(got, ref), j
        _dr, sp_ref, sd_ref = O.recv_range(O.Demod().feed_cf32(padded[j]))
        ns = int(res[j]["n_sync"])
        assert ns == len(sp_ref) >= 1, (j, ns, len(sp_ref))
        assert np.array_equal(spos[j, :ns].cpu().numpy(), sp_ref) and np.array_equal(sdib[j, :ns].cpu().numpy().view(np.uint64), sd_ref), j
        places = place_of(got, truths[src])
        assert len(places) == 1, (j, places)
        cnt = symbols_compared(CM.SCENE_SOURCES[src], len(x)) - places[0]
        errs = int(np.count_nonzero(got[:cnt] != truths[src][places[0]:places[0] + cnt]))
        print("keying %d (raster %d): %d errors in %d symbols from truth symbol %d" % (j, r, errs, cnt, places[0]))
        assert cnt >= 300 and len(got) >= cnt and errs == 0, (j, errs, cnt)
