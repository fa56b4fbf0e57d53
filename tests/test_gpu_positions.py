"""GPU tests at stream positions past 2^31 and 2^32: a front end that runs for days.

At 240 ksps the IQ index passes 2^32 after 4 h 58 min, the baseband index passes 2^31 after 12 h 26 min and 2^32 after 24 h 51 min.
Every stage is shift-invariant up to its grid residue (docs/SPEC.md section 4), so the CPU oracle run on the SAME samples at a small
position P' congruent to P modulo the stage's periods -- 5 for the decimator, 10 for the pre-decimator, 10 and the mixer's 192
for the channeliser, nothing for the receiver -- is a complete reference for any large position P: baseband bits, dibits, counts
and sync dibit indices are equal, every absolute index (sync_pos, anchor_out.s, first_event, carry_end, first_seg_end) is shifted by
exactly the baseband offset, and the -1 sentinels stay -1.

Every case places its range so that the power of two falls INSIDE it -- K samples past its start, where K lies on no receiver tile
edge (7 680 baseband samples) and no K1 sub-tile edge (320, hence on no segment edge) -- and asserts that it did: sync positions (or
baseband tiles, for the front end) on both sides.  No case allocates for its position, only for its length."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 7680                                  # receiver tile, baseband samples
K = 3 * TILE + 1234                          # baseband distance from a range's start to the boundary it straddles
assert K % TILE and K % 320 and K % 80       # not on a tile edge, a K1 sub-tile / segment edge or a plane byte
I64_MAX = np.iinfo(np.int64).max

# (name, power of two, the unit it counts): the boundaries a running receiver meets first, then two far ones
BOUNDS = [("bb31", 1 << 31, "bb"), ("bb32", 1 << 32, "bb"), ("iq32", 1 << 32, "iq"), ("p40", 1 << 40, "bb"), ("p56", 1 << 56, "bb")]
IDS = [b[0] for b in BOUNDS]


def bb_base(bound, k=K):
    """absolute baseband index of a range's first sample such that the boundary falls k (k_iq = 5 k + 2 for an IQ boundary: then
    in the middle of a decimation step) samples into it -> (base, boundary as a baseband index: the first sample at or above it)"""
    _, two, unit = bound
    if unit == "bb":
        return two - k, two
    first_above = (two - 4 + 4) // 5                     # baseband m is made at IQ index 5 m + 4: first m with 5 m + 4 >= 2^32
    return first_above - k, first_above


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def FE():
    from p25rx_amd.frontend import FrontEnd
    return FrontEnd


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


import chz_model as CM
from spec_model import grid_count as cnt       # samples i of [abs0, abs0 + n) with i % step == phase, in Python integers


def cf32_dev(iq):
    import torch
    return torch.from_numpy(np.ascontiguousarray(iq).view(np.float32).reshape(-1, 2)).cuda()


def u8_dev(u8):
    import torch
    return torch.from_numpy(np.ascontiguousarray(u8).reshape(-1, 2)).cuda()


def straddles(sp, boundary, what=""):
    sp = [int(x) for x in sp]
    assert any(x < boundary for x in sp) and any(x >= boundary for x in sp), "%s: no sync position on each side of %d" % (what, boundary)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. front end
# ------------------------------------------------------------------------------------------------------------------------------

def iq_base(bound, r):
    """absolute IQ index P with P % 5 == r whose first baseband sample is bb_base(bound)[0] (+ 1 where the residue skips one)"""
    b, edge = bb_base(bound)
    return 5 * b + r, edge


def check_front_tiles(P, n_iq, edge, phase=4):
    """the front-end straddle condition: at least one whole baseband tile of the range on each side of the boundary"""
    first = cnt(0, P, phase, 5)
    last = first + cnt(P, n_iq, phase, 5)
    assert first + TILE <= edge <= last - TILE, (first, edge, last)


@pytest.mark.parametrize("bound", BOUNDS, ids=IDS)
def test_demod_dev_fresh_history_every_residue(O, FE, c4fm_1s, bound):
    """p25fe_demod_dev, cf32, n_hist = 0 at abs0 = P: history reads as zeros, so the reference is the oracle with P % 5 zero samples
    in front.  All five residues, the built-in kernels; the count functions against Python integers on the way."""
    iq = c4fm_1s[0]
    t = cf32_dev(iq)
    fe = FE()
    assert fe.kernel_variant == 0
    L = fe.L
    for r in range(5):
        P, edge = iq_base(bound, r)
        check_front_tiles(P, len(iq), edge)
        ref = O.Demod().feed_cf32(np.concatenate([np.zeros(r, np.complex64), iq]))
        want = cnt(P, len(iq), 4, 5)
        assert len(ref) == want
        assert L.p25fe_n_baseband(P, len(iq)) == want and L.p25fe_n_baseband_h(fe.h, P, len(iq)) == want
        assert L.p25fe_n_predecim(P, len(iq)) == cnt(P, len(iq), 9, 10)
        bb, nb = fe.demod_dev(t, n_hist=0, abs0=P)
        assert nb == want
        assert np.array_equal(bits(bb[0, :nb].cpu().numpy()), bits(ref)), (bound[0], r)


@pytest.mark.parametrize("variant", ["builtin", "generic", "specialised"])
@pytest.mark.parametrize("bound", BOUNDS, ids=IDS)
def test_demod_dev_with_real_history_cf32_and_u8(O, FE, c4fm_1s, spec, bound, variant):
    """p25fe_demod_dev on a range INSIDE a buffer, p25fe_shard_halo() samples of real history in front of it, cf32 and u8, through
    the library's own kernels, the generic ones and one specialised handle.  The reference is the oracle over the whole buffer from
    position 0 (P' = the range's offset in the buffer, congruent to P modulo 5); every decimator phase other than the default runs
    too, with the handle's count function checked against Python integers."""
    from p25rx_amd import c4fm, _lib
    iq = c4fm_1s[0]
    u8 = c4fm.to_u8(iq)
    t, t8 = cf32_dev(iq), u8_dev(u8)
    dt = [float(np.float32(v)) for v in spec["decim_taps"]]
    dt[3] = float(np.float32(dt[3] * 1.25))                          # not the build's table: no immediate-coefficient kernel has it
    off = _lib.SPECIALIZE_OFF
    cases = {"builtin": [({}, {})] + [(dict(decim_phase=p), dict(decim_phase=p, specialize=off)) for p in (0, 1, 2, 3)],
             "generic": [(dict(decim_taps=dt, decim_phase=p), dict(decim_taps=dt, decim_phase=p, specialize=off)) for p in (4, 1)],
             "specialised": [({}, dict(specialize=_lib.SPECIALIZE_FORCE))]}[variant]
    want_variant = {"builtin": _lib.VARIANT_BUILTIN, "generic": _lib.VARIANT_GENERIC, "specialised": _lib.VARIANT_SPECIALIZED}[variant]
    for okw, fkw in cases:
        fe = FE(**fkw)
        assert fe.kernel_variant == want_variant
        phase = okw.get("decim_phase", 4)
        halo = fe.shard_halo()
        a = halo + 8 + 8 * phase                                     # 16-byte aligned start for both formats
        ocfg = O.make_config(**okw)
        for src, ref in ((t, O.Demod(ocfg).feed_cf32(iq)), (t8, O.Demod(ocfg).feed_u8(u8))):
            b, edge = bb_base(bound)
            p0 = cnt(0, a, phase, 5)
            P = 5 * (b - p0) + a                                     # P % 5 == a % 5, first owned baseband sample at index b
            n = len(iq) - a
            assert P % 5 == a % 5 and cnt(0, P, phase, 5) == b
            check_front_tiles(P, n, edge, phase)
            want = cnt(P, n, phase, 5)
            assert fe.n_baseband(P, n) == want == cnt(a, n, phase, 5)
            bb, nb = fe.demod_dev(src, n_hist=halo, abs0=P, offset=a)
            assert nb == want
            assert np.array_equal(bits(bb[0, :nb].cpu().numpy()), bits(ref[p0:p0 + nb])), (bound[0], variant, phase, src.dtype)


@pytest.mark.parametrize("two", [31, 32, 40, 56])
def test_predecim_and_channelise_at_large_abs0(O, FE, spec, two):
    """p25fe_predecim_dev (bit-exact) and p25fe_channelise_dev (the tolerance of test_channeliser_parity_and_end_to_end: per output
    (2e-6 + 2^-24) * T of tests/chz_model.py, and never more than 2e-6 * sum|h| * max|x|) with abs0 straddling 2^31, 2^32, 2^40
    and 2^56 wideband samples, over all ten residues of the 10:1 grid.
    References: the oracle's pre-decimator with P % 10 zeros in front; oracle.channelise at P' = P mod lcm(10, 192) AND at P itself."""
    hsum = float(np.abs(np.array(spec["pre_taps"], dtype=np.float64)).sum())
    rng = np.random.default_rng(two)
    n = 20008
    x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.3).astype(np.complex64)
    tol = 2e-6 * hsum * float(np.abs(x).max())
    t = cf32_dev(x)
    fe = FE()
    for r in range(10):
        P = (1 << two) - n // 2 - 3
        P += (r - P) % 10
        assert P % 10 == r and P < (1 << two) < P + n - 640
        no_want = cnt(P, n, 9, 10)
        assert fe.L.p25fe_n_predecim(P, n) == no_want
        ref0 = O.PreDecim(spec).feed(np.concatenate([np.zeros(r, np.complex64), x]))
        y, no = fe.predecim_dev(t, n_hist=0, abs0=P)
        assert no == no_want == len(ref0)
        assert np.array_equal(y[0, :no].cpu().numpy().view(np.uint32), ref0.view(np.float32).reshape(-1, 2).view(np.uint32)), r
        small = O.channelise(x, abs0=P % 960, spec=spec)
        large = O.channelise(x, abs0=P, spec=spec)
        assert small.shape[1] == no_want and np.array_equal(small.view(np.uint32), large.view(np.uint32))
        z, nz = fe.channelise_dev(t, n_hist=0, abs0=P)
        assert nz == no_want
        got = z[:, :nz].cpu().numpy().view(np.complex64)[..., 0]
        CM.within(got, x, 0, P, k=CM.K_SPEC + CM.U, ref=small, cap=tol, what="2^%d, r = %d" % (two, r))


# ------------------------------------------------------------------------------------------------------------------------------
# 2. receiver: p25fe_slice_dev at a large abs_bb0
# ------------------------------------------------------------------------------------------------------------------------------

def oracle_recv(O, bb, mode, resync=()):
    """the oracle's receiver over bb from a fresh stream (position 0), lock dropped before each listed index; mode 2: SPEC 3.8c"""
    cfg = O.make_config(symbol_clock=mode)
    if mode == 2:
        d, sp, sd = O.recv_range(bb, cfg, sorted(resync))
        return d, sp, sd.astype(np.uint64)
    r = O.Recv(cfg)
    outs, o = [], 0
    for q in sorted(resync):
        q = min(max(int(q), 0), len(bb))
        outs.append(r.feed(bb[o:q]))
        r.resync()
        o = q
    outs.append(r.feed(bb[o:]))
    return (np.concatenate([x[0] for x in outs]), np.concatenate([x[1] for x in outs]),
            np.concatenate([x[2] for x in outs]).astype(np.uint64))


def dev_slice(fe, t, n_bb, base, resync=None, anchor=None, offset=0, n_hist=0, sync_cap=4096):
    """p25fe_slice_dev at abs_bb0 = base (+ offset into t); resync: ABSOLUTE indices, one list or one per channel (short rows padded
    with INT64_MAX) -> per channel (dibits, sync_pos, sync_dibit, result record)"""
    import torch
    from p25rx_amd.frontend import parse_results
    if resync is not None:
        rows = resync if resync and isinstance(resync[0], (list, tuple)) else [resync]
        arr = np.full((len(rows), max(len(x) for x in rows)), I64_MAX, dtype=np.int64)
        for c, x in enumerate(rows):
            arr[c, :len(x)] = sorted(int(q) for q in x)
        fe.resync_at_dev(torch.from_numpy(arr).cuda() if len(rows) > 1 else torch.from_numpy(arr[0]).cuda())
    dib, res, sp, sd = fe.slice_dev(t, n_bb, n_hist_bb=n_hist, abs_bb0=base + offset, anchor_in=anchor, offset=offset, sync_cap=sync_cap)
    rr = parse_results(res)
    out = []
    for c in range(fe.C):
        nd, ns = int(rr[c]["n_dibits"]), int(rr[c]["n_sync"])
        assert ns <= sync_cap and nd <= dib.shape[1]
        out.append((dib[c, :nd].cpu().numpy(), sp[c, :ns].cpu().numpy(), sd[c, :ns].cpu().numpy().astype(np.uint64), rr[c]))
    return out


def same_shifted(got, ref, shift, what):
    """(dibits, sync_pos, sync_dibit) against the reference at position 0: sync_pos shifted, the rest equal"""
    assert len(got[0]) == len(ref[0]) and np.array_equal(got[0], ref[0]), what + ": dibits"
    assert len(got[1]) == len(ref[1]) and [int(x) for x in got[1]] == [int(x) + shift for x in ref[1]], what + ": sync_pos"
    assert np.array_equal(got[2], np.asarray(ref[2], dtype=np.uint64)), what + ": sync_dibit"


def record_shifted(big, small, shift, what):
    """the result record at the large position against the same call's at the small one: counts, thresholds, clock and flags equal,
    every absolute index shifted by exactly `shift`, -1 stays -1"""
    for f in ("n_baseband", "n_dibits", "n_sync", "n_dibits_after_first", "flags", "reserved"):
        assert int(big[f]) == int(small[f]), (what, f, int(big[f]), int(small[f]))
    for f in ("first_event", "carry_end", "first_seg_end"):
        s = int(small[f])
        assert int(big[f]) == (s + shift if s >= 0 else -1), (what, f, int(big[f]), s, shift)
    a, b = big["anchor_out"], small["anchor_out"]
    for f in ("hi", "mid", "lo", "valid", "period_d", "period_n"):
        assert a[f].tobytes() == b[f].tobytes(), (what, "anchor_out." + f)
    if int(b["valid"]):
        assert int(a["s"]) == int(b["s"]) + shift, (what, "anchor_out.s", int(a["s"]), int(b["s"]), shift)


def recv_case(O, FE, bb, mode, bound, what, drops=None, oracle_ref=None, k=K, sync_cap=4096):
    """one baseband through p25fe_slice_dev at the small position 0 and at the large one; drops are indices into bb.  The oracle pins
    dibits and events, the small-position call pins the record.  Returns the large run."""
    import torch
    base, edge = bb_base(bound, k)
    ref = oracle_ref if oracle_ref is not None else oracle_recv(O, bb, mode, drops or ())
    t = torch.from_numpy(np.ascontiguousarray(bb)).cuda()
    fe = FE(symbol_clock=mode)
    small = dev_slice(fe, t, len(bb), 0, resync=drops, sync_cap=sync_cap)[0]
    big = dev_slice(fe, t, len(bb), base, resync=None if drops is None else [q + base for q in drops], sync_cap=sync_cap)[0]
    same_shifted(small, ref, 0, what + " (small)")
    same_shifted(big, ref, base, what)
    record_shifted(big[3], small[3], base, what)
    straddles(big[1], edge, what)
    if len(ref[1]) and not drops:
        assert int(big[3]["anchor_out"]["s"]) == int(ref[1][-1]) + base
    return big


@pytest.fixture(scope="module")
def bb_1s(O, c4fm_1s):
    return O.Demod().feed_cf32(c4fm_1s[0])


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("bound", BOUNDS, ids=IDS)
def test_slice_dev_free_running_and_carry_in(O, FE, bb_1s, bound, mode):
    """Free running over the boundary; then the same baseband as two calls, the second with a carry-in anchor whose s lies shortly
    before its range (the first call's anchor_out, which for the fixed stride must be the oracle's state, shifted)."""
    import torch
    bb = bb_1s
    big = recv_case(O, FE, bb, mode, bound, "free running, mode %d" % mode)
    base, edge = bb_base(bound)
    # cut 60 samples behind a sync word's decision, below the boundary, so that the second range crosses it under the carried lock
    sp = [int(x) - base for x in big[1]]
    cut = [s for s in sp if s + 65 < K][-1] + 65
    t = torch.from_numpy(bb).cuda()
    outs = {}
    for name, shift in (("small", 0), ("big", base)):
        fe = FE(symbol_clock=mode)
        a = dev_slice(fe, t[:cut], cut, shift)[0]
        anc = np.array([a[3]["anchor_out"]], dtype=a[3]["anchor_out"].dtype)
        assert int(anc["valid"][0]) & 1 and cut - 80 <= int(anc["s"][0]) - shift < cut
        b = dev_slice(fe, t, len(bb) - cut, shift, anchor=anc, offset=cut, n_hist=cut)[0]
        outs[name] = (a, b)
    (sa, sb), (ba, bbig) = outs["small"], outs["big"]
    for x, y, w in ((ba, sa, "head"), (bbig, sb, "carry-in")):
        same_shifted(x[:3], y[:3], base, "%s, mode %d" % (w, mode))
        record_shifted(x[3], y[3], base, "%s, mode %d" % (w, mode))
    straddles(list(ba[1]) + list(bbig[1]), edge)
    assert any(int(x) < edge for x in ba[1]) and int(bbig[3]["n_dibits"]) > 3000
    if mode < 2:                                                     # causal clocks: two calls give the one-pass oracle's stream
        r = O.Recv(O.make_config(symbol_clock=mode))
        ra = r.feed(bb[:cut])
        st = r.state()
        rb = r.feed(bb[cut:])
        assert np.array_equal(np.concatenate([ba[0], bbig[0]]), np.concatenate([ra[0], rb[0]]))
        assert [int(x) for x in bbig[1]] == [int(x) + base for x in rb[1]]
        if mode == 0:
            a = ba[3]["anchor_out"]
            assert int(a["s"]) == st["s"] + base
            assert [np.float32(a[f]).tobytes() for f in ("hi", "mid", "lo")] == [np.float32(st[f]).tobytes() for f in ("hi", "mid", "lo")]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("bound", BOUNDS, ids=IDS)
def test_slice_dev_lock_drops_at_large_absolute_indices(O, FE, bb_1s, bound, mode):
    """p25fe_resync_at_dev lists given as large ABSOLUTE indices: at a decision index, one sample either side, on a tile edge, at
    the power of two itself and beside it, past the end -- one at a time and together."""
    bb = bb_1s
    look = 2 if mode else 0
    free = oracle_recv(O, bb, mode if mode < 2 else 1)
    e = [int(s) + 5 + look for s in free[1]]                         # decision indices (s + W, the tracking clocks 2 later)
    below = [x for x in e if x < K]
    above = [x for x in e if x > K + 300]
    assert len(below) >= 2 and len(above) >= 2
    cases = {"decision index below": [below[-1]], "one before": [above[0] - 1], "decision index above": [above[0]], "one after": [above[0] + 1],
             "tile edge": [2 * TILE - look], "tile edge + 1": [4 * TILE - look + 1], "the power of two": [K], "one below it": [K - 1],
             "past the end": [len(bb) + 50],
             "several": [below[0], below[-1] + 1, K - 1, K, above[0], above[1] - 1, 4 * TILE, 5 * TILE - 1, len(bb) + 7]}
    for name, drops in cases.items():
        recv_case(O, FE, bb, mode, bound, "%s, mode %d" % (name, mode), drops=drops)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("bound", BOUNDS, ids=IDS)
def test_slice_dev_two_channels_with_padded_drop_rows(O, FE, bb_1s, bound, mode):
    """A two-channel handle whose second row of lock drops is shorter: padded with INT64_MAX, which is no position and must drop
    nothing, however close to it the real indices come."""
    import torch
    base, edge = bb_base(bound)
    rows = np.stack([bb_1s, np.roll(bb_1s, 1777)])
    drops = [[K - 3000, K + 11, K + 5000, 40000], [K + 2222]]
    refs = [oracle_recv(O, rows[c], mode, drops[c]) for c in range(2)]
    assert len(refs[1][0]) != len(oracle_recv(O, rows[1], mode)[0])   # the one real drop of row 1 costs symbols
    t = torch.from_numpy(rows).cuda()
    fe = FE(n_channels=2, symbol_clock=mode)
    small = dev_slice(fe, t, rows.shape[1], 0, resync=drops)
    big = dev_slice(fe, t, rows.shape[1], base, resync=[[q + base for q in x] for x in drops])
    for c in range(2):
        same_shifted(big[c], refs[c], base, "channel %d" % c)
        record_shifted(big[c][3], small[c][3], base, "channel %d" % c)
        straddles(big[c][1], edge)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("bound", BOUNDS, ids=IDS)
def test_slice_dev_dense_planes_at_a_large_base(FE, O, bound, mode):
    """tests/golden/dense_planes.npz (hundreds of detections per tile: the slicers' 64-at-a-time register lists, K2's sorted in-tile
    lists and their packed fields) at a large base, without and with its lock drops; the file's own expected outputs are the
    reference."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "dense_planes.npz"))
    bb = g["bb_bits"].view(np.float32)
    k = K if len(bb) > K + TILE else len(bb) // 2 + 37
    assert k % TILE and k % 320
    for tag, drops in (("", None), ("_drops", [int(x) for x in g["drops"]])):
        want = (g["dibits_m%d%s" % (mode, tag)], g["sync_pos_m%d%s" % (mode, tag)], g["sync_dibit_m%d%s" % (mode, tag)].astype(np.uint64))
        recv_case(O, FE, bb, mode, bound, "dense planes, mode %d%s" % (mode, tag), drops=drops, oracle_ref=want, k=k, sync_cap=4096)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("bound", BOUNDS, ids=IDS)
def test_slice_dev_clock_error_at_a_large_base(O, FE, bound, mode):
    """A capture with a sample-clock error: rational-clock instants (s + (j D) div N), clock_count and count_instants with large
    operands, under both tracking clocks -- and the fixed stride, which re-anchors at every sync word of such a capture and slips
    symbols in between exactly as the oracle's does."""
    from p25rx_amd import c4fm
    iq = c4fm.synth(2.0, seed=21, snr_db=30.0, frame_dibits=864, clock_ppm=100.0)[0]
    bb = O.Demod().feed_cf32(iq[:len(iq) // 8 * 8])
    big = recv_case(O, FE, bb, mode, bound, "100 ppm, mode %d" % mode)
    a = big[3]["anchor_out"]
    if mode == 1:
        assert int(a["period_n"]) == 4 * 864 and abs(int(a["period_d"]) - 4 * 864 * 10 * (1 + 100e-6)) <= 6


# ------------------------------------------------------------------------------------------------------------------------------
# 3. time shards at a large abs0
# ------------------------------------------------------------------------------------------------------------------------------

# The calls that see the stream in pieces -- the shard passes and the streaming entry points -- refuse symbol_clock = 2 by design
# (include/p25fe.h, ABI 6); with P25FE_CLOCK_CAUSAL_OK or-ed in they run it as the causal tracking clock.
PIECEWISE_MODES = [0, 1, 2, 0x102]
PIECEWISE_IDS = ["fixed", "tracking", "reslice", "reslice+causal_ok"]


def oracle_mode(mode):
    return 1 if mode == 0x102 else mode


def run_shards(FE, t, a0, cuts, D, mode=0):
    """The shard procedure over the capture t[a0:] (buffer index = absolute index - D; D % 5 == 0; the lead-in t[:a0] is the first
    shard's history) cut at `cuts`: pass 1 in its four forms, host and device resolve, pass 2 in its three forms (one of them as a
    pipelined step).  -> dict of everything that has to be position-independent or shifted."""
    import torch
    from p25rx_amd.frontend import parse_results
    fe = FE(symbol_clock=mode)
    halo = fe.shard_halo()
    L = fe.L
    fes = [FE(symbol_clock=mode) for _ in range(len(cuts) - 1)]
    summ, bb0, bbn = [], [], []
    side = torch.cuda.Stream()
    for r, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        h = min(a, halo)
        assert h == halo
        args = dict(offset=h, n_hist=h, abs0=a + D)
        src = t[a - h:b]
        if r == 0:
            res = fes[r].shard_pass1(src, **args)
        elif r == 1:
            fes[r].shard_pass1_main(src, **args)
            res = fes[r].shard_pass1_finish(src, **args)
        elif r == 2:
            fes[r].shard_pass1_main(src, **args)
            fes[r].shard_pass1_head(src, **args)
            res = fes[r].shard_pass1_finish(src, **args)
        else:
            fes[r].shard_pass1_k1(src, **args)
            res = fes[r].shard_pass1_finish(src, **args)
        summ.append(parse_results(res)[0])
        bb0.append(int(L.p25fe_n_baseband(0, a + D)))
        bbn.append(int(L.p25fe_n_baseband(a + D, b - a)))
        assert bb0[-1] == cnt(0, a + D, 4, 5) and bbn[-1] == cnt(a + D, b - a, 4, 5)
    anc, off = fe.shard_resolve(np.array(summ), bb0, bbn)
    summ_t = torch.from_numpy(np.frombuffer(np.array(summ).tobytes(), dtype=np.uint8).copy()).view(len(summ), -1).cuda()
    d_bb0 = torch.tensor(bb0, dtype=torch.int64, device="cuda")
    d_bbn = torch.tensor(bbn, dtype=torch.int64, device="cuda")
    d_anc, d_off = fe.shard_resolve_dev(summ_t, d_bb0, d_bbn)
    assert d_anc.cpu().numpy().tobytes() == anc.tobytes(), "host and device resolve: anchors"
    assert d_off.cpu().numpy().astype(np.uint64).tobytes() == off.tobytes(), "host and device resolve: offsets"
    out = dict(summ=np.array(summ), anc=anc, off=off, bb0=bb0)
    # pass 2 with the combine inside it, straight after pass 1
    fused, recs = [], []
    for r in range(len(fes)):
        dib, res, anc3, off3 = fes[r].shard_pass2_dev(summ_t, d_bb0, d_bbn, r, bbn[r])
        assert anc3.cpu().numpy().tobytes() == anc.tobytes() and off3.cpu().numpy().astype(np.uint64).tobytes() == off.tobytes()
        rec = parse_results(res)[0]
        recs.append(rec)
        fused.append(dib[0, :int(rec["n_dibits"])].cpu().numpy())
    out["pass2_dev"], out["recs"] = np.concatenate(fused), np.array(recs)
    # plain pass 2 with the host anchors, then with the device anchors
    for key, anchors in (("pass2", lambda r: anc[r:r + 1]), ("pass2_dev_anchor", lambda r: d_anc[r:r + 1])):
        rows = []
        for r in range(len(fes)):
            dib, res = fes[r].shard_pass2(anchors(r), bbn[r], t.device)
            rec = parse_results(res)[0]
            assert rec.tobytes() == recs[r].tobytes(), (key, r)
            assert int(off[r]) == sum(len(x) for x in rows)
            rows.append(dib[0, :int(rec["n_dibits"])].cpu().numpy())
        out[key] = np.concatenate(rows)
    # one pipelined step of the last shard: main on the caller's stream, head on a side stream, the rest on the receive stream
    r = len(fes) - 1
    a, b = cuts[r], cuts[r + 1]
    src = t[a - halo:b]
    args = dict(offset=halo, n_hist=halo, abs0=a + D)
    f = fes[r]
    st = torch.cuda.current_stream()
    rx = f.shard_pipe_begin()
    fork = st.record_event()
    f.shard_pass1_main(src, **args)
    with torch.cuda.stream(side):
        side.wait_event(fork)
        f.shard_pass1_head(src, **args)
    with torch.cuda.stream(rx):
        res1 = f.shard_pass1_finish(src, **args)
        summ_p = torch.cat([summ_t[:r], res1])
        dib, res2, _, _ = f.shard_pass2_dev(summ_p, d_bb0, d_bbn, r, bbn[r])
    f.shard_pipe_end()
    f.join_dev()
    torch.cuda.synchronize()
    f.shard_head_check()
    rec = parse_results(res2)[0]
    assert parse_results(res1)[0].tobytes() == summ[r].tobytes() and rec.tobytes() == recs[r].tobytes(), "pipelined step"
    assert np.array_equal(dib[0, :int(rec["n_dibits"])].cpu().numpy(), fused[r]), "pipelined step: dibits"
    return out


@pytest.mark.parametrize("mode", PIECEWISE_MODES, ids=PIECEWISE_IDS)
@pytest.mark.parametrize("bound", BOUNDS, ids=IDS)
def test_time_shards_at_a_large_abs0(O, FE, bound, mode):
    """Four shards of one capture placed at P (behind a lead-in of zeros, which is what the start of a stream reads as): every form
    of pass 1, both resolves (byte-equal to each other), every form of pass 2 and one pipelined step.  The concatenated dibits equal
    the one-pass oracle; summaries, anchors and final records equal those of the same capture at P' = its offset in the buffer,
    shifted; offsets equal."""
    from p25rx_amd import c4fm, _lib
    iq = c4fm.synth(2.0, seed=33, snr_db=20.0, frame_dibits=1500, clock_ppm=80.0 if mode else 0.0)[0]
    halo = FE().shard_halo()
    a0 = halo + 8
    buf = np.concatenate([np.zeros(a0, np.complex64), iq])
    buf = buf[:len(buf) // 8 * 8]
    t = cf32_dev(buf)
    cuts = [a0, a0 + 100004, a0 + 100004 + 3002, a0 + 310006, len(buf)]      # uneven, even cut points, one short shard
    base, edge = bb_base(bound)
    p0 = cnt(0, a0, 4, 5)
    D = 5 * (base - p0)
    if mode == 2:
        fe = FE(symbol_clock=2)
        for form in (fe.shard_pass1, fe.shard_pass1_main, fe.shard_pass1_k1):
            with pytest.raises(_lib.P25feError) as e:
                form(t[cuts[0] - halo:cuts[1]], offset=halo, n_hist=halo, abs0=cuts[0] + D)
            assert e.value.status == _lib.ERR_ARG
        pytest.skip("symbol_clock = 2 through p25fe_shard_pass1 / _main / _k1 (and with them _head, _finish, p25fe_shard_pass2, "
                    "p25fe_shard_pass2_dev, p25fe_shard_pipe_begin / _end) at %s: refused by design with P25FE_ERR_ARG (checked above); "
                    "the reslice+causal_ok case runs these calls" % bound[0])
    ref = oracle_recv(O, O.Demod().feed_cf32(buf), oracle_mode(mode))
    small = run_shards(FE, t, a0, cuts, 0, mode)
    big = run_shards(FE, t, a0, cuts, D, mode)
    shift = D // 5
    assert big["bb0"][0] == base and [x - shift for x in big["bb0"]] == small["bb0"]
    for key in ("pass2_dev", "pass2", "pass2_dev_anchor"):
        assert np.array_equal(small[key], ref[0]), key + " (small)"
        assert np.array_equal(big[key], ref[0]), key
    assert big["off"].tobytes() == small["off"].tobytes() and int(big["off"][-1]) == len(ref[0])
    for r in range(len(cuts) - 1):
        record_shifted(big["summ"][r], small["summ"][r], shift, "summary %d" % r)
        record_shifted(big["recs"][r], small["recs"][r], shift, "final record %d" % r)
        a, b = big["anc"][r], small["anc"][r]
        for f in ("hi", "mid", "lo", "valid", "period_d", "period_n"):
            assert a[f].tobytes() == b[f].tobytes(), ("anchor", r, f)
        if int(b["valid"]):                                          # (s of an anchor that is not valid means nothing)
            assert int(a["s"]) == int(b["s"]) + shift, ("anchor", r)
    s_all = [int(x["anchor_out"]["s"]) for x in big["summ"] if int(x["anchor_out"]["valid"])] + \
            [int(x["first_event"]) for x in big["summ"] if int(x["first_event"]) >= 0]
    straddles(s_all, edge, "shard summaries")
    assert int(big["recs"][-1]["anchor_out"]["s"]) == int(ref[1][-1]) + shift


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the streaming handle
# ------------------------------------------------------------------------------------------------------------------------------
# The state blob, as p25fe_api.hip writes it (StreamState::write; `struct StateHeader { uint32_t magic, abi; int32_t n_channels,
# fmt_locked; uint64_t abs_iq, abs_bb; }`, 32 bytes):
#     header | IQ history | baseband tail | anchors [C] (p25fe_anchor_t) | totals [C] (uint64_t)
# so abs_iq is the uint64 at byte 16, abs_bb the one at byte 24, and with n = p25fe_state_size the anchors are the C *
# sizeof(p25fe_anchor_t) bytes that end C * 8 bytes before n.  The two middle sections hold samples, no positions.
HDR = np.dtype([("magic", "<u4"), ("abi", "<u4"), ("n_channels", "<i4"), ("fmt_locked", "<i4"), ("abs_iq", "<u8"), ("abs_bb", "<u8")])
assert HDR.itemsize == 32


def blob_header(blob):
    return np.frombuffer(blob[:32].tobytes(), dtype=HDR)[0]


def blob_anchors(blob, Cn):
    from p25rx_amd._lib import ANCHOR_DTYPE
    lo = len(blob) - 8 * Cn - ANCHOR_DTYPE.itemsize * Cn
    return lo, np.frombuffer(blob[lo:lo + ANCHOR_DTYPE.itemsize * Cn].tobytes(), dtype=ANCHOR_DTYPE).copy()


def move_stream(fe, d_iq, d_bb):
    """export, move the stream d_iq IQ / d_bb baseband samples ahead (header counters and every valid anchor's s), import"""
    from p25rx_amd._lib import ANCHOR_DTYPE
    blob = np.array(fe.state_export(), copy=True)
    hd = np.frombuffer(blob[:32].tobytes(), dtype=HDR).copy()
    assert int(hd["n_channels"][0]) == fe.C
    before = (int(hd["abs_iq"][0]), int(hd["abs_bb"][0]))
    hd["abs_iq"] += np.uint64(d_iq)
    hd["abs_bb"] += np.uint64(d_bb)
    blob[:32] = np.frombuffer(hd.tobytes(), dtype=np.uint8)
    lo, anc = blob_anchors(blob, fe.C)
    for c in range(fe.C):
        if int(anc["valid"][c]):
            anc["s"][c] += d_bb
    blob[lo:lo + ANCHOR_DTYPE.itemsize * fe.C] = np.frombuffer(anc.tobytes(), dtype=np.uint8)
    fe.state_import(blob)
    return before, anc


STREAM_CALLS = ["demod_cf32+slice", "demod_u8+slice", "run_cf32", "run_u8", "run_host_windows"]


def stream_through(fe, call, iq, u8, chunks, shift_bb, dev_drops=(), host_at=()):
    """the capture through one streaming entry point in chunks [(o, n) IQ samples]; dev_drops: ABSOLUTE baseband indices handed to
    p25fe_resync_at_dev before the receiver call of the chunk that holds them; host_at: chunk starts (IQ) before which p25fe_resync()
    is called.  -> (dibits per channel, sync_pos per channel or None)"""
    import torch
    Cn = fe.C
    dib, sps = [[] for _ in range(Cn)], [[] for _ in range(Cn)]
    for o, n in chunks:
        lo, hi = shift_bb + cnt(0, o, 4, 5), shift_bb + cnt(0, o + n, 4, 5)
        if o in host_at:
            fe.resync()
        mine = [q for q in dev_drops if lo <= q < hi]

        def arm():
            if mine:
                fe.resync_at_dev(torch.tensor(mine, dtype=torch.int64, device="cuda"))
        x = iq[..., o:o + n]
        x8 = u8[..., 2 * o:2 * (o + n)]
        if call.endswith("+slice"):
            bb = fe.demod_cf32(x) if call == "demod_cf32+slice" else fe.demod_u8(x8)
            assert np.shape(bb)[-1] == hi - lo
            arm()
            out = fe.slice(bb)
            for c, (d, sp, _) in enumerate(out if Cn > 1 else [out]):
                dib[c].append(d); sps[c].append(sp)
        else:
            arm()
            if call == "run_cf32":
                out = fe.run_cf32(x)
            elif call == "run_u8":
                out = fe.run_u8(x8)
            else:
                out = fe.run_host_windows(np.ascontiguousarray(x), window=16384)[0]
            for c, d in enumerate(out if Cn > 1 else [out]):
                dib[c].append(d)
    d = [np.concatenate(x) if x else np.zeros(0, np.uint8) for x in dib]
    s = [np.concatenate(x) if x else np.zeros(0, np.int64) for x in sps] if call.endswith("+slice") else None
    return d, s


def ragged(n_iq, seed, must_cut, coarse=False):
    """ragged chunks of [0, n_iq) with cuts at every index of must_cut"""
    rng = np.random.default_rng(seed)
    sizes = [] if coarse else [1, 2, 7, 333, 16384, 16385, 40000, 3, 16384]
    cuts, o = [0], 0
    while o < n_iq:
        n = sizes.pop(0) if sizes else int(rng.integers(30000, 60000) if coarse else rng.integers(1, 50000))
        o = min(o + n, n_iq)
        cuts.append(o)
    cuts = sorted(set(cuts + [int(x) for x in must_cut]))
    return [(a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]


@pytest.mark.parametrize("mode", PIECEWISE_MODES, ids=PIECEWISE_IDS)
@pytest.mark.parametrize("call", STREAM_CALLS)
@pytest.mark.parametrize("start", ["fresh", "midstream"])
@pytest.mark.parametrize("bound", BOUNDS, ids=IDS)
def test_stream_reaches_a_large_position_through_the_state_blob(O, FE, c4fm_1s, bound, start, call, mode):
    """A streaming handle moved to a large position through its state blob -- from a fresh handle, and mid-stream while locked --
    then fed ragged chunks across the boundary through every streaming entry point, with a p25fe_resync() and a p25fe_resync_at_dev
    list on the way (p25fe_run_host_windows takes no list: its drops are all p25fe_resync() between calls), and exported /
    re-imported once more after the crossing: the dibits are the oracle's for the unmoved stream, the sync positions the oracle's
    plus the baseband offset, and the header carries the advanced counters."""
    from p25rx_amd import c4fm, _lib
    iq = c4fm_1s[0]
    u8 = c4fm.to_u8(iq)
    if mode == 2:
        # (p25fe_demod_* run no receiver and take any clock; it is the receiver half of each form that refuses)
        fe = FE(symbol_clock=2)
        refusing = {"demod_cf32+slice": lambda: fe.slice(np.zeros(3000, np.float32)), "demod_u8+slice": lambda: fe.slice(np.zeros(3000, np.float32)),
                    "run_cf32": lambda: fe.run_cf32(iq[:16384]), "run_u8": lambda: fe.run_u8(u8[:32768]),
                    "run_host_windows": lambda: fe.run_host_windows(iq[:65536], window=16384)}[call]
        move_stream(fe, 5 * bb_base(bound)[0], bb_base(bound)[0])
        with pytest.raises(_lib.P25feError) as e:
            refusing()
        assert e.value.status == _lib.ERR_ARG
        pytest.skip("symbol_clock = 2 through %s at %s (%s): the streaming receiver calls refuse it by design with P25FE_ERR_ARG "
                    "(checked above); the reslice+causal_ok case runs them" % (call.replace("demod_cf32+", "p25fe_").replace("demod_u8+", "p25fe_"), bound[0], start))
    omode = oracle_mode(mode)
    od = O.Demod()
    bb_ref = od.feed_u8(u8) if call in ("demod_u8+slice", "run_u8") else od.feed_cf32(iq)
    base, edge = bb_base(bound)
    free = oracle_recv(O, bb_ref, omode)
    # the move happens at IQ sample m_iq of the capture (0: a fresh handle; else 65 baseband samples behind a sync word: locked);
    # the capture's baseband sample 0 then sits at absolute index `base`, its IQ sample 0 at 5 * base
    m_iq = 0 if start == "fresh" else 5 * ([int(s) for s in free[1] if int(s) + 65 < K // 2][-1] + 65)
    second_cut = 5 * (K + 9000)                                      # the export / import after the crossing
    q_host = K + 13000                                               # p25fe_resync() here
    local = [K - 2000, K, K + 3000]                                  # lock drops around the power of two
    windows = call == "run_host_windows"
    chunks = ragged(len(iq), 7, [m_iq, second_cut, 5 * q_host] + ([5 * q for q in local] if windows else []), coarse=windows)
    host_at = {5 * q_host} | ({5 * q for q in local} if windows else set())
    dev_drops = [] if windows else [q + base for q in local]
    ref = oracle_recv(O, bb_ref, omode, local + [q_host])
    assert len(ref[0]) < len(free[0])
    part = lambda lo, hi: [(o, n) for o, n in chunks if lo <= o < hi]
    fe = FE(symbol_clock=mode)
    d0, s0 = stream_through(fe, call, iq, u8, part(0, m_iq), 0)
    before, anc = move_stream(fe, 5 * base, base)
    assert before == (m_iq, cnt(0, m_iq, 4, 5)) and bool(int(anc["valid"][0]) & 1) == (start == "midstream")
    d1, s1 = stream_through(fe, call, iq, u8, part(m_iq, second_cut), base, dev_drops, host_at)
    # after the crossing: the header carries the advanced counters; a new handle continues from the blob
    blob = fe.state_export()
    hd = blob_header(blob)
    assert int(hd["abs_iq"]) == 5 * base + second_cut and int(hd["abs_iq"]) > bound[1] * (5 if bound[2] == "bb" else 1)
    assert int(hd["abs_bb"]) == base + cnt(0, second_cut, 4, 5) and int(hd["abs_bb"]) > edge
    fe2 = FE(symbol_clock=mode)
    fe2.state_import(blob)
    d2, s2 = stream_through(fe2, call, iq, u8, part(second_cut, len(iq)), base, dev_drops, host_at)
    got = np.concatenate([d0[0], d1[0], d2[0]])
    assert len(got) == len(ref[0]) and np.array_equal(got, ref[0]), (bound[0], start, call)
    if s0 is not None:
        sp = [int(x) + base for x in s0[0]] + [int(x) for x in s1[0]] + [int(x) for x in s2[0]]
        assert sp == [int(x) + base for x in ref[1]]
        straddles(sp, edge)
    hd2 = blob_header(fe2.state_export())
    assert int(hd2["abs_iq"]) == 5 * base + len(iq) and int(hd2["abs_bb"]) == base + len(bb_ref)


@pytest.mark.parametrize("bound", BOUNDS, ids=IDS)
def test_stream_two_channels_across_the_boundary(O, FE, c4fm_1s, bound):
    """The same move on a two-channel handle (two anchors, two totals in the blob), tracking clock, run_cf32 and demod + slice."""
    from p25rx_amd import c4fm
    mode = 1
    iq = np.stack([c4fm_1s[0], c4fm.synth(1.0, seed=9, snr_db=24.0, timing_offset=13, clock_ppm=60.0)[0]])
    base, edge = bb_base(bound)
    bbs = [O.Demod().feed_cf32(iq[c]) for c in range(2)]
    refs = [oracle_recv(O, bbs[c], mode) for c in range(2)]
    m_iq = 5 * (max(int(refs[c][1][1]) for c in range(2)) + 400)     # both channels locked
    assert m_iq < 5 * K // 2
    chunks = ragged(iq.shape[1], 11, [m_iq])
    k_move = next(k for k, (a, _) in enumerate(chunks) if a == m_iq)
    for call in ("run_cf32", "demod_cf32+slice"):
        fe = FE(n_channels=2, symbol_clock=mode)
        d0, s0 = stream_through(fe, call, iq, iq, chunks[:k_move], 0)
        before, anc = move_stream(fe, 5 * base, base)
        assert all(int(v) & 1 for v in anc["valid"]) and before[0] == m_iq
        d1, s1 = stream_through(fe, call, iq, iq, chunks[k_move:], base)
        for c in range(2):
            got = np.concatenate([d0[c], d1[c]])
            assert len(got) == len(refs[c][0]) and np.array_equal(got, refs[c][0]), (call, c)
            if s0 is not None:
                sp = [int(x) + base for x in s0[c]] + [int(x) for x in s1[c]]
                assert sp == [int(x) + base for x in refs[c][1]]
                straddles(sp, edge)
        hd = blob_header(fe.state_export())
        assert int(hd["abs_iq"]) == 5 * base + iq.shape[1]


# ------------------------------------------------------------------------------------------------------------------------------
# 5. passengers
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bound", BOUNDS, ids=IDS)
def test_nid_and_channel_stats_carry_large_sync_positions(O, FE, bound):
    """p25fe_nid_dev and p25fe_nid_batch_dev return a large sync_pos unchanged in their records (the oracle's records, for the same
    events); p25fe_chan_stats_dev reports last_sync_pos at the large value."""
    import torch
    from p25rx_amd import c4fm
    from p25rx_amd._lib import NID_DTYPE, CHAN_STATS_DTYPE
    nidf = lambda f: ((0x100 + 37 * f) & 0xFFF, (5 * f + 1) & 15)
    Cn = 2
    iqs = [c4fm.synth(1.5, seed=44 + c, snr_db=22.0, frame_dibits=400, nid=nidf)[0] for c in range(Cn)]
    bbs = np.stack([O.Demod().feed_cf32(x) for x in iqs])
    base, edge = bb_base(bound)
    fe = FE(n_channels=Cn)
    t = torch.from_numpy(bbs).cuda()
    cap = 128
    dib, res, sp, sd = fe.slice_dev(t, bbs.shape[1], abs_bb0=base, sync_cap=cap)
    nid = fe.nid_batch_dev(dib, res, sd, sp)
    st = np.frombuffer(fe.chan_stats_dev(res, nid).cpu().numpy().tobytes(), dtype=CHAN_STATS_DTYPE)
    nid_h = nid.cpu().numpy()
    for c in range(Cn):
        ref = oracle_recv(O, bbs[c], 0)
        ns = len(ref[1])
        assert 10 <= ns <= cap
        spl = np.array([int(x) + base for x in ref[1]], dtype=np.int64)
        assert np.array_equal(sp[c, :ns].cpu().numpy(), spl)
        straddles(spl, edge)
        want = O.nid_decode(ref[0], ref[2], spl)
        got = np.frombuffer(nid_h[c, :ns].tobytes(), dtype=NID_DTYPE)
        assert got.tobytes() == want.tobytes() and np.array_equal(got["sync_pos"], spl), c
        assert int((got["valid"] == 1).sum()) >= ns - 2
        one = np.frombuffer(fe.nid_dev(dib[c], len(ref[0]), sd[c, :ns], sp[c, :ns]).cpu().numpy().tobytes(), dtype=NID_DTYPE)
        assert one.tobytes() == want.tobytes(), c
        assert int(st[c]["last_sync_pos"]) == int(spl[-1]) and int(st[c]["n_sync"]) == ns and int(st[c]["locked"]) == 1


# ------------------------------------------------------------------------------------------------------------------------------
# 6. the one bound: P25FE_MAX_POSITION (include/p25fe.h)
# ------------------------------------------------------------------------------------------------------------------------------

def test_positions_are_bounded_by_a_documented_argument_error(O, FE, c4fm_1s, bb_1s, spec):
    """include/p25fe.h: a position of P25FE_MAX_POSITION = 2^62 or more is P25FE_ERR_ARG at every entry point that takes one, and in a
    state blob.  Just below the bound every stage still computes what the oracle computes at the small congruent position -- a
    test on each side, never a silent wrong answer."""
    import torch
    from p25rx_amd import _lib
    from p25rx_amd._lib import P25feError, ERR_ARG
    top = _lib.MAX_POSITION
    assert top == 1 << 62
    iq = c4fm_1s[0][:60000]
    t = cf32_dev(iq)
    fe = FE()
    halo = fe.shard_halo()

    def refused(call):
        with pytest.raises(P25feError) as e:
            call()
        assert e.value.status == ERR_ARG
    # below: the last admissible position, whatever its residues
    P = top - 1
    ref = O.Demod().feed_cf32(np.concatenate([np.zeros(P % 5, np.complex64), iq]))
    bb, nb = fe.demod_dev(t, n_hist=0, abs0=P)
    assert nb == len(ref) == cnt(P, len(iq), 4, 5) and np.array_equal(bits(bb[0, :nb].cpu().numpy()), bits(ref))
    x = iq[:20000]
    y, no = fe.predecim_dev(t[:20000], n_hist=0, abs0=P)
    ref0 = O.PreDecim(spec).feed(np.concatenate([np.zeros(P % 10, np.complex64), x]))
    assert no == len(ref0) and np.array_equal(y[0, :no].cpu().numpy().view(np.uint32), ref0.view(np.float32).reshape(-1, 2).view(np.uint32))
    z, nz = fe.channelise_dev(t[:20000], n_hist=0, abs0=P)
    small = O.channelise(x, abs0=P % 960, spec=spec)
    hsum = float(np.abs(np.array(spec["pre_taps"], dtype=np.float64)).sum())
    assert nz == small.shape[1]
    assert np.abs(z[:, :nz].cpu().numpy().view(np.complex64)[..., 0] - small).max() <= 2e-6 * hsum * float(np.abs(x).max())
    tb = torch.from_numpy(bb_1s).cuda()
    want = oracle_recv(O, bb_1s, 0)
    got = dev_slice(fe, tb, len(bb_1s), P)[0]
    same_shifted(got, want, P, "slice_dev at 2^62 - 1")
    assert int(got[3]["anchor_out"]["s"]) == int(want[1][-1]) + P and int(got[3]["first_event"]) == int(want[1][0]) + 5 + P
    blob = np.array(fe.state_export(), copy=True)
    hd = np.frombuffer(blob[:32].tobytes(), dtype=HDR).copy()
    hd["abs_iq"], hd["abs_bb"] = top - 5, top - 1
    blob[:32] = np.frombuffer(hd.tobytes(), dtype=np.uint8)
    fe.state_import(blob)
    d, sp, _ = fe.slice(bb_1s[:20000])
    ref_s = O.Recv().feed(bb_1s[:20000])
    assert np.array_equal(d, ref_s[0]) and [int(v) for v in sp] == [int(v) + top - 1 for v in ref_s[1]] and len(sp) >= 2
    # at the bound and above it: refused, and nothing is launched
    for pos in (top, top + 1, (1 << 63) - 1, 1 << 63, (1 << 64) - 1):
        refused(lambda: fe.demod_dev(t, n_hist=0, abs0=pos))
        refused(lambda: fe.predecim_dev(t, n_hist=0, abs0=pos))
        refused(lambda: fe.channelise_dev(t, n_hist=0, abs0=pos))
        refused(lambda: fe.slice_dev(tb, len(bb_1s), abs_bb0=pos))
        for form in (fe.shard_pass1_main, fe.shard_pass1_head, fe.shard_pass1_k1):
            refused(lambda: form(t, offset=halo, n_hist=halo, abs0=pos))
        for form in (fe.shard_pass1, fe.shard_pass1_finish):
            refused(lambda: form(t, offset=halo, n_hist=halo, abs0=pos))
    for field in ("abs_iq", "abs_bb"):
        bad = np.array(blob, copy=True)
        hd2 = hd.copy()
        hd2[field] = top
        bad[:32] = np.frombuffer(hd2.tobytes(), dtype=np.uint8)
        refused(lambda: fe.state_import(bad))
    # a valid anchor of a blob is a position too
    fe.reset()
    fe.slice(bb_1s[:20000])
    locked = np.array(fe.state_export(), copy=True)
    lo, anc = blob_anchors(locked, 1)
    assert int(anc["valid"][0]) & 1
    for s_new, ok in ((top - 1, True), (top, False), (-top, False)):
        anc["s"][0] = s_new
        locked[lo:lo + anc.itemsize] = np.frombuffer(anc.tobytes(), dtype=np.uint8)
        if ok:
            fe.state_import(locked)
        else:
            refused(lambda: fe.state_import(locked))
    # the count functions have no bound: exact for every uint64_t
    for pos in (top, (1 << 64) - 7):
        assert fe.L.p25fe_n_baseband(pos, 6) == cnt(pos, 6, 4, 5) and fe.L.p25fe_n_predecim(pos, 6) == cnt(pos, 6, 9, 10)
    torch.cuda.synchronize()
    # ... and the handle is as good as before
    fe.reset()
    bb2, nb2 = fe.demod_dev(t)
    assert np.array_equal(bits(bb2[0, :nb2].cpu().numpy()), bits(O.Demod().feed_cf32(iq)))
