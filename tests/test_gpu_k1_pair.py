"""k_frontend_pair -- the two-wave form of K1 that takes the main part of a cf32 range on the planar scratch -- cell by cell.

Reference: the oracle's LINEAR baseband pushed through the numpy model of the layout (tests/planes_model.py), read back through
p25fe_debug_planes_dev, floats compared as uint32 under the mask of the cells a call defines (tests/test_gpu_planes.py: `check`).
Every case then repeats the call on a handle made with P25FE_K1_PAIR=0 (read once, at p25fe_create: that handle runs the one-wave
k_frontend for every launch): planes under the mask, dibits and p25fe_result_t must be byte-identical.

The pair kernel lays a range out in the prologue form: outputs m in [-(320 + look), n), in segments of 3 sub-tiles = 960 outputs from
there; it runs when the main part of the range holds at least one whole segment.  So a call of n_bb baseband samples has
TOTAL = n_bb + 320 + look outputs, and the lengths are chosen by TOTAL:
  959, 960, 961      the one-wave kernel still / exactly one segment / a second segment of ONE output
  1927               two segments and 7 outputs
  3080               the range ends inside the first sub-tile (200 outputs) of its fourth segment
  n_bb = 7681        two receive tiles
Channels 1 and 3 (padded stride), symbol_clock 0 and 1 (pl_shift 320 and 322).  Entry points: p25fe_run_dev at the start of a
stream (history cells +0.0, bit 0), p25fe_shard_pass1_main + _head + _finish with n_hist > 0 at an odd absolute position and at one
past 2^32 (reference: the oracle at a small position congruent modulo 5, tests/test_gpu_positions.py), and two pipelined calls
enqueued back to back, then joined.

Adversarial capture: -0.0, NaN and infinities of both signs in the last window of segment 0 / the prologue window of segment 1, in
segment 1's first window and in its last.  A sub-tile's ten sign words are written by one store of ten lanes, next to rows written
by 64: the words must be the sign bits of the floats that came back, whatever they are.  Against the oracle the comparison is bit
for bit wherever the oracle's sample is not a NaN; where it is one (an infinity meets the opposite one in a FIR sum, or a NaN sample
passes through) the GPU must hold a NaN too but its sign and payload are the hardware's: x86 makes the default NaN negative, gfx950
positive.  Between the two kernels every bit is compared, NaNs included: they run the same instruction sequence per output."""
import contextlib
import os

import numpy as np
import pytest

import planes_model as PM
from test_gpu_planes import check, dev, iq_len, noise_iq, stream

pytestmark = pytest.mark.gpu

SEG = 960
TOTALS = (959, 960, 961, 2 * SEG + 7, 3 * SEG + 200)


def lengths(look):
    return [t - PM.PLPAD - look for t in TOTALS] + [7681]


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def FE():
    from p25rx_amd.frontend import FrontEnd
    return FrontEnd


@contextlib.contextmanager
def one_wave_kernel():
    """handles created inside run k_frontend everywhere"""
    old = os.environ.get("P25FE_K1_PAIR")
    os.environ["P25FE_K1_PAIR"] = "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["P25FE_K1_PAIR"]
        else:
            os.environ["P25FE_K1_PAIR"] = old


def same_planes(pa, pb, bbs, hists, look, what):
    for c in range(len(bbs)):
        _, _, fmask, wmask = PM.expect(bbs[c], hists[c], look)
        fa, fb = pa[0][c].view(np.uint32), pb[0][c].view(np.uint32)
        wa, wb = pa[1][c].view(np.uint32), pb[1][c].view(np.uint32)
        assert np.array_equal(fa[fmask], fb[fmask]), (what, c, "floats differ between the kernels")
        assert np.array_equal(wa & wmask, wb & wmask), (what, c, "sign words differ between the kernels")


def same_outputs(a, b, C, what):
    from p25rx_amd.frontend import parse_results
    (da, ra), (db, rb) = a, b
    ra, rb = ra.cpu().numpy(), rb.cpu().numpy()
    assert ra.tobytes() == rb.tobytes(), (what, "p25fe_result_t differs")
    for c, r in enumerate(parse_results(a[1])):
        n = int(r["n_dibits"])
        assert np.array_equal(da[c, :n].cpu().numpy(), db[c, :n].cpu().numpy()), (what, c, "dibits differ")


def channels_tensor(O, C, n, seed0):
    """C streams of n IQ samples ([n, 2] for one channel, [C, n, 2] with a padded stride whose padding holds loud samples)"""
    st = [stream(O, "cf32", seed0 + c) for c in range(C)]
    if C == 1:
        return dev(st[0][0][:n]), st
    stride = (n + 7) // 8 * 8 + 24
    buf = dev(np.stack([stream(O, "cf32", seed0 - 10 - c)[0][:stride] for c in range(C)]))
    for c in range(C):
        buf[c, :n] = dev(st[c][0][:n])
    return buf[:, :n], st


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("clock", [0, 1])
def test_run_dev_at_the_start_of_a_stream(O, FE, clock, C):
    look = PM.look_of(clock)
    fe = FE(n_channels=C, symbol_clock=clock)
    with one_wave_kernel():
        fo = FE(n_channels=C, symbol_clock=clock)
    for n_bb in lengths(look):
        n = 5 * n_bb + n_bb % 5
        t, st = channels_tensor(O, C, n, 100)
        assert fe.n_baseband(0, n) == n_bb
        what = "run_dev clock %d C %d n_bb %d" % (clock, C, n_bb)
        bbs, hists = [s[1][:n_bb] for s in st], [PM.history(None, look)] * C
        a = fe.run_dev(t)
        pa = check(fe, n_bb, bbs, hists, look, what)
        b = fo.run_dev(t)
        pb = check(fo, n_bb, bbs, hists, look, what + " (one-wave kernel)")
        same_planes(pa, pb, bbs, hists, look, what)
        same_outputs(a, b, C, what)


def local_start(halo, abs0):
    """a small stream index congruent to abs0 modulo 5 with the halo in front of it"""
    a = halo + 40
    while a % 5 != abs0 % 5:
        a += 1
    return a


@pytest.mark.parametrize("clock", [0, 1])
@pytest.mark.parametrize("abs0", [None, (1 << 32) + 1], ids=["odd", "past2e32"])
def test_shard_main_head_finish_with_history(O, FE, abs0, clock):
    """n_hist = the shard halo.  The head (two lead segments = positions [0, 640)) runs on k_frontend, the main launch on the pair
    kernel; `odd`: abs0 = halo + 43."""
    look = PM.look_of(clock)
    fe = FE(symbol_clock=clock)
    with one_wave_kernel():
        fo = FE(symbol_clock=clock)
    halo = fe.shard_halo()
    rows, bb_all = stream(O, "cf32", 33)
    if abs0 is None:
        abs0 = halo + 43
        assert abs0 % 2 == 1
    a0 = local_start(halo, abs0)
    for n_bb in (TOTALS[2] + 640 - PM.PLPAD - look, 2881, 7681):        # (961 outputs behind the head; the planes test's; two tiles)
        n = iq_len(n_bb, a0, 2)
        assert a0 + n <= len(rows) and fe.n_baseband(abs0, n) == n_bb and fe.n_baseband(a0, n) == n_bb
        nb0 = fe.n_baseband(0, a0)
        t, bb, hist = dev(rows[a0 - halo:a0 + n]), bb_all[nb0:nb0 + n_bb], PM.history(bb_all[:nb0], look)
        what = "shard main + head clock %d abs0 %d n_bb %d" % (clock, abs0, n_bb)
        out = []
        for h, tag in ((fe, ""), (fo, " (one-wave kernel)")):
            h.shard_pass1_main(t, halo, halo, abs0)
            h.shard_pass1_head(t, halo, halo, abs0)
            p = check(h, n_bb, [bb], [hist], look, what + tag)
            r = h.shard_pass1_finish(t, halo, halo, abs0).cpu().numpy()
            h.shard_head_check()
            out.append((p, r))
        same_planes(out[0][0], out[1][0], [bb], [hist], look, what)
        assert out[0][1].tobytes() == out[1][1].tobytes(), (what, "p25fe_result_t differs")


@pytest.mark.parametrize("clock", [0, 1])
def test_two_pipelined_calls_back_to_back(O, FE, clock):
    import torch
    look = PM.look_of(clock)
    rows, bb = stream(O, "cf32", 41)
    rows2, bb2 = stream(O, "cf32", 42)
    na, nb = 7680, 2 * SEG + 7 - PM.PLPAD - look
    ta, tb = dev(rows[:5 * na]), dev(rows2[:5 * nb + 2])
    res = []
    for tag in ("", " (one-wave kernel)"):
        with (one_wave_kernel() if tag else contextlib.nullcontext()):
            fe = FE(symbol_clock=clock)
        ra = fe.run_dev_pipelined(ta)
        rb = fe.run_dev_pipelined(tb)
        fe.join_dev()
        p = check(fe, nb, [bb2[:nb]], [PM.history(None, look)], look, "pipelined, two deep, joined, clock %d%s" % (clock, tag))
        torch.cuda.synchronize()
        res.append((ra, rb, p))
    same_planes(res[0][2], res[1][2], [bb2[:nb]], [PM.history(None, look)], look, "pipelined")
    same_outputs(res[0][0], res[1][0], 1, "pipelined, first call")
    same_outputs(res[0][1], res[1][1], 1, "pipelined, second call")


def test_adversarial_samples_at_segment_edges(O, FE):
    look = 0
    n_bb = 2 * SEG + 7 - PM.PLPAD
    iq = noise_iq(77, 5 * n_bb + 3).copy()
    u = iq.view(np.uint32)                                               # [re, im] pairs
    seg1 = 5 * (SEG - PM.PLPAD)                                          # input index of segment 1's first output (m = 640)
    seg2 = 5 * (2 * SEG - PM.PLPAD)
    specials = [0x80000000, 0x7fc00000, 0x7f800000, 0xff800000, 0xffc00001, 0x80000000]
    for base in (seg1 - 160, seg1 + 60, seg2 - 700):                    # prologue window of segment 1 = last window of segment 0; first; last window
        for j, s in enumerate(specials):
            u[2 * (base + 37 * j) + (j & 1)] = s
    ref = O.Demod().feed_cf32(iq)
    assert len(ref) == n_bb
    nan = np.isnan(ref)
    assert nan.any()
    t = dev(iq.view(np.float32).reshape(-1, 2))
    fe = FE()
    with one_wave_kernel():
        fo = FE()
    hist = PM.history(None, look)
    ef, ew, fmask, wmask = PM.expect(ref, hist, look)
    fi, wi, bit = PM.cell(np.arange(n_bb, dtype=np.int64), look)
    planes = []
    for h in (fe, fo):
        h.run_dev(t)
        f, w = h.debug_planes(n_bb)
        f, w = f.cpu().numpy()[0].view(np.uint32), w.cpu().numpy()[0].view(np.uint32)
        got = f[fi]
        assert np.array_equal(got[~nan], ref.view(np.uint32)[~nan]), "a sample that is no NaN differs from the oracle"
        assert np.isnan(got.view(np.float32)[nan]).all(), "the oracle's NaNs are NaNs"
        hm = np.arange(-len(hist), 0, dtype=np.int64)
        assert not f[PM.cell(hm, look)[0]].any(), "history cells are +0.0"
        own = PM.words_of_floats(f)
        assert not ((w ^ own) & wmask).any(), "a sign word disagrees with the signs of its own floats"
        planes.append((f, w))
    assert np.array_equal(planes[0][0][fmask], planes[1][0][fmask]) and np.array_equal(planes[0][1] & wmask, planes[1][1] & wmask)
