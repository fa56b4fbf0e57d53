"""K1's planar output -- the blocked polyphase baseband (`pl_f`) and its sign words (`pl_bits`) in the handle's scratch -- cell by
cell against the oracle, through the diagnostic read-out p25fe_debug_planes_dev (FrontEnd.debug_planes).

The reference is always the oracle's LINEAR baseband (O.Demod().feed_*) pushed through the numpy model of the layout
(tests/planes_model.py, written from the comment at PLPAD in p25fe_kernels.hip); never another GPU kernel.  Floats are compared as
uint32, there is no tolerance, and only the cells a call DEFINES are compared: samples m in [-hist, n) of its range, hist =
min(available history, HIST_BB + look), at position m + 320 + look.  A failure names channel, block, plane, symbol and both bit
patterns of the first few cells (planes_model.diff_report).  After every comparison the sign words under the mask must also equal the
sign bits of the floats that came back from the GPU (the same function): independent of the oracle, it catches a word store that
lags behind its rows.

Input is seeded Gaussian IQ at an amplitude of 0.3: every baseband sample has a random sign, so every sign word is non-trivial.
Baseband lengths LENGTHS: 1, 7 and n - 1, n, n + 1 around 80 (a sign byte of the halo form), 240, 320 (a sub-tile = a block), 880
(the cf32 segment), 2880 (the u8 / s16 segment), 7680 (a tile).

case                                        mask rule (the cells compared)
------------------------------------------  ---------------------------------------------------------------------------------
run_dev, first call (cf32 / u8 / s16,       m in [-(240 + look), n); the history is the zeros in front of a stream: +0.0, bit 0.
  clocks 0 / 1, C = 1 and C = 3 padded)     (The prologue form also writes m in [-(320 + look), -(240 + look)): not compared.)
kernel variants (built-in, generic 31 / 41  the same
  and 64 / 64, hipRTC with tables and
  with the build's numbers; cf32, u8)
run_dev again on a used handle              the same: p25fe_run_dev always starts a stream (include/p25fe.h), so the history cells
                                            are zeros again and must not keep the earlier call's samples
shard_pass1_k1, shard_pass1 with n_hist > 0 m in [-(240 + look), n); history = the stream's previous 240 + look baseband samples,
  every decimator phase abs0 % 5            recomputed by K1 from the IQ history (zeros where the stream starts inside them)
shard_pass1_main + _head  vs  shard_pass1   the same mask for both handles, each against the model and against each other
run_dev_pipelined (+ join_dev)              as run_dev; read from the scratch set the LAST call used
run_cf32 / run_u8 / run_s16, three chunks   m in [-(240 + look), n) per chunk; history from the handle's IQ history
slice(), chunk of at most a tile            every cell of symbols < n_sym of k_recv_chunk's loop: the defined ones as above, all
                                            others +0.0 / bit 0
slice_dev with adversarial floats           EVERY cell of the scratch: k_planarize writes all blocks; m in [-hist, n) with hist =
                                            min(n_hist_bb, 240 + look) bit for bit (NaN payloads, -0.0, denormals), the rest +0.0
short calls after a loud one (part 4)       m in [-(240 + look), n) of every short call; and the receiver's outputs
"""
import numpy as np
import pytest

import planes_model as PM

pytestmark = pytest.mark.gpu

LENGTHS = sorted({1, 7} | {b + d for b in (80, 240, 320, 880, 2880, 7680) for d in (-1, 0, 1)})
FMTS = ["cf32", "u8", "s16"]
N_STREAM = 2560 + 64 + 5 * 7681 + 16                                 # IQ samples of a test stream: a shard halo, a largest range
SPECIALS = np.array([0x80000000, 0x00000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x7f800000, 0xff800000, 0x7fc00000,
                     0xffc00000, 0xff800001, 0x7fa00000, 0xffffffff, 0x7fffffff], dtype=np.uint32)


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def lib():
    from p25rx_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def FE():
    from p25rx_amd.frontend import FrontEnd
    return FrontEnd


def noise_iq(seed, n=N_STREAM):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (0.3 / np.sqrt(2.0))).astype(np.complex64)


def in_format(O, iq, fmt, ocfg=None):
    """complex64 -> (the samples as the [n, 2] array the device calls take, the oracle's baseband of exactly those samples)"""
    from p25rx_amd import c4fm
    if fmt == "cf32":
        return iq.view(np.float32).reshape(-1, 2), O.Demod(ocfg).feed_cf32(iq)
    if fmt == "u8":
        b = c4fm.to_u8(iq)
        return b.reshape(-1, 2), O.Demod(ocfg).feed_u8(b)
    s = c4fm.to_s16(iq)
    return s.reshape(-1, 2), O.Demod(ocfg).feed_cf32((s.astype(np.float32) * np.float32(2.0 ** -15)).view(np.complex64))


_streams = {}


def stream(O, fmt, seed):
    """(rows [N_STREAM, 2], baseband of the whole stream): computed once per format and seed, shared, never written"""
    key = (fmt, seed)
    if key not in _streams:
        rows, bb = in_format(O, noise_iq(seed), fmt)
        rows.setflags(write=False)
        bb.setflags(write=False)
        _streams[key] = (rows, bb)
    return _streams[key]


def iq_len(n_bb, abs0, extra=0):
    """IQ samples from absolute index abs0 that give n_bb baseband samples (decimator phase 4), plus up to 4 that give none"""
    o0 = (4 + 5 - abs0 % 5) % 5
    return o0 + 5 * (n_bb - 1) + 1 + extra % 5


def dev(rows):
    import torch
    return torch.from_numpy(np.array(rows)).cuda()                   # (a copy: the shared streams are read-only)


def check(fe, n_bb, bbs, hists, look, what, widen=None):
    """the planes of the handle's last call against the model, channel by channel; `widen`(exp) may extend the masks"""
    f, w = fe.debug_planes(n_bb)
    f, w = f.cpu().numpy(), w.cpu().numpy()
    assert (f.shape[1], w.shape[1]) == PM.geometry(n_bb), (what, f.shape, w.shape)
    for c in range(fe.C):
        exp = PM.expect(bbs[c], hists[c], look)
        if widen is not None:
            widen(exp)
        msg = PM.diff_report(f[c], w[c], exp, look, "%s, n_bb %d, channel %d" % (what, n_bb, c))
        assert msg is None, msg
    return f, w


def shuffled(seq, seed):
    return [seq[k] for k in np.random.default_rng(seed).permutation(len(seq))]


# ---- the read-out itself ------------------------------------------------------------------------------------------------------
def test_debug_planes_refusals_and_sizes(O, FE, lib):
    """no call yet, a geometry that is not the last call's, short strides and null pointers are argument errors; the size query is
    the model's geometry; a length of the same geometry is accepted"""
    import ctypes as C
    import torch
    fe = FE()
    for n in (0, 1, 7680, 7681, 15360, 15361, 100000):
        nf, nw = C.c_size_t(0), C.c_size_t(0)
        assert fe.L.p25fe_debug_planes_size(fe.h, n, C.byref(nf), C.byref(nw)) == lib.OK and (nf.value, nw.value) == PM.geometry(n)
    assert fe.L.p25fe_debug_planes_size(fe.h, 1, None, None) == lib.ERR_ARG
    nf, nw = PM.geometry(881)
    f = torch.zeros(nf, dtype=torch.float32, device="cuda")
    w = torch.zeros(nw, dtype=torch.int32, device="cuda")
    pf, pw, st = C.c_void_p(f.data_ptr()), C.c_void_p(w.data_ptr()), fe._stream()
    assert fe.L.p25fe_debug_planes_dev(fe.h, 881, pf, nf, pw, nw, st) == lib.ERR_ARG          # nothing has used the scratch yet
    rows, bb = stream(O, "cf32", 1)
    fe.run_dev(dev(rows[:5 * 881]))
    assert fe.L.p25fe_debug_planes_dev(fe.h, 7681, pf, 1 << 20, pw, 1 << 20, st) == lib.ERR_ARG   # two tiles: not what the call sized
    assert fe.L.p25fe_debug_planes_dev(fe.h, 881, pf, nf - 1, pw, nw, st) == lib.ERR_ARG
    assert fe.L.p25fe_debug_planes_dev(fe.h, 881, pf, nf, pw, nw - 1, st) == lib.ERR_ARG
    assert fe.L.p25fe_debug_planes_dev(fe.h, 881, None, nf, pw, nw, st) == lib.ERR_ARG
    assert fe.L.p25fe_debug_planes_dev(fe.h, 881, pf, nf, None, nw, st) == lib.ERR_ARG
    torch.cuda.synchronize()
    assert not f.any() and not w.any()
    assert fe.L.p25fe_debug_planes_dev(fe.h, 100, pf, nf, pw, nw, st) == lib.OK               # one tile like 881
    check(fe, 881, [bb[:881]], [PM.history(None, 0)], 0, "after the refusals")


# ---- run_dev, first call --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("clock", [0, 1])
@pytest.mark.parametrize("fmt", FMTS)
def test_run_dev_first_call(O, FE, fmt, clock, C):
    """a fresh handle per length: halo form (cf32) and prologue form (u8, s16) of the segment, pl_shift 320 and 322, one channel and
    three with a padded channel stride (whose padding holds loud samples)"""
    import torch
    look = PM.look_of(clock)
    st = [stream(O, fmt, 100 + c) for c in range(C)]
    for n_bb in LENGTHS:
        n = 5 * n_bb + n_bb % 5
        if C == 1:
            t = dev(st[0][0][:n])
        else:
            stride = (n + 7) // 8 * 8 + 24
            buf = dev(np.stack([stream(O, fmt, 90 - c)[0][:stride] for c in range(C)]))
            for c in range(C):
                buf[c, :n] = dev(st[c][0][:n])
            t = buf[:, :n]
        fe = FE(n_channels=C, symbol_clock=clock)
        assert fe.n_baseband(0, n) == n_bb
        fe.run_dev(t)
        check(fe, n_bb, [s[1][:n_bb] for s in st], [PM.history(None, look)] * C, look, "run_dev %s clock %d C %d" % (fmt, clock, C))
        fe.close()


def rand_taps(rng, n):
    return (rng.standard_normal(n) * np.hanning(n + 2)[1:-1] / 6).astype(np.float32).tolist()


@pytest.mark.parametrize("variant", ["builtin", "generic", "generic_long", "jit_tables", "jit_default"])
def test_kernel_variants(O, FE, lib, variant):
    """the built-in constants, the generic kernels with random 31 / 41 and 64 / 64 tables, and the hipRTC kernels (forced the way
    tests/test_gpu_spec.py forces them, with its tables: one cache entry): cf32 and u8 at three lengths, both clocks"""
    if variant in ("generic", "jit_tables"):
        rng = np.random.default_rng(500 + 31)
        tabs = dict(decim_taps=rand_taps(rng, 31), chan_taps=rand_taps(rng, 41))
    elif variant == "generic_long":
        rng = np.random.default_rng(500 + 64)
        tabs = dict(decim_taps=rand_taps(rng, 64), chan_taps=rand_taps(rng, 64))
    else:
        tabs = {}
    kw = dict(tabs)
    if variant in ("generic", "generic_long"):
        kw["specialize"], want = lib.SPECIALIZE_OFF, lib.VARIANT_GENERIC
    elif variant == "jit_tables":
        kw["specialize"], want = lib.SPECIALIZE_REQUIRE, lib.VARIANT_SPECIALIZED
    elif variant == "jit_default":
        kw["specialize"], want = lib.SPECIALIZE_FORCE, lib.VARIANT_SPECIALIZED
    else:
        want = lib.VARIANT_BUILTIN
    ocfg = O.make_config(O.load_spec(), **tabs)
    iq = noise_iq(7, 5 * 7681 + 8)
    for clock in (0, 1):
        look = PM.look_of(clock)
        fe = FE(symbol_clock=clock, **kw)
        assert fe.kernel_variant == want, (fe.kernel_variant, want, lib.specialize_log()[-500:])
        for fmt in ("cf32", "u8"):
            rows, bb = in_format(O, iq, fmt, ocfg)
            for n_bb in (7681, 881, 2879):
                fe.run_dev(dev(rows[:5 * n_bb + 3]))
                check(fe, n_bb, [bb[:n_bb]], [PM.history(None, look)], look, "%s %s clock %d" % (variant, fmt, clock))
        fe.close()


# ---- continuation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clock", [0, 1])
@pytest.mark.parametrize("fmt", FMTS)
def test_run_dev_again_starts_a_stream_again(O, FE, fmt, clock):
    """p25fe_run_dev is "from a fresh stream state" (include/p25fe.h): it has no history argument, so a second call on the handle does
    NOT continue the first.  Its history cells are the zeros in front of a stream again -- not the loud samples the longer first call
    left at those positions and behind the new range's end."""
    look = PM.look_of(clock)
    rows_a = stream(O, fmt, 21)[0]
    rows_b, bb_b = stream(O, fmt, 22)
    fe = FE(symbol_clock=clock)
    fe.run_dev(dev(rows_a[:5 * 7681]))
    for n_bb in (2881, 7679, 321, 79, 880, 1):
        fe.run_dev(dev(rows_b[:5 * n_bb + 4]))
        check(fe, n_bb, [bb_b[:n_bb]], [PM.history(None, look)], look, "second run_dev %s clock %d" % (fmt, clock))


def shard_case(O, fe, fmt, seed, abs0, n_hist, n_bb, extra):
    """the range of n_bb baseband samples that starts at IQ index abs0 of a stream, with n_hist samples of it in front:
    (device rows [n_hist + n, 2], its baseband, its history with the stream's start in front)"""
    rows, bb = stream(O, fmt, seed)
    n = iq_len(n_bb, abs0, extra)
    assert abs0 + n <= len(rows) and fe.n_baseband(abs0, n) == n_bb
    nb0 = fe.n_baseband(0, abs0)
    return dev(rows[abs0 - n_hist:abs0 + n]), bb[nb0:nb0 + n_bb], bb[:nb0]


@pytest.mark.parametrize("clock", [0, 1])
@pytest.mark.parametrize("fmt", FMTS)
def test_shard_k1_history_recomputed_from_the_iq_halo(O, FE, fmt, clock):
    """p25fe_shard_pass1_k1 on one handle, the lengths in a shuffled order, every decimator phase: the history cells hold the
    stream's previous 240 + look baseband samples, which K1 recomputes from the IQ halo.  Then ranges that start 8 .. 40 samples
    into the stream (n_hist = abs0): a few real samples behind the zeros of the stream's start."""
    look = PM.look_of(clock)
    fe = FE(symbol_clock=clock)
    halo = fe.shard_halo()
    for k, n_bb in enumerate(shuffled(LENGTHS, 3)):
        for ph in range(5):
            abs0 = halo + 40 + ph + 5 * (k % 3)
            t, bb, prev = shard_case(O, fe, fmt, 31, abs0, halo, n_bb, n_bb + ph)
            fe.shard_pass1_k1(t, halo, halo, abs0)
            check(fe, n_bb, [bb], [PM.history(prev, look)], look, "shard_pass1_k1 %s clock %d abs0 %d" % (fmt, clock, abs0))
    for abs0 in (8, 16, 24, 32, 40):                                 # (n_hist = abs0 keeps the first owned sample 16-byte aligned)
        for n_bb in (879, 1, 2881):
            t, bb, prev = shard_case(O, fe, fmt, 31, abs0, abs0, n_bb, abs0)
            assert len(prev) == abs0 // 5
            fe.shard_pass1_k1(t, abs0, abs0, abs0)
            check(fe, n_bb, [bb], [PM.history(prev, look)], look, "shard_pass1_k1 %s clock %d abs0 %d" % (fmt, clock, abs0))


@pytest.mark.parametrize("clock", [0, 1])
@pytest.mark.parametrize("fmt", FMTS)
def test_shard_pass1_with_history_at_odd_positions(O, FE, fmt, clock):
    """the whole p25fe_shard_pass1 (K1, detection, scan) with n_hist > 0 at positions that are no multiple of 5"""
    look = PM.look_of(clock)
    fe = FE(symbol_clock=clock)
    halo = fe.shard_halo()
    for k, n_bb in enumerate((7681, 319, 2880, 81, 881, 7)):
        abs0 = halo + 11 + k % 4 + (1 if (halo + 11 + k % 4) % 5 == 0 else 0)
        assert abs0 % 5 != 0
        t, bb, prev = shard_case(O, fe, fmt, 32, abs0, halo, n_bb, k)
        fe.shard_pass1(t, halo, halo, abs0)
        check(fe, n_bb, [bb], [PM.history(prev, look)], look, "shard_pass1 %s clock %d abs0 %d" % (fmt, clock, abs0))


@pytest.mark.parametrize("n_bb", [100, 2881])
@pytest.mark.parametrize("fmt", FMTS)
def test_shard_main_then_head_equals_one_pass(O, FE, fmt, n_bb):
    """p25fe_shard_pass1_main, then p25fe_shard_pass1_head on the same range (the head's lead segments of one sub-tile each:
    SegGeo::set_lead) leave the planes of one p25fe_shard_pass1; both equal the model.  The head is the segments whose input
    reaches in front of the owned samples.  n_bb = 100: all of the range is head, which ends inside block 1 (position 420 + look).
    n_bb = 2881: the halo form's head (cf32) is two lead segments of 240 and ends inside a block (position 560 + look), the
    prologue form's (u8, s16) two of 320 and ends on the boundary of blocks 1 and 2 (position 640)."""
    for clock in (0, 1):
        look = PM.look_of(clock)
        fa, fb = FE(symbol_clock=clock), FE(symbol_clock=clock)
        halo = fa.shard_halo()
        abs0 = halo + 43
        t, bb, prev = shard_case(O, fa, fmt, 33, abs0, halo, n_bb, 2)
        hist = PM.history(prev, look)
        fa.shard_pass1_main(t, halo, halo, abs0)
        fa.shard_pass1_head(t, halo, halo, abs0)
        pa = check(fa, n_bb, [bb], [hist], look, "main + head %s clock %d" % (fmt, clock))
        ra = fa.shard_pass1_finish(t, halo, halo, abs0).cpu().numpy()
        fa.shard_head_check()
        rb = fb.shard_pass1(t, halo, halo, abs0).cpu().numpy()
        pb = check(fb, n_bb, [bb], [hist], look, "one pass %s clock %d" % (fmt, clock))
        _, _, fmask, wmask = PM.expect(bb, hist, look)
        assert np.array_equal(pa[0][0].view(np.uint32)[fmask], pb[0][0].view(np.uint32)[fmask])
        assert np.array_equal(pa[1][0].view(np.uint32) & wmask, pb[1][0].view(np.uint32) & wmask)
        assert np.array_equal(ra, rb)


def test_run_dev_pipelined_reads_the_set_the_last_call_used(O, FE):
    """p25fe_run_dev_pipelined moves through the scratch sets: after each call of a sequence, and after two calls enqueued back to
    back and joined, the read-out is the LAST call's planes"""
    import torch
    for fmt, clock in (("cf32", 0), ("u8", 1), ("s16", 0)):
        look = PM.look_of(clock)
        rows, bb = stream(O, fmt, 41)
        rows2, bb2 = stream(O, fmt, 42)
        fe = FE(symbol_clock=clock)
        for k, n_bb in enumerate((7681, 2881, 881, 7679, 319)):
            r, b = (rows, bb) if k % 2 == 0 else (rows2, bb2)
            fe.run_dev_pipelined(dev(r[:5 * n_bb]))
            check(fe, n_bb, [b[:n_bb]], [PM.history(None, look)], look, "pipelined call %d %s" % (k, fmt))
        ta, tb = dev(rows[:5 * 7680]), dev(rows2[:5 * 2879 + 2])
        fe.run_dev_pipelined(ta)
        fe.run_dev_pipelined(tb)
        fe.join_dev()
        check(fe, 2879, [bb2[:2879]], [PM.history(None, look)], look, "pipelined, two deep, joined %s" % fmt)
        torch.cuda.synchronize()


# ---- the chunk path -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clock", [0, 1])
@pytest.mark.parametrize("fmt", FMTS)
def test_chunk_calls_three_consecutive_chunks(O, FE, fmt, clock):
    """p25fe_run_cf32 / _u8 / _s16 with chunks of at most one tile (the fixed clock runs k_chunk, one launch; the tracking clock
    K1 and the receive chain): after each of three consecutive chunks the history cells are the stream's previous samples,
    recomputed from the handle's IQ history; the chunk sizes walk the decimator's phase"""
    look = PM.look_of(clock)
    rows, bb = stream(O, fmt, 51)
    fe = FE(symbol_clock=clock)
    o = 0
    for n in (16384, 1603, 38397):
        n_bb = fe.n_baseband(o, n)
        assert 0 < n_bb <= PM.TILE
        part = np.ascontiguousarray(rows[o:o + n])
        if fmt == "cf32":
            fe.run_cf32(part.view(np.complex64).reshape(-1))
        elif fmt == "u8":
            fe.run_u8(part.reshape(-1))
        else:
            fe.run_s16(part.reshape(-1))
        nb0 = fe.n_baseband(0, o)
        check(fe, n_bb, [bb[nb0:nb0 + n_bb]], [PM.history(bb[:nb0], look)], look, "chunk at %d %s clock %d" % (o, fmt, clock))
        o += n


def test_slice_chunk_writes_zeros_behind_the_range(O, FE):
    """p25fe_slice with chunks of at most a tile runs k_recv_chunk, whose own loop planarises [tail | new]: whole strides of 64
    symbols, n_sym = the symbols of n + 320 positions rounded up to 64 (at most the scratch).  Every cell of those symbols is
    asserted: the defined ones against the model, all others (in front of the history, behind the range) +0.0 with bit 0 -- also
    where a longer earlier chunk left data."""
    sizes = (7680, 500, 777, 63, 1, 3000)
    bb = in_format(O, noise_iq(61, 5 * sum(sizes)), "cf32")[1]
    assert len(bb) == sum(sizes)
    fe = FE()
    o = 0
    for n in sizes:
        fe.slice(bb[o:o + n])
        n_sym = min((-(-(n + PM.PLPAD) // PM.SPS) + 63) // 64 * 64, PM.geometry(n)[0] // PM.SPS)

        def widen(exp, n_sym=n_sym):
            exp[2][:n_sym // 32 * PM.BLK] = True
            exp[3][:n_sym // 32 * PM.SPS] = 0xffffffff
        check(fe, n, [bb[o:o + n]], [PM.history(bb[:o], 0)], 0, "slice chunk at %d" % o, widen)
        o += n


# ---- k_planarize --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_hist_bb", [0, 1, 239, 240, 241, 500])
@pytest.mark.parametrize("clock", [0, 1])
def test_planarize_adversarial_floats(FE, clock, n_hist_bb):
    """p25fe_slice_dev on a linear baseband the test builds: -0.0, +0.0, denormals, infinities and NaNs of both signs and several
    payloads at m = 0, n - 1, -hist, on both sides of the block / word edges and of the sign bytes, and sprinkled over the rest.
    Floats come back with identical bit patterns, words are the raw sign bits, and every other cell of the scratch is +0.0 / bit 0
    (k_planarize writes all blocks)."""
    look = PM.look_of(clock)
    hist = min(n_hist_bb, PM.HIST_BB + look)
    fe = FE(symbol_clock=clock)
    for n in (7681, 321, 80):
        rng = np.random.default_rng(10000 * clock + 10 * n_hist_bb + n)
        off = 504
        u = (rng.standard_normal(off + n + 8) * 0.5).astype(np.float32).view(np.uint32).copy()
        k = rng.integers(0, len(u), size=len(u) // 25)
        u[k] = SPECIALS[rng.integers(0, len(SPECIALS), size=len(k))]
        edges = [0, 1, n - 1, n - 2, -hist, -hist + 1, -1]
        for p in (80, 160, 320, 640, 960):                           # byte, block and word edges, in positions
            edges += [p - look - PM.PLPAD + d for d in range(-10, 10)]
        for j, m in enumerate(e for e in edges if -hist <= e < n):
            u[off + m] = SPECIALS[j % len(SPECIALS)]
        u[off + n:] = 0xffc00000                                     # behind the range: must not be read
        u[:off - hist] = 0xff800000                                  # in front of the history the call may use: neither
        buf = u.view(np.float32)
        fe.slice_dev(dev(buf), n, n_hist_bb=n_hist_bb, offset=off)

        def widen(exp):
            exp[2][:] = True
            exp[3][:] = 0xffffffff
        check(fe, n, [buf[off:off + n]], [buf[off - hist:off]], look, "slice_dev clock %d n_hist_bb %d" % (clock, n_hist_bb), widen)


# ---- part 4: what a call leaves unwritten is not read -------------------------------------------------------------------------------
_c4fm = {}


def c4fm_stream(O, fmt, which):
    """a strong capture with many sync words ("loud": two tiles + 500 baseband samples) and another seed's ("quiet": the longest
    LENGTHS entry), as rows and oracle baseband"""
    from p25rx_amd import c4fm
    key = (fmt, which)
    if key not in _c4fm:
        if which == "loud":
            iq = c4fm.synth(0.34, seed=11, snr_db=30.0, frame_dibits=150)[0][:5 * (2 * 7680 + 500)]
        else:
            iq = c4fm.synth(0.17, seed=12, snr_db=20.0, frame_dibits=230, timing_offset=3)[0][:5 * 7681]
        _c4fm[key] = in_format(O, iq, fmt)
    return _c4fm[key]


def oracle_receiver(O, bb, clock):
    """(dibits, sync_pos, sync_dibit, final state or None) of the oracle's receiver over a range from a fresh stream"""
    cfg = O.make_config(symbol_clock=clock)
    if clock == 0:
        r = O.Recv(cfg)
        d, sp, sd = r.feed(bb)
        return d, sp, sd, r.state()
    d, sp, sd = O.recv_range(bb, cfg)
    return d, sp, sd, None


def same_receiver_outputs(got, fresh, ref, what):
    """got / fresh: (dibit row, result record[, sync_pos row, sync_dibit row]) of the used and of a fresh handle; ref: the oracle's"""
    d, sp, sd, st = ref
    for name, x in (("used handle", got), ("fresh handle", fresh)):
        r = x[1]
        assert int(r["n_dibits"]) == len(d) and int(r["n_sync"]) == len(sp), (what, name, int(r["n_dibits"]), len(d), int(r["n_sync"]), len(sp))
        assert np.array_equal(x[0][:len(d)], d), (what, name, "dibits")
        if len(x) > 2:
            assert np.array_equal(x[2][:len(sp)], sp), (what, name, "sync_pos")
            assert np.array_equal(x[3][:len(sp)].astype(np.uint64), sd.astype(np.uint64)), (what, name, "sync_dibit")
        if st is not None:                                           # fixed clock: the oracle's lock is the anchor
            a = r["anchor_out"]
            assert bool(int(a["valid"])) == st["valid"], (what, name)
            if st["valid"]:
                assert int(a["s"]) == st["s"] and [np.float32(a[k]) for k in ("hi", "mid", "lo")] == [np.float32(st[k]) for k in ("hi", "mid", "lo")], (what, name)
    # (tracking clocks: the oracle does not export its clock; the used handle's whole record must be the fresh handle's)
    assert got[1].tobytes() == fresh[1].tobytes(), (what, got[1], fresh[1])


@pytest.mark.parametrize("clock", [0, 1, 2])
@pytest.mark.parametrize("fmt", FMTS)
def test_short_run_dev_calls_after_a_loud_one(O, FE, fmt, clock):
    """One handle: a loud call (strong C4FM with a sync word every 150 dibits over two tiles + 500 samples) fills the scratch, then
    another capture at descending lengths.  K1 leaves floats and sign bits past n_out unwritten: they now hold sync-like data.
    Every short call's dibits, counts and anchor_out equal the oracle's and a fresh handle's, and its planes equal the model
    under the mask (the short call did not keep the long call's values inside its own range).  (p25fe_run_dev has no sync-event
    outputs: positions and dibit indices are in the slice_dev test below.)"""
    from p25rx_amd.frontend import parse_results
    look = PM.look_of(clock)
    loud = c4fm_stream(O, fmt, "loud")[0]
    rows, bb = c4fm_stream(O, fmt, "quiet")
    fe = FE(symbol_clock=clock)
    dib, res = fe.run_dev(dev(loud))
    assert int(parse_results(res)[0]["n_sync"]) >= 8
    for n_bb in reversed(LENGTHS):
        t = dev(rows[:5 * n_bb])
        what = "run_dev %s clock %d n_bb %d" % (fmt, clock, n_bb)
        dib, res = fe.run_dev(t)
        got = (dib[0].cpu().numpy(), parse_results(res)[0])
        check(fe, n_bb, [bb[:n_bb]], [PM.history(None, look)], look, what)
        f2 = FE(symbol_clock=clock)
        dib2, res2 = f2.run_dev(t)
        fresh = (dib2[0].cpu().numpy(), parse_results(res2)[0])
        f2.close()
        same_receiver_outputs(got, fresh, oracle_receiver(O, bb[:n_bb], clock), what)


@pytest.mark.parametrize("clock", [0, 1, 2])
def test_short_slice_dev_calls_after_a_loud_one(O, FE, clock):
    """the same through p25fe_slice_dev (k_planarize) after a loud p25fe_run_dev on the handle: dibits, count, sync positions, sync
    dibit indices and anchor_out equal the oracle's and a fresh handle's; planes equal the model"""
    from p25rx_amd.frontend import parse_results
    look = PM.look_of(clock)
    loud = c4fm_stream(O, "cf32", "loud")[0]
    bb = c4fm_stream(O, "cf32", "quiet")[1]
    fe = FE(symbol_clock=clock)
    fe.run_dev(dev(loud))

    def call(h, t, n_bb):
        dib, res, sp, sd = h.slice_dev(t, n_bb, sync_cap=256)
        return dib[0].cpu().numpy(), parse_results(res)[0], sp[0].cpu().numpy(), sd[0].cpu().numpy()
    for n_bb in reversed(LENGTHS):
        t = dev(bb[:n_bb])
        what = "slice_dev clock %d n_bb %d" % (clock, n_bb)
        got = call(fe, t, n_bb)
        check(fe, n_bb, [bb[:n_bb]], [PM.history(None, look)], look, what)
        f2 = FE(symbol_clock=clock)
        fresh = call(f2, t, n_bb)
        f2.close()
        same_receiver_outputs(got, fresh, oracle_receiver(O, bb[:n_bb], clock), what)
