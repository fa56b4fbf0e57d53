"""P25FE_FMT_S16 on the GPU, through every entry point that takes a format.

An s16 stream IS the cf32 stream of its converted samples (docs/SPEC.md 3.1), so every expected value here comes from one
recipe: int16 -> numpy float32 `v.astype(np.float32) * np.float32(2**-15)` -> the CPU oracle, compared bit for bit; and where
the cf32 path of the same handle runs on the converted samples, its output must equal the s16 output byte for byte.
Only power_dbm (tree against sequential reduction) has a tolerance: 1e-3 dB, as in tests/test_gpu_parity.py.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCALE = np.float32(2.0 ** -15)


def conv(s16):
    """[..., 2 n] int16 -> [..., n] complex64: the definition of the format"""
    return np.ascontiguousarray(np.asarray(s16, dtype=np.int16).astype(np.float32) * SCALE).view(np.complex64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def FE():
    from p25rx_amd.frontend import FrontEnd
    return FrontEnd


@pytest.fixture(scope="module")
def cap(c4fm_1s):
    """the 1 s capture as s16, its converted samples and the oracle's one-pass outputs (computed once, never written to)"""
    from oracle import oracle as O
    from p25rx_amd import c4fm
    s16 = c4fm.to_s16(c4fm_1s[0])
    cf = conv(s16)
    bb = O.Demod().feed_cf32(cf)
    dib, spos, sdib = O.recv_range(bb)
    for a in (s16, cf, bb, dib, spos, sdib):
        a.setflags(write=False)
    assert len(dib) == 4769 and np.array_equal(dib, O.run_cf32(cf)) and len(spos) >= 5
    return dict(s16=s16, cf=cf, bb=bb, dib=dib, spos=spos, sdib=sdib)


def dev_s16(a):
    import torch
    a = np.asarray(a, dtype=np.int16)
    return torch.from_numpy(a.reshape(a.shape[:-1] + (-1, 2)).copy()).cuda()


def dev_cf(a):
    import torch
    a = np.ascontiguousarray(a, dtype=np.complex64)
    return torch.from_numpy(a.view(np.float32).reshape(a.shape + (2,)).copy()).cuda()


N1 = 40007       # > two whole segments at any sub-tile count up to 9 (9 x 320 outputs x 5 = 14 400 samples), a partial one, a ragged tail


def edge_noise(rng, rows, n):
    """random int16 noise with the rows -32768, 32767, 0 and an alternating +/- full-scale stretch spliced in"""
    x = rng.integers(-32768, 32768, size=(rows, 2 * n), dtype=np.int64).astype(np.int16)
    x[:, 2000:2600] = -32768
    x[:, 9000:9700] = 32767
    x[:, 15000:15500] = 0
    alt = np.where(np.arange(1200) % 2 == 0, 32767, -32768).astype(np.int16)
    x[:, 30000:31200] = alt
    x[:, 31200:32400] = np.repeat(alt[:600], 2)                     # ... and alternating per complex sample
    return x


def _tables(kind):
    """(FrontEnd keywords, oracle keywords) of the three kernel variants"""
    rng = np.random.default_rng(11)
    if kind == "builtin":
        return {}, {}
    if kind == "generic":
        kw = dict(decim_taps=list((rng.standard_normal(31) * 0.1).astype(np.float32)),
                  chan_taps=list((rng.standard_normal(41) * 0.1).astype(np.float32)))
    else:                                                           # the long geometry: 64 / 64 tables + a 41-tap post-discriminator filter
        kw = dict(decim_taps=list((rng.standard_normal(64) * 0.1).astype(np.float32)),
                  chan_taps=list((rng.standard_normal(64) * 0.1).astype(np.float32)),
                  avg_taps=list((rng.standard_normal(41) * 0.1).astype(np.float32)))
    return kw, dict(kw)


def _check_demod_dev(O, FE, kind, Cn, **fe_extra):
    import torch
    from p25rx_amd import _lib
    fkw, okw = _tables(kind)
    if fkw:
        fkw = dict(fkw, specialize=_lib.SPECIALIZE_OFF)
    fkw.update(fe_extra)
    rng = np.random.default_rng(100 + Cn)
    x = edge_noise(rng, Cn, N1)
    cf = conv(x)
    fe = FE(n_channels=Cn, **fkw)
    assert fe.format_variant(_lib.FMT_S16) == (_lib.VARIANT_BUILTIN if kind == "builtin" else _lib.VARIANT_GENERIC)
    stride = (N1 + 3) // 4 * 4 + 4                                   # channel stride: n rounded up to 4, plus 4
    buf = torch.zeros((Cn, stride, 2), dtype=torch.int16, device="cuda")
    buf[:, :N1] = dev_s16(x)
    bufc = torch.zeros((Cn, stride, 2), dtype=torch.float32, device="cuda")
    bufc[:, :N1] = dev_cf(cf)
    t, tc = (buf[0, :N1], bufc[0, :N1]) if Cn == 1 else (buf[:, :N1], bufc[:, :N1])
    # (a) from the start of a stream
    bb, nb, pw = fe.demod_dev(t, want_power=True)
    bbc, nbc, pwc = fe.demod_dev(tc, want_power=True)
    assert nb == nbc
    for c in range(Cn):
        ref, rp = O.Demod(O.make_config(**okw)).feed_cf32(cf[c], want_power=True)
        assert nb == len(ref)
        got = bb[c, :nb].cpu().numpy()
        assert np.array_equal(bits(got), bits(ref)), (kind, Cn, c, int(np.flatnonzero(bits(got) != bits(ref))[0]))
        assert abs(float(pw[c]) - rp) < 1e-3
    assert torch.equal(bb[:, :nb].view(torch.int32), bbc[:, :nb].view(torch.int32))
    # (b) as a range: 2 559 samples of history (odd: the in-vector fix-up runs), abs0 = 3 (mod 5), the range 4 samples into the
    # buffer: owned sample 0 at 4 + 2 560 (a 16-byte boundary), the history in [5, 2 564); what lies in front of it is NOT history
    # and must read as zero, so it is filled with full-scale garbage
    off, nh, abs0 = 4 + 2560, 2559, 5 * 700 + 3
    n = N1 - off
    buf[:, :off - nh] = 32767
    bufc[:, :off - nh] = 1.0
    bb2, nb2 = fe.demod_dev(t, n_hist=nh, abs0=abs0, offset=off)
    bb2c, _ = fe.demod_dev(tc, n_hist=nh, abs0=abs0, offset=off)
    for c in range(Cn):
        od = O.Demod(O.make_config(**okw))
        # the oracle's stream: zeros (its filters start from zero, as the kernel's history does in front of the nh valid samples)
        # that put the first owned sample on abs0's place in the 5:1 grid, the history, the owned samples; the outputs of the
        # owned part are the reference
        lead = np.zeros((abs0 - nh) % 5, dtype=np.complex64)
        full = od.feed_cf32(np.concatenate([lead, cf[c, off - nh:off + n]]))
        ref = full[len(full) - nb2:]
        got = bb2[c, :nb2].cpu().numpy()
        assert np.array_equal(bits(got), bits(ref)), (kind, Cn, c)
    assert torch.equal(bb2[:, :nb2].view(torch.int32), bb2c[:, :nb2].view(torch.int32))


@pytest.mark.parametrize("Cn", [1, 3])
def test_demod_dev_linear_baseband(O, FE, Cn):
    """test 1: p25fe_demod_dev, built-in kernels, from the stream's start and as a range, C = 1 and C = 3 with a padded stride"""
    _check_demod_dev(O, FE, "builtin", Cn)


@pytest.mark.parametrize("kind", ["generic", "long"])
def test_demod_dev_generic_variants(O, FE, kind):
    """test 2: the same input through the generic kernels (31 / 41 random tables) and the generic long geometry (64 / 64 + a
    41-tap post-discriminator filter), the oracle configured with the same numbers"""
    _check_demod_dev(O, FE, kind, 1)


_AUTO_CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_s16 as T
from oracle import oracle as O
from p25rx_amd import _lib
from p25rx_amd.frontend import FrontEnd
fkw, okw = T._tables("generic")
fe = FrontEnd(**fkw)                                                 # specialize = AUTO
assert fe.kernel_variant == _lib.VARIANT_SPECIALIZED, fe.kernel_variant
assert fe.format_variant(_lib.FMT_S16) == _lib.VARIANT_GENERIC
assert fe.format_variant(_lib.FMT_CF32) == _lib.VARIANT_SPECIALIZED == fe.format_variant(_lib.FMT_U8)
x = T.edge_noise(np.random.default_rng(7), 1, T.N1)
cf = T.conv(x)
ref = O.Demod(O.make_config(**okw)).feed_cf32(cf[0])
bb, nb = fe.demod_dev(T.dev_s16(x[0]))
bbc, nbc = fe.demod_dev(T.dev_cf(cf[0]))
assert nb == nbc == len(ref)
assert np.array_equal(T.bits(bb[0, :nb].cpu().numpy()), T.bits(ref)), "s16 through the generic kernels"
assert np.array_equal(T.bits(bbc[0, :nb].cpu().numpy()), T.bits(ref)), "cf32 through the specialised kernels"
d, r = fe.run_dev(T.dev_s16(x[0]))                                   # the planar generic s16 kernel beside the specialised planar cf32 one
dc, rc = fe.run_dev(T.dev_cf(cf[0]))
torch.cuda.synchronize()
from p25rx_amd.frontend import parse_results
rs, rcf = parse_results(r)[0], parse_results(rc)[0]
assert rs.tobytes() == rcf.tobytes(), (rs, rcf)
k = int(rs["n_dibits"])                                              # (the rows are uninitialised behind their last dibit)
assert torch.equal(d[0, :k], dc[0, :k]), "dibits of the generic s16 pass and the specialised cf32 pass"
print("AUTO-OK")
"""


def test_auto_handle_runs_s16_generic_beside_specialised_cf32(tmp_path):
    """test 2, the AUTO handle: with 31 / 41 tables cf32 gets specialised kernels, s16 the generic ones -- reported per format --
    and both match the oracle.  In a process of its own: the suite switches AUTO's specialisation off (conftest.py: P25FE_JIT=0),
    and the library reads that once per process.  The code object is compiled here ahead of time, so the child only loads it."""
    import os
    import subprocess
    import sys
    from p25rx_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = str(tmp_path / "spec")
    assert _lib.specialize(_lib.make_config(**_tables("generic")[0]), spec)
    env = dict(os.environ, P25FE_JIT="1", P25FE_SPEC_DIR=spec, P25FE_CACHE_DIR=str(tmp_path / "cache"))
    p = subprocess.run([sys.executable, "-c", _AUTO_CHILD, root], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "AUTO-OK" in p.stdout, p.stdout + p.stderr
    # the fallback is announced, once, on stderr
    assert p.stderr.count("P25FE_FMT_S16 has no specialised kernels") == 1, p.stderr


@pytest.mark.parametrize("clock", [0, 1, 2])
def test_fused_pass_run_dev_and_pipelined(O, FE, cap, clock):
    """test 3: p25fe_run_dev and p25fe_run_dev_pipelined + join on the 1 s capture as s16, under each symbol clock: dibits, the
    result record, sync positions and sync dibit indices against the oracle; 64-byte guard bands around the output rows"""
    import torch
    from p25rx_amd._lib import RESULT_DTYPE
    from p25rx_amd.frontend import parse_results
    cfg = O.make_config(symbol_clock=clock)
    if clock == 0:
        bb, dib, spos, sdib = cap["bb"], cap["dib"], cap["spos"], cap["sdib"]
    else:
        bb = cap["bb"]
        dib, spos, sdib = O.recv_range(bb, cfg)
    fe = FE(symbol_clock=clock)
    t, tc = dev_s16(cap["s16"]), dev_cf(cap["cf"])
    n = t.shape[0]
    capd = fe.dibit_cap(n)
    G = 64

    def guarded(nbytes):
        g = torch.full((G + nbytes + G,), 0xA5, dtype=torch.uint8, device="cuda")
        return g, g[G:G + nbytes].view(1, nbytes)

    outs = []
    for pipelined in (False, True):
        gd, d = guarded(capd)
        gr, r = guarded(RESULT_DTYPE.itemsize)
        if pipelined:
            fe.run_dev_pipelined(t, dibits=d, result=r)
            fe.join_dev()
        else:
            fe.run_dev(t, dibits=d, result=r)
        torch.cuda.synchronize()
        res = parse_results(r)[0]
        assert int(res["n_baseband"]) == len(bb) and int(res["n_dibits"]) == len(dib) and int(res["n_sync"]) == len(spos)
        assert np.array_equal(d[0, :len(dib)].cpu().numpy(), dib), (clock, pipelined)
        if clock == 0:
            assert int(res["anchor_out"]["valid"]) != 0 and int(res["anchor_out"]["s"]) == int(spos[-1])
        for g, nb in ((gd, capd), (gr, RESULT_DTYPE.itemsize)):
            assert bool((g[:G] == 0xA5).all()) and bool((g[G + nb:] == 0xA5).all())
        outs.append((d[0, :len(dib)].clone(), res))
    assert outs[0][1].tobytes() == outs[1][1].tobytes() and torch.equal(outs[0][0], outs[1][0])
    # the cf32 path of the same handle on the converted samples: the same bytes
    dc, rc = fe.run_dev(tc)
    assert parse_results(rc)[0].tobytes() == outs[0][1].tobytes() and torch.equal(dc[0, :len(dib)], outs[0][0])
    # sync positions and sync dibit indices: the s16 baseband through the receiver with its event outputs
    bbd, nb = fe.demod_dev(t)
    assert nb == len(bb) and np.array_equal(bits(bbd[0, :nb].cpu().numpy()), bits(bb))
    d2, r2, sp, sd = fe.slice_dev(bbd[0], nb, sync_cap=64)
    k = int(parse_results(r2)[0]["n_sync"])
    assert k == len(spos)
    assert np.array_equal(sp[0, :k].cpu().numpy(), spos) and np.array_equal(sd[0, :k].cpu().numpy().astype(np.uint64), sdib)
    assert np.array_equal(d2[0, :len(dib)].cpu().numpy(), dib)


CHUNKS = [1, 2, 7, 333, 16384, 16385, 40000, 3, 16384]


def _chunks(n):
    edges = np.concatenate([[0], np.cumsum(CHUNKS), [n]])
    return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


def test_streaming_run_and_demod(O, FE, cap):
    """test 4: p25fe_run_s16 / p25fe_demod_s16 in ragged chunks (1 sample .. 40 000, both sides of the one-launch chunk path's
    16 384) equal the one-pass oracle; the format lock; the state blob of an s16 stream"""
    from p25rx_amd import _lib
    s16, cf = cap["s16"], cap["cf"]
    n = len(cf)
    ch = _chunks(n)
    fe, fd = FE(), FE()
    got, gotbb = [], []
    blob = None
    for i, (a, b) in enumerate(ch):
        got.append(fe.run_s16(s16[2 * a:2 * b]))
        gotbb.append(fd.demod_s16(s16[2 * a:2 * b]))
        if i == 3:
            blob = fe.state_export()
            # a cf32 call on the s16 stream: refused, and nothing moves
            L = fe.L
            dib = np.zeros(64, dtype=np.uint8)
            nd = C.c_size_t(99)
            x = np.ascontiguousarray(cf[b:b + 100])
            rc = L.p25fe_run_cf32(fe.h, x.ctypes.data_as(C.c_void_p), 100, dib.ctypes.data_as(C.c_void_p), 64, C.byref(nd))
            assert rc == _lib.ERR_FORMAT
            assert fe.state_export().tobytes() == blob.tobytes()
    assert np.array_equal(np.concatenate(got), cap["dib"])
    assert np.array_equal(bits(np.concatenate(gotbb)), bits(cap["bb"]))
    # the blob after the fourth chunk continues identically in a fresh handle
    assert int(np.frombuffer(blob[12:16].tobytes(), dtype=np.int32)[0]) == _lib.FMT_S16         # fmt_locked
    fe2 = FE()
    fe2.state_import(blob)
    rest = [fe2.run_s16(s16[2 * a:2 * b]) for a, b in ch[4:]]
    assert np.array_equal(np.concatenate(got[:4] + rest), cap["dib"])
    # a blob naming a format that does not exist is still refused
    bad = np.array(blob, dtype=np.uint8, copy=True)
    bad[12] = 3
    with pytest.raises(_lib.P25feError):
        FE().state_import(bad)


def test_host_windows_pinned_and_pageable(O, FE, cap):
    """test 5: p25fe_run_host_windows(P25FE_FMT_S16), window 8 192, 100 000 samples, C = 2, pinned and pageable input: the bytes of
    the resident pass"""
    import torch
    from p25rx_amd.frontend import parse_results
    n = 100000
    x = np.stack([cap["s16"][:2 * n], cap["s16"][2 * 20000:2 * (20000 + n)]])
    fe = FE(n_channels=2)
    dib, res = fe.run_dev(dev_s16(x))
    r = parse_results(res)
    want = [dib[c, :int(r["n_dibits"][c])].cpu().numpy() for c in range(2)]
    assert np.array_equal(want[0], O.run_cf32(conv(x[0]))) and np.array_equal(want[1], O.run_cf32(conv(x[1])))
    for pinned in (False, True):
        f2 = FE(n_channels=2)
        src = torch.from_numpy(x.copy()).pin_memory() if pinned else x
        outs, st = f2.run_host_windows(src, window=8192)
        assert st["n_windows"] == (n + 8191) // 8192 and st["pinned_input"] == pinned
        for c in range(2):
            assert np.array_equal(outs[c], want[c]), (pinned, c)


def test_time_shards_and_one_rank_step(O, FE, cap):
    """test 6: three shards of unequal length with p25fe_shard_halo() samples of halo through pass 1 / resolve / pass 2, and the
    one-rank p25fe_shard_step (halo of 2 560 x 4 bytes in front of the owned samples): the single pass's bytes"""
    import torch
    from p25rx_amd import _lib, rccl
    from p25rx_amd._lib import RESULT_DTYPE
    from p25rx_amd.frontend import parse_results, n_baseband
    t = dev_s16(cap["s16"])
    n = t.shape[0]
    ref = cap["dib"]
    fe = FE()
    halo = fe.shard_halo()
    assert halo == 2560
    cuts = [0, 70004, 70004 + 30008, n]                              # cut points on 16-byte boundaries of the s16 stream
    summ, bb0, bbn, fes = [], [], [], []
    for r in range(3):
        a, b = cuts[r], cuts[r + 1]
        h = min(a, halo)
        f = FE()
        fes.append(f)
        summ.append(parse_results(f.shard_pass1(t[a - h:b], offset=h, n_hist=h, abs0=a))[0])
        bb0.append(n_baseband(0, a))
        bbn.append(n_baseband(a, b - a))
    anc, off = fe.shard_resolve(np.array(summ), bb0, bbn)
    out = []
    for r in range(3):
        d, res = fes[r].shard_pass2(anc[r:r + 1], bbn[r], t.device)
        out.append(d[0, :int(parse_results(res)[0]["n_dibits"])].cpu().numpy())
        assert off[r] == sum(len(x) for x in out[:-1])
    assert np.array_equal(np.concatenate(out), ref)
    # one rank of the step behind include/p25fe_rccl.h, no communicator
    n8 = n // 8 * 8
    ss = rccl.ShardStep(fe, 0, 1, n8, None)
    ss.prepare()
    buf = torch.zeros((halo + n8, 2), dtype=torch.int16, device="cuda")
    buf[halo:] = t[:n8]
    d = torch.zeros((1, ss.dibit_cap), dtype=torch.uint8, device="cuda")
    res = torch.empty((1, RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    ss.step(buf, d, res, gather="root", fmt=_lib.FMT_S16)
    torch.cuda.synchronize()
    want, wres = FE().run_dev(t[:n8])
    nd = int(parse_results(wres)[0]["n_dibits"])
    assert int(parse_results(res)[0]["n_dibits"]) == nd and torch.equal(d[0, :nd], want[0, :nd])
    ss.close()


def test_refusals(O, FE, cap, tmp_path, monkeypatch):
    """test 7: the s16 layout rules (owned sample 0 on 16 bytes, stride a multiple of 4 samples) and s16 on a handle that may only run
    specialised kernels"""
    import torch
    from p25rx_amd import _lib
    n = 4096
    t = dev_s16(cap["s16"][:2 * (n + 8)])
    fe = FE()
    with pytest.raises(_lib.P25feError) as e:
        fe.demod_dev(t, offset=2)                                   # 8 bytes off alignment
    assert e.value.status == _lib.ERR_ARG
    fe.demod_dev(t, offset=4)                                       # 16 bytes: fine
    fe3 = FE(n_channels=3)
    bad = torch.zeros((3, n + 2, 2), dtype=torch.int16, device="cuda")
    with pytest.raises(_lib.P25feError) as e:
        fe3.demod_dev(bad[:, :n])                                   # channel stride n + 2
    assert e.value.status == _lib.ERR_ARG
    fe3.demod_dev(torch.zeros((3, n + 4, 2), dtype=torch.int16, device="cuda")[:, :n])
    with pytest.raises(_lib.P25feError) as e:                      # a format that does not exist
        fe._chk(fe.L.p25fe_demod_dev(fe.h, C.c_void_p(t.data_ptr()), 3, n, 0, n, 0, C.c_void_p(t.data_ptr()), n, None, None))
    assert e.value.status == _lib.ERR_ARG
    # REQUIRE + non-default tables: every s16 call is P25FE_ERR_JIT, the stream does not move, cf32 goes on working
    monkeypatch.setenv("P25FE_CACHE_DIR", str(tmp_path / "cache"))
    rng = np.random.default_rng(11)
    kw = dict(decim_taps=list((rng.standard_normal(31) * 0.1).astype(np.float32)),
              chan_taps=list((rng.standard_normal(41) * 0.1).astype(np.float32)))
    fr = FE(specialize=_lib.SPECIALIZE_REQUIRE, **kw)
    assert fr.kernel_variant == _lib.VARIANT_SPECIALIZED
    cf, s16 = cap["cf"], cap["s16"]
    a = fr.run_cf32(cf[:20000])
    before = fr.state_export().tobytes()
    for call in (lambda: fr.run_s16(s16[:2 * 5000]), lambda: fr.demod_s16(s16[:2 * 5000]), lambda: fr.demod_dev(t),
                 lambda: fr.run_dev(t), lambda: fr.run_dev_pipelined(t), lambda: fr.run_host_windows(s16[:2 * 20000], window=8192),
                 lambda: fr.shard_pass1(t, offset=0, n_hist=0, abs0=0), lambda: fr.format_variant(_lib.FMT_S16)):
        with pytest.raises(_lib.P25feError) as e:
            call()
        assert e.value.status == _lib.ERR_JIT
    assert fr.state_export().tobytes() == before
    b = fr.run_cf32(cf[20000:60000])
    assert np.array_equal(np.concatenate([a, b]), O.run_cf32(cf[:60000], O.make_config(**kw)))
