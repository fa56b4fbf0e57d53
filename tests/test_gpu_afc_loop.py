"""The AFC loop on the GPU (docs/SPEC.md 3.0g: k_afc_loop and the sequencer p25fe_track_run_dev), through the C ABI, bit for bit
against tests/afc_loop_model.py.

update: every outcome in one launch, records written from the host, K = 1, 3 and 256, positions past 2^32.  Sequencer: tuner
ratios 12/125 (T 84) and 24/25 (T 9) as in tests/test_gpu_afc.py's test_retune, the measure's smallest shape (D 3, T 7), windows
of 1024 input samples: one call equals any split of it and the hand-written sequence, rows and states equal the model.  End to end:
the drifting capture of tests/test_afc_loop_abi.py through the tracked tuner and a one-channel handle's receive chain."""
import numpy as np
import pytest

import afc_loop_model as LM
import afc_model as AM
import resample_model as RM
from test_gpu_afc import check_rows, model_range
from test_gpu_tune import cnoise, host, rand_taps
from test_gpu_wide_fmt import bits, conv, dev, noise

pytestmark = pytest.mark.gpu

MASK = (1 << 32) - 1
D_, T_ = 3, 7                                                        # the smallest of test_gpu_afc.SHAPES
RATIOS = [(12, 125, 84), (24, 25, 9)]
SMALL = dict(shift=24, min_products=100, coh_min_q15=8192, gain_q16=65536, max_pull=1 << 22, max_dev=1 << 23)


@pytest.fixture(scope="module")
def mods():
    from p25rx_amd import _lib
    from p25rx_amd.frontend import Afc, AfcLoop, FrontEnd, Tuner
    return _lib, FrontEnd, Tuner, Afc, AfcLoop


@pytest.fixture(scope="module")
def rot(mods):
    return mods[2].rotator(256)


def _state(rec):
    return {f: int(rec[f]) for f in LM.STATE_FIELDS}


def _recs(rec_array):
    return [tuple(int(v) for v in r) for r in rec_array]


def _refused(_lib, fn, *a, **kw):
    with pytest.raises(_lib.P25feError) as ei:
        fn(*a, **kw)
    assert ei.value.status == _lib.ERR_ARG


# ---- update -------------------------------------------------------------------------------------------------------------------
def _outcome_records(K, rng):
    """K records that take every path of the law: short, pow <= 0, incoherent, applied small / large / either sign / half turn"""
    base = [(5000, 100, 5100, 99), (5000, 100, 5100, 100), (5000, 100, 0, 500), (5000, 100, -7, 500), (100, 50, 5000, 500),
            (-4000, 3000, 5001, 500), (0, -(1 << 40), (1 << 40) + 5, 1200), (-(1 << 50), 0, 1 << 50, 1200), (1 << 61, -(1 << 61), 1 << 62, 1200),
            (123456789, 2345678, 123500000, 100), (0, 0, 5000, 500), (0, 0, 0, 0)]
    out = []
    for k in range(K):
        if k < len(base):
            out.append(base[k])
        else:
            b = int(rng.integers(8, 62))
            re, im = (int(v) for v in rng.integers(-(1 << b), 1 << b, size=2))
            out.append((re, im, int(max(abs(re), abs(im)) * float(rng.uniform(0.8, 4.0))) + 1, int(rng.integers(0, 300))))
    return out


@pytest.mark.parametrize("K", [1, 3, 256])
@pytest.mark.parametrize("ratio", RATIOS, ids=lambda r: "%d_%d" % r[:2])
def test_update_is_the_law(mods, rot, ratio, K):
    """records written from the host, one launch, then the state records, the tuner's (step, ph0) (through read and get_step) and
    the zeroed or kept records against the model, field for field; three updates in a row at 5000, 2^32 + 77 and 2^40 + 5, the
    counts carried along; then a range through the tuner with the updated numbers against the model (K <= 3)"""
    _lib, FE, TN, Afc, Loop = mods
    L, M, T = ratio
    rng = np.random.default_rng(500 + K + L)
    taps = rand_taps(rng, L, T)
    steps = [int(v) for v in rng.integers(-(1 << 31), 1 << 31, size=K)]
    steps[0] = (1 << 31) - 1000                                      # the int32 clamp is within one pull
    fe = FE()
    tn = TN.nco(fe, L, M, T, taps, steps)
    afc = Afc(fe, K, D_, T_)
    cfg = dict(SMALL, max_dev=(1 << 31) - 1, max_pull=1 << 26)
    loop = Loop(tn, afc, **cfg)
    states = [LM.new_state(s) for s in steps]
    assert [_state(s) for s in loop.read()] == states and _recs(loop.records()) == [(0, 0, 0, 0)] * K
    seen = set()
    for rnd, at in enumerate((5000, (1 << 32) + 77, (1 << 40) + 5)):
        recs = _outcome_records(max(K, 12), rng)
        recs = (recs[rnd:] + recs[:rnd])[:K] if K > 1 else [recs[(1, 5, 0)[rnd]]]
        arr = np.zeros(K, dtype=_lib.AFC_ACC_DTYPE)
        for k, r in enumerate(recs):
            arr[k] = r
        loop.records(set=arr)
        loop.update(at)
        _refused(_lib, tn.get_step, 0)                               # stale from the first update on
        _refused(_lib, tn.set_step, 0, 5, at)
        want = [LM.step(cfg, L, M, D_, steps[k], recs[k], states[k], at) for k in range(K)]
        got = loop.read()
        assert [_state(s) for s in got] == [w[1] for w in want], (K, at)
        assert _recs(loop.records()) == [w[0] for w in want], (K, at)
        states = [w[1] for w in want]
        assert [tn.get_step(k) for k in range(K)] == [(s["step"], s["ph0"]) for s in states]
        seen |= {s["status"] for s in states}
    if K > 1:
        assert seen == {LM.SHORT, LM.REJECT, LM.APPLY}
        assert states[0]["step"] <= (1 << 31) - 1
    assert _lib.ERR_ARG == fe.L.p25fe_track_update_dev(loop.lp, 1 << 62, None)
    if K <= 3:
        n, hist, P = 600, 96, (1 << 40) + 8
        x = cnoise(rng, hist + n)
        y, no = tn.tune_dev(dev(x), n_hist=hist, abs0=P, offset=hist)
        check_rows(y, no, model_range(rot, x, hist, P, L, M, T, taps, [(s["step"], s["ph0"]) for s in states]), ("after updates", K))
    loop.close()


# ---- the sequencer ------------------------------------------------------------------------------------------------------------
W = 1024


def model_tracked(rot, x, hist, P, n, L, M, T, taps, steps, g, cfg):
    """x = [hist samples | n owned samples from position P] -> (rows [K, count], states, open records): the sequencer's pieces, each
    tuned with the channel's current (step, ph0) (the T - 1 history samples too), measured from the rows so far (zero before the
    first row: the measure's position is the absolute OUTPUT index), updated at every multiple of W"""
    K = len(steps)
    states = [LM.new_state(s) for s in steps]
    out_first = P * L // M
    r = out_first % D_
    rows = np.zeros((K, 0), dtype=np.complex64)
    accs = [(0, 0, 0, 0)] * K
    for a, b, upd in LM.pieces(P, n, W):
        lo, hi = hist + (a - P), hist + (b - P)
        part = model_range(rot, x[lo - (T - 1):hi], T - 1, a, L, M, T, taps, [(s["step"], s["ph0"]) for s in states])
        o_a = rows.shape[1]
        rows = np.concatenate([rows, part], axis=1)
        o_b = rows.shape[1]
        for k in range(K):
            z = np.concatenate([np.zeros(r, dtype=np.complex64), rows[k]])
            new = AM.record(AM.products(z, D_, T_, g, cfg["shift"]), (r + o_a) // D_, (r + o_b) // D_ - (r + o_a) // D_)
            accs[k] = tuple(AM.wrap64(p + q) for p, q in zip(accs[k][:3], new[:3])) + (accs[k][3] + new[3],)
            if upd:
                accs[k], states[k] = LM.step(cfg, L, M, D_, steps[k], accs[k], states[k], b)
    return rows, states, accs


def _fresh(mods, L, M, T, taps, steps, cfg):
    _lib, FE, TN, Afc, Loop = mods
    fe = FE()
    tn = TN.nco(fe, L, M, T, taps, steps)
    afc = Afc(fe, len(steps), D_, T_)
    return fe, tn, afc, Loop(tn, afc, **cfg)


@pytest.mark.parametrize("fmt", ["cf32", "s16", "u8"])
@pytest.mark.parametrize("ratio", RATIOS, ids=lambda r: "%d_%d" % r[:2])
def test_tracked_range(mods, rot, ratio, fmt):
    """K = 3 from P = 5000 and 2^32 + 72 (multiples of 8, not of the window): 3600 samples = a partial window, three whole ones and
    a trailing partial one.  One call against the model (rows bit for bit, states, open records), against the same range split at a
    window boundary and off it, and against the hand-written tune / measure / update; guard bands in front of and behind the rows;
    the alignment refusals."""
    import torch
    _lib, FE, TN, Afc, Loop = mods
    L, M, T = ratio
    K, hist, n, sentinel = 3, 96, 3600, -123456.75
    rng = np.random.default_rng(700 + L)
    taps = rand_taps(rng, L, T)
    steps = [232387521, -3527459, 0]
    raw = cnoise(rng, hist + n) if fmt == "cf32" else noise(fmt, rng, hist + n)
    x = raw if fmt == "cf32" else conv(raw)
    tx = dev(raw)
    g = Afc.design(D_, T_)
    # every judged window is applied (gate 0); the first piece from 5000 (120 samples) is short and its products stay in the record
    cfg = dict(SMALL, coh_min_q15=0, min_products=20 if L == 12 else 40)
    for P in (5000, (1 << 32) + 72):
        assert P % 8 == 0 and P % W != 0
        ref, want_states, want_acc = model_tracked(rot, x, hist, P, n, L, M, T, taps, steps, g, cfg)
        cnt = ref.shape[1]
        assert cnt == RM.n_resample(L, M, P, n) and len(LM.pieces(P, n, W)) == (5 if P == 5000 else 4)
        assert all(s["status"] == LM.APPLY and s["step"] != st for s, st in zip(want_states, steps))
        assert all(s["n_short"] == (1 if P == 5000 else 0) for s in want_states) and all(a[3] > 0 for a in want_acc)
        front = 4

        def run(cuts):
            fe, tn, afc, loop = _fresh(mods, L, M, T, taps, steps, cfg)
            out = torch.full((K, front + cnt + 38, 2), sentinel, device="cuda")
            done = 0
            for a, b in zip(cuts, cuts[1:]):
                o, no = loop.tune_tracked_dev(tx[:hist + b], W, n_hist=hist + a, abs0=P + a, offset=hist + a, out=out, out_offset=front + done,
                                              n_hist_out=done)
                done += no
            assert done == cnt
            assert bool((out[:, :front] == sentinel).all()) and bool((out[:, front + cnt:] == sentinel).all()), "guard bands"
            st = [_state(s) for s in loop.read()]
            acc = _recs(loop.records())
            rows = out[:, front:front + cnt].cpu().numpy().view(np.complex64).reshape(K, cnt)
            loop.close()
            return rows, st, acc, out
        rows, st, acc, out = run((0, n))
        check_rows(out[:, front:], cnt, ref, ("one call", P, fmt))
        assert st == want_states and acc == want_acc, (P, fmt)
        edge = W - P % W                                             # the first window boundary inside the range
        for cuts in ((0, edge, n), (0, edge + W, edge + W + 8, n), (0, 8, edge - 8, edge + 2 * W + 512, n)):
            r2, s2, a2, _ = run(cuts)
            assert np.array_equal(bits(r2), bits(rows)) and s2 == st and a2 == acc, (cuts, P, fmt)
        # by hand: tune, measure, update
        fe, tn, afc, loop = _fresh(mods, L, M, T, taps, steps, cfg)
        parts, done = [], 0
        for a, b, upd in LM.pieces(P, n, W):
            y, no = tn.tune_dev(tx[:hist + b - P], n_hist=hist + a - P, abs0=a, offset=hist + a - P)
            parts.append(y[:, :no])
            allrows = torch.cat(parts, dim=1).contiguous()
            loop.measure(allrows, n_hist=done, abs0=P * L // M + done, offset=done, n=no)
            done += no
            if upd:
                loop.update(b)
        assert np.array_equal(bits(allrows.cpu().numpy().view(np.complex64).reshape(K, cnt)), bits(rows))
        assert [_state(s) for s in loop.read()] == st and _recs(loop.records()) == acc
        # refusals: nothing is enqueued, the states stay
        o = torch.full((K, cnt + 8, 2), sentinel, device="cuda")
        for window, at in ((W + 1, P), (W, P + 1), (0, P), (1 << 62, P), ((T - 2) // 8 * 8, P), (W, 1 << 62)):
            _refused(_lib, loop.tune_tracked_dev, tx, window, n_hist=hist, abs0=at, offset=hist, out=o)
        small = torch.full((K, cnt - 2, 2), sentinel, device="cuda")
        code = {"cf32": _lib.FMT_CF32, "s16": _lib.FMT_S16, "u8": _lib.FMT_U8}[fmt]
        assert fe.L.p25fe_track_run_dev(loop.lp, tx.data_ptr() + hist * tx.element_size() * 2, code, hist, n, P, W, small.data_ptr(), cnt - 2,
                                        0, None) == _lib.ERR_ARG
        assert bool((o == sentinel).all()) and bool((small == sentinel).all())
        assert [_state(s) for s in loop.read()] == st
        loop.close()


def test_staleness_and_create_refusals(mods):
    """set_step / get_step are refused from the first update (or sequencer call) until read, after which the host's pair is the
    device's; a loop wants an NCO tuner that is not stale, the measure's channel count and handle"""
    _lib, FE, TN, Afc, Loop = mods
    L, M, T = 24, 25, 9
    rng = np.random.default_rng(9)
    taps = rand_taps(rng, L, T)
    fe, tn, afc, loop = _fresh(mods, L, M, T, taps, [1000, -1000], SMALL)
    assert tn.get_step(1) == (-1000, 0)
    tn.set_step(1, -900, 800)                                        # before any update: as ever
    par = AM.set_step(-1000, 0, -900, 800)
    arr = np.zeros(2, dtype=_lib.AFC_ACC_DTYPE)
    arr[0], arr[1] = (0, 5000, 5000, 500), (5000, 0, 5000, 5)
    loop.records(set=arr)
    loop.update(1600)
    _refused(_lib, tn.get_step, 0)
    _refused(_lib, tn.set_step, 0, 5, 1600)
    _refused(_lib, Loop, tn, afc, **SMALL)                           # a second loop on a stale tuner
    st = loop.read()
    want0 = LM.step(SMALL, L, M, D_, 1000, (0, 5000, 5000, 500), LM.new_state(1000), 1600)[1]
    assert _state(st[0]) == want0 and want0["step"] > 1000 and want0["ph0"] != 0
    # channel 1 was short: the kernel kept what set_step had left in the tuner's record
    assert (int(st[1]["step"]), int(st[1]["ph0"]), int(st[1]["status"])) == (par[0], par[1], LM.SHORT)
    assert tn.get_step(0) == (want0["step"], want0["ph0"]) and tn.get_step(1) == par
    tn.set_step(0, 1234, 2400)                                       # works again, and the next update goes on from it
    p0 = AM.set_step(want0["step"], want0["ph0"], 1234, 2400)
    loop.records(set=arr)
    loop.update(3200)
    st = loop.read()
    want = LM.step(SMALL, L, M, D_, 1000, (0, 5000, 5000, 500), dict(want0, step=p0[0], ph0=p0[1]), 3200)[1]
    assert _state(st[0]) == want
    loop.close()
    assert tn.get_step(0) == (want["step"], want["ph0"])             # the tuner outlives the loop
    rat = TN(fe, L, M, T, taps, [(11, 200), (1, 8)])
    _refused(_lib, Loop, rat, afc, **SMALL)
    _refused(_lib, Loop, tn, Afc(fe, 3, D_, T_), **SMALL)
    _refused(_lib, Loop, tn, Afc(FE(), 2, D_, T_), **SMALL)
    _refused(_lib, Loop, tn, afc, **dict(SMALL, gain_q16=0))


# ---- end to end ---------------------------------------------------------------------------------------------------------------
E_FS, E_WINDOW, E_RASTER = 2500000, 125000, 137500


def test_end_to_end_on_a_drifting_carrier(mods, rot):
    """tests/test_afc_loop_abi.py's capture (1871.3 Hz off the raster, +3000 Hz/s) through the tracked tuner with the recommended
    loop and a one-channel handle's receive chain: the states are the model's, and from the first frame sync after the first update
    (the generator's symbol 888) to the end of the capture there is no symbol error.  The same capture with ONE set_step after
    50 ms (what p25fe_replay -a 50 does) is out of lock at the end: its last 500 symbols hold errors."""
    from p25rx_amd.frontend import parse_results
    _lib, FE, TN, Afc, Loop = mods
    wide, truth = LM.drifting_capture()
    L, M, T, taps, steps = TN.design_nco(E_FS, [E_RASTER])
    D, Tg, fc = Afc.DEFAULT
    fe = FE()
    tn = TN.nco(fe, L, M, T, taps, steps)
    afc = Afc(fe, 1)
    loop = Loop(tn, afc)
    assert {k: int(loop.cfg[k][0]) for k in LM.RECOMMENDED} == LM.RECOMMENDED
    tw = dev(wide)
    y, no = loop.tune_tracked_dev(tw, E_WINDOW)
    st = _state(loop.read()[0])
    _, states, _ = LM.track(wide, L, M, T, taps, steps[0], *rot, D, Tg, Afc.design(D, Tg, fc), LM.RECOMMENDED, E_WINDOW)
    assert st == states[-1] and st["n_applied"] == 15
    dib, res = fe.run_dev(y[0, :no])
    got = dib[0, :int(parse_results(res)[0]["n_dibits"])].cpu().numpy()
    k = min(len(got), len(truth) - 888)
    assert k > 2600 and np.array_equal(got[:k], truth[888:888 + k])
    loop.close()
    # one correction after 50 ms
    tn2 = TN.nco(fe, L, M, T, taps, steps)
    head, nh = tn2.tune_dev(tw[:E_WINDOW])
    hz, coh = Afc.hz(Afc.records(afc.measure(head, n=nh))[0], D)
    tn2.set_step(0, steps[0] + TN.nco_step(E_FS, hz), E_WINDOW)
    y2, n2 = tn2.tune_dev(tw, n_hist=T - 1, abs0=E_WINDOW, offset=E_WINDOW)
    fe.reset()
    dib2, res2 = fe.run_dev(y2[0, :n2])
    got2 = dib2[0, :int(parse_results(res2)[0]["n_dibits"])].cpu().numpy()
    k2 = min(len(got2), len(truth) - 888)
    tail = got2[:k2][-500:] != truth[888:888 + k2][-500:]
    print("one-shot: %d symbols, %d errors in the last 500" % (k2, int(tail.sum())))
    assert k2 < k - 400 or int(tail.sum()) > 0


def test_replay_tracks(tmp_path):
    """p25fe_replay -r 2500000 -F 137500 -A 50 on the drifting capture decodes to the end without a symbol error from the first
    frame sync after the first update, and writes one afc event per 50 ms boundary (15), each with a status; -a 50 on the same file
    decodes fewer symbols correctly (it is out of lock at the end); -A with -a, or without -F, is a usage error"""
    import json
    import os
    import subprocess
    wide, truth = LM.drifting_capture()
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "p25fe_replay")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    src, out, out2, js = tmp_path / "cap.cf32", tmp_path / "dib.out", tmp_path / "dib2.out", tmp_path / "ev.jsonl"
    np.asarray(wide).tofile(src)
    r = subprocess.run([exe, "-j", str(js), "-r", str(E_FS), "-F", str(E_RASTER), "-A", "50", "cf32", str(src), str(out)],
                       capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stderr[-1000:]
    got = np.fromfile(out, dtype=np.uint8)
    k = min(len(got), len(truth) - 888)
    assert k > 2600 and np.array_equal(got[:k], truth[888:888 + k])
    ev = [json.loads(line) for line in open(js) if '"afc"' in line]
    assert [e["at"] for e in ev] == [E_WINDOW * (w + 1) for w in range(15)]
    assert all(e["event"] == "afc" and e["status"] == "apply" and e["products"] == 1200 and e["coherence"] > 0.75 for e in ev)
    assert abs(ev[0]["hz"] - 1871.3) <= 150.0 and all(abs(e["hz"]) <= 600.0 for e in ev[1:])
    r = subprocess.run([exe, "-r", str(E_FS), "-F", str(E_RASTER), "-a", "50", "cf32", str(src), str(out2)], capture_output=True, text=True,
                       timeout=100)
    assert r.returncode == 0, r.stderr[-1000:]
    got2 = np.fromfile(out2, dtype=np.uint8)
    k2 = min(len(got2), len(truth) - 888)
    good2 = int(np.count_nonzero(got2[:k2] == truth[888:888 + k2]))
    print("-a 50: %d symbols, %d of them right; -A 50: %d, all right" % (k2, good2, k))
    assert good2 < k - 400
    for args in (["-r", str(E_FS), "-F", str(E_RASTER), "-a", "50", "-A", "50"], ["-r", str(E_FS), "-f", str(E_RASTER), "-A", "50"],
                 ["-r", str(E_FS), "-A", "50"]):
        r = subprocess.run([exe] + args + ["cf32", str(src), str(out2)], capture_output=True, text=True)
        assert r.returncode != 0 and "usage" in r.stderr
