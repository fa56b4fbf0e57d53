#!/usr/bin/env python3
"""The tuner's cuts (k_tune_cuts, docs/SPEC.md 3.0j) beside the two things a caller could do without them, in one process, on
device-resident captures of --seconds (2) at 2.5 and 10 Msps held as cf32 and u8.  The capture holds 8 NCO channels; 24 keyings,
three per channel, each a twelfth of the capture long, cover a quarter of channel-time.  Cases, per rate and format:
  cuts   (a) ONE p25fe_cuts_dev for the 24 keyings;
  whole  (b) ONE p25fe_tune_dev of the 8 channels over the whole range;
  loop   (c) 24 p25fe_tune_dev calls on one-channel objects, one per keying -- issued from Python through ctypes: what is timed is
         this caller's launch path, a C caller's was not measured;
  full   (a) with cuts that cover everything: the 8 whole rows, to hold against (b).
Before anything is timed the three are compared bit for bit: every cut is the slice of the whole-range row, and the loop's rows are
the cuts'.  Every case sits between its own pair of device events, around the launches only (the outputs are allocated once and not
zeroed inside the timed region), and the cases alternate round by round, so a drift of the machine falls on all of them alike.
Per case: median / min / max in ms; for cuts its time against whole beside the fraction of channel-time it cuts.
One JSON line, also written to <out>/tune_cuts_time_<box>_<tag>.json.
usage: tune_cuts_time.py [--seconds 2] [--reps 20] [--out profiles] [--box NAME] [--tag run1]"""
import argparse, json, os, socket, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from p25rx_amd.frontend import Cuts, FrontEnd, Tuner

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=2.0)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
ap.add_argument("--box", default=socket.gethostname())
ap.add_argument("--tag", default="run")
a = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = torch.device("cuda", 0)
OFFSETS = (-412500 + 1871.3, -137500 - 912.4, -12500 + 120.0, 733.1, 137500 - 2210.7, 150000 - 2411.6, 300000 + 55.5, 500000 - 1300.9)
K, PER_CH = len(OFFSETS), 3
fe = FrontEnd(device=0)

gen = torch.Generator(device=dev)
gen.manual_seed(7)
rng = np.random.default_rng(7)
setups = {}
for fs in (2500000, 10000000):
    L, M, T, taps, steps = Tuner.design_nco(fs, OFFSETS)
    n = int(fs * a.seconds) // 8 * 8
    x = 0.3 * torch.randn((n, 2), generator=gen, device=dev, dtype=torch.float32)
    length = n // 12 // 8 * 8
    # three keyings per channel, each a twelfth of the capture, starting on a multiple of 8 samples (case loop hands p25fe_tune_dev
    # a pointer at the keying's first sample, which must be 16-byte aligned in every format), never before sample 8 ceil((T - 1) / 8)
    lead = (T - 1 + 7) // 8 * 8
    cuts = []
    for k in range(K):
        for j in range(PER_CH):
            first = int(rng.integers(lead // 8, (n - length) // 8)) * 8
            cuts.append((first, length, steps[k], 0))
    tn = Tuner.nco(fe, L, M, T, taps, steps)
    ones = [Tuner.nco(fe, L, M, T, taps, [c[2]]) for c in cuts]
    ct = Cuts(tn, cuts)
    full = Cuts(tn, [(0, n, s, 0) for s in steps])
    for f in ("cf32", "u8"):
        t = x if f == "cf32" else torch.clamp(torch.round((x + 1.0) * 127.5), 0, 255).to(torch.uint8)
        setups[(fs, f)] = dict(t=t.contiguous(), tn=tn, ones=ones, ct=ct, full=full, cuts=cuts, T=T, L=L, M=M, n=n,
                               fraction=sum(c[1] for c in cuts) / float(K * n))
    del x

outs = {}
for key, s in setups.items():                                        # the same bits, before anything is timed
    t, tn, ct, full, cuts = s["t"], s["tn"], s["ct"], s["full"], s["cuts"]
    whole, no = tn.tune_dev(t)
    o_cuts = ct.tune_dev(t)
    o_full = full.tune_dev(t)
    assert full.counts == [no] * K and torch.equal(o_full[:, :no].view(torch.int32), whole[:, :no].view(torch.int32)), key
    o_loop = torch.zeros_like(o_cuts)
    for j, c in enumerate(cuts):
        m0 = tn.n_out(0, c[0])
        assert torch.equal(o_cuts[j, :ct.counts[j]].view(torch.int32), whole[j // PER_CH, m0:m0 + ct.counts[j]].view(torch.int32)), (key, j)
        y, nj = s["ones"][j].tune_dev(t[:c[0] + c[1]], n_hist=s["T"] - 1, abs0=c[0], offset=c[0], out=o_loop[j:j + 1])
        assert nj == ct.counts[j]
    assert torch.equal(o_loop.view(torch.int32), o_cuts.view(torch.int32)), key
    outs[key] = (whole, o_cuts, o_full, o_loop)
torch.cuda.synchronize()

cases = {}
for key, s in setups.items():
    name = "%g_%s" % (key[0] / 1e6, key[1])
    whole, o_cuts, o_full, o_loop = outs[key]

    def cuts_(s=s, o=o_cuts):
        s["ct"].tune_dev(s["t"], out=o)

    def whole_(s=s, o=whole):
        s["tn"].tune_dev(s["t"], out=o)

    def full_(s=s, o=o_full):
        s["full"].tune_dev(s["t"], out=o)

    def loop_(s=s, o=o_loop):
        t, T = s["t"], s["T"]
        for j, c in enumerate(s["cuts"]):
            s["ones"][j].tune_dev(t[:c[0] + c[1]], n_hist=T - 1, abs0=c[0], offset=c[0], out=o[j:j + 1])
    cases["cuts_" + name], cases["whole_" + name], cases["full_" + name], cases["loop_" + name] = cuts_, whole_, full_, loop_

for _ in range(3):
    for call in cases.values():
        call()
torch.cuda.synchronize()
ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)] for k in cases}
for r in range(a.reps):
    for k, call in cases.items():
        e0, e1 = ev[k][r]
        e0.record()
        call()
        e1.record()
torch.cuda.synchronize()
res = {"box": a.box, "tag": a.tag, "seconds": a.seconds, "channels": K, "keyings": K * PER_CH, "reps": a.reps, "cases": {}}
for k in cases:
    ms = [e0.elapsed_time(e1) for e0, e1 in ev[k]]
    res["cases"][k] = {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
for key, s in setups.items():
    name = "%g_%s" % (key[0] / 1e6, key[1])
    c, w = res["cases"]["cuts_" + name], res["cases"]["whole_" + name]
    c["fraction_of_channel_time"] = round(s["fraction"], 4)
    c["outputs"], w["outputs"] = int(sum(s["ct"].counts)), int(sum(s["full"].counts))
    c["vs_whole"] = round(c["ms_median"] / w["ms_median"], 3)
    res["cases"]["full_" + name]["vs_whole"] = round(res["cases"]["full_" + name]["ms_median"] / w["ms_median"], 3)
    res["cases"]["loop_" + name]["vs_cuts"] = round(res["cases"]["loop_" + name]["ms_median"] / c["ms_median"], 3)
    res["cases"]["loop_" + name]["launches"] = K * PER_CH
line = json.dumps(res)
print(line, flush=True)
os.makedirs(a.out, exist_ok=True)
with open(os.path.join(a.out, "tune_cuts_time_%s_%s.json" % (a.box, a.tag)), "w") as fh:
    fh.write(line + "\n")
