#!/usr/bin/env python3
"""The rational resampler (k_resample, docs/SPEC.md 3.0b) beside K0 in one process, on one device-resident capture of at least 1e8
samples (bench.py's recipe: seeded C4FM at 240 ksps, zero-order hold x 10; what the samples are does not matter to a FIR), held as
cf32, s16 and u8.  Cases:
  (i)   L/M/T = 1/10/80 with SPEC 3.0's taps -- the same arithmetic as K0 -- beside p25fe_predecim_dev, for cf32, s16 and u8;
  (ii)  12/125 (2.5 Msps) and 15/128 (2.048 Msps) with the designed tables, cf32 and s16;
  (iii) 3/250 (20 Msps), T = 667, cf32.
Every call sits between its own pair of device events and the cases alternate call by call, so a drift of the machine falls on all
of them alike; run the tool more than once (one process each) and compare the medians.  Before anything is timed, case (i)'s output
is compared bit for bit with K0's.  Per case: median / min / max of the kernel time in ms and the input bytes per second.
One JSON line, also written to <out>/resample_time_<box>_<tag>.json.
usage: resample_time.py [--samples 120000000] [--reps 20] [--out profiles] [--box NAME] [--tag run1]"""
import argparse, json, os, socket, statistics, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from p25rx_amd import c4fm
from p25rx_amd.frontend import FrontEnd, Resampler

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=120000000)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"))
ap.add_argument("--box", default=socket.gethostname())
ap.add_argument("--tag", default="run")
a = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = torch.device("cuda", 0)
n240 = a.samples // 80 * 8
iq240, _ = c4fm.synth_torch(n240, seed=31, device=dev, snr_db=30.0)
wide = iq240[:n240].repeat_interleave(10, dim=0).contiguous()
del iq240
n = wide.shape[0]
BPS = {"cf32": 8, "s16": 4, "u8": 2}
caps = {"cf32": wide,
        "s16": torch.clamp(torch.round(wide * 32767.0), -32768, 32767).to(torch.int16),
        "u8": torch.clamp(torch.round((wide + 1.0) * 127.5), 0, 255).to(torch.uint8)}
fe = FrontEnd(device=0)
spec = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "spec.json")))
rs_k0 = Resampler(fe, 1, 10, 80, np.array(spec["pre_taps"], dtype=np.float32))
designed = {}
for fs in (2500000, 2048000, 20000000):
    L, M, T, taps = Resampler.design(fs)
    designed["%d/%d" % (L, M)] = (Resampler(fe, L, M, T, taps), T)

for f in caps:                                                       # case (i) IS K0
    y, no = rs_k0.resample_dev(caps[f])
    yk, nk = fe.predecim_dev(caps[f])
    assert no == nk and torch.equal(y[:, :no].view(torch.int32), yk[:, :nk].view(torch.int32)), "1/10/80 differs from K0 on %s" % f
    del y, yk
torch.cuda.synchronize()

cases = {}                                                           # name -> (call(out) -> (out, n_out), input format)
for f in caps:
    cases["k0_" + f] = (lambda o, f=f: fe.predecim_dev(caps[f], out=o), f)
    cases["rs_1/10_T80_" + f] = (lambda o, f=f: rs_k0.resample_dev(caps[f], out=o), f)
for name, (rs, T) in designed.items():
    for f in (("cf32", "s16") if name != "3/250" else ("cf32",)):
        cases["rs_%s_T%d_%s" % (name, T, f)] = (lambda o, rs=rs, f=f: rs.resample_dev(caps[f], out=o), f)

outs = {k: None for k in cases}
for _ in range(3):
    for k, (call, _f) in cases.items():
        outs[k], _ = call(outs[k])
torch.cuda.synchronize()
ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)] for k in cases}
for r in range(a.reps):
    for k, (call, _f) in cases.items():
        e0, e1 = ev[k][r]
        e0.record()
        call(outs[k])
        e1.record()
torch.cuda.synchronize()
res = {"box": a.box, "tag": a.tag, "n_samples": n, "reps": a.reps, "cases": {}}
for k, (_call, f) in cases.items():
    ms = [e0.elapsed_time(e1) for e0, e1 in ev[k]]
    med = statistics.median(ms)
    res["cases"][k] = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                       "input_GBps": round(BPS[f] * n / (med * 1e-3) / 1e9, 1)}
for f in caps:
    res["cases"]["rs_1/10_T80_" + f]["vs_k0"] = round(res["cases"]["rs_1/10_T80_" + f]["ms_median"] / res["cases"]["k0_" + f]["ms_median"], 3)
line = json.dumps(res)
print(line, flush=True)
os.makedirs(a.out, exist_ok=True)
with open(os.path.join(a.out, "resample_time_%s_%s.json" % (a.box, a.tag)), "w") as fh:
    fh.write(line + "\n")
