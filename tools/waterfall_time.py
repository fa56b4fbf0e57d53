#!/usr/bin/env python3
"""The survey over time (k_waterfall, docs/SPEC.md 3.0i) beside the survey it is built from (k_scan, 3.0h, whose code it shares), in
one process, on tools/scan_time.py's device-resident captures of --seconds (2) at 2.5 and 10 Msps held as cf32 and u8.  N = 4096,
hop 2048, the designed window, shift 16.  Cases, per rate and format, with slots of about 10 ms and about 100 ms (a whole number
of frames):
  wf     p25fe_waterfall_dev over the whole capture into zeroed rows: ONE launch;
  scan   p25fe_scan_dev over the whole capture into a zeroed record: the same bytes and the same arithmetic, the reference for what
         the per-slot delivery costs (one round of atomics per slot and workgroup instead of one per workgroup);
  loop   what a caller writes without the new call: one p25fe_scan_dev per slot, each into its own zeroed row.
Before anything is timed the three are compared bit for bit: the loop's rows are the waterfall's, and their wrapping sum is the
record.  Every case sits between its own pair of device events and the cases alternate round by round, so a drift of the machine
falls on all of them alike.  Per case: median / min / max in ms; for wf its time against scan and the loop's time against wf.
One JSON line, also written to <out>/waterfall_time_<box>_<tag>.json.
usage: waterfall_time.py [--seconds 2] [--reps 20] [--out profiles] [--box NAME] [--tag run1]"""
import argparse, json, os, socket, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from p25rx_amd import Scanner
from p25rx_amd.frontend import FrontEnd

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=2.0)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
ap.add_argument("--box", default=socket.gethostname())
ap.add_argument("--tag", default="run")
a = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = torch.device("cuda", 0)
N, HOP, SHIFT = 4096, 2048, 16
SLOTS_MS = (10, 100)
fe = FrontEnd(device=0)
sc = Scanner(fe, N, HOP, shift=SHIFT)

caps = {}
gen = torch.Generator(device=dev)
gen.manual_seed(7)
for fs in (2500000, 10000000):
    n = int(fs * a.seconds) // HOP * HOP
    x = 0.15 * torch.randn((n, 2), generator=gen, device=dev, dtype=torch.float32)
    ph = 2.0 * np.pi * 0.0371 * torch.arange(n, device=dev, dtype=torch.float64)
    x += 0.3 * torch.stack([torch.cos(ph), torch.sin(ph)], dim=1).to(torch.float32)
    caps[(fs, "cf32")] = x.contiguous()
    caps[(fs, "u8")] = torch.clamp(torch.round((x + 1.0) * 127.5), 0, 255).to(torch.uint8).contiguous()
    del x, ph


def slot_frames(fs, ms):
    return max(1, int(round(ms * fs / 1000.0 / HOP)))


def loop(t, B, rows):
    """one p25fe_scan_dev per slot into its own row: slot s owns the samples [s B HOP, (s + 1) B HOP)"""
    n, step = t.shape[0], B * HOP
    for s in range(rows.shape[0]):
        at = s * step
        sc.scan_dev(t, n_hist=min(at, N - 1), abs0=at, offset=at, n=min(step, n - at), acc=rows[s])


acc = torch.zeros(N + 1, dtype=torch.int64, device=dev)
rows = {}
for (fs, f), t in caps.items():                                      # the same words, before anything is timed
    acc.zero_()
    sc.scan_dev(t, acc=acc)
    frames = t.shape[0] // HOP
    assert int(acc[N]) == frames
    for ms in SLOTS_MS:
        B = slot_frames(fs, ms)
        r = rows[(fs, f, ms)] = torch.zeros((-(-frames // B), N + 1), dtype=torch.int64, device=dev)
        sc.waterfall_dev(t, B, rows=r, slot0=0)
        assert torch.equal(r.sum(dim=0), acc), (fs, f, ms)           # (int64 sums wrap as the uint64 words do)
        by_loop = torch.zeros_like(r)
        loop(t, B, by_loop)
        assert torch.equal(by_loop, r), (fs, f, ms)
        del by_loop
torch.cuda.synchronize()

cases = {}
for (fs, f), t in caps.items():
    name = "%g_%s" % (fs / 1e6, f)

    def scan(t=t):
        acc.zero_()
        sc.scan_dev(t, acc=acc)
    cases["scan_" + name] = scan
    for ms in SLOTS_MS:
        def wf(t=t, B=slot_frames(fs, ms), r=rows[(fs, f, ms)]):
            r.zero_()
            sc.waterfall_dev(t, B, rows=r, slot0=0)

        def lp(t=t, B=slot_frames(fs, ms), r=rows[(fs, f, ms)]):
            r.zero_()
            loop(t, B, r)
        cases["wf%d_%s" % (ms, name)] = wf
        cases["loop%d_%s" % (ms, name)] = lp

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
res = {"box": a.box, "tag": a.tag, "seconds": a.seconds, "N": N, "hop": HOP, "reps": a.reps, "cases": {}}
for k in cases:
    ms = [e0.elapsed_time(e1) for e0, e1 in ev[k]]
    res["cases"][k] = {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
for (fs, f), t in caps.items():
    name = "%g_%s" % (fs / 1e6, f)
    for ms in SLOTS_MS:
        w, lp = res["cases"]["wf%d_%s" % (ms, name)], res["cases"]["loop%d_%s" % (ms, name)]
        w["slot_frames"], w["n_slots"] = slot_frames(fs, ms), rows[(fs, f, ms)].shape[0]
        w["vs_scan"] = round(w["ms_median"] / res["cases"]["scan_" + name]["ms_median"], 3)
        lp["vs_wf"] = round(lp["ms_median"] / w["ms_median"], 3)
        lp["launches"] = w["n_slots"]
line = json.dumps(res)
print(line, flush=True)
os.makedirs(a.out, exist_ok=True)
with open(os.path.join(a.out, "waterfall_time_%s_%s.json" % (a.box, a.tag)), "w") as fh:
    fh.write(line + "\n")
