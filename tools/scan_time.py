#!/usr/bin/env python3
"""The survey (k_scan, docs/SPEC.md 3.0h) beside two yardsticks in one process, on device-resident captures of --seconds (2) at 2.5
and 10 Msps held as cf32 and u8 (seeded noise and a tone; what the samples are does not matter to a DFT).  N = 4096, hop 2048, the
designed window, shift 16.  Cases, per rate and format:
  scan   p25fe_scan_dev over the whole capture into a zeroed record;
  copy   torch's device-to-device copy of the same input bytes: the roofline the README uses (it moves every byte twice, the survey
         reads each once);
  torch  the same Welch sum as a user of this project's plumbing would write it today: (u8: the conversion,) unfold into frames,
         window, torch.fft.fft, |X|^2, sum over the frames in fp32.
Before anything is timed the survey's record is compared with torch's sums (fp32 sums of thousands of frames: 1e-3 of the largest).
Every case sits between its own pair of device events and the cases alternate round by round, so a drift of the machine falls on
all of them alike.  Per case: median / min / max in ms; for scan its time against copy and against torch, and the input bytes per
second of the median.
One JSON line, also written to <out>/scan_time_<box>_<tag>.json.
usage: scan_time.py [--seconds 2] [--reps 20] [--out profiles] [--box NAME] [--tag run1]"""
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
fe = FrontEnd(device=0)
sc = Scanner(fe, N, HOP, shift=SHIFT)
win = torch.from_numpy(Scanner.design(N)).to(dev)
u8_scale, u8_offset = float(fe.cfg.u8_scale), float(fe.cfg.u8_offset)

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


def welch_torch(t):
    """the record's bins as fp32 sums, the frames of a stream that starts at position 0 (N - HOP zeros in front of it)"""
    x = t if t.dtype == torch.float32 else t.to(torch.float32) * u8_scale + u8_offset
    z = torch.view_as_complex(torch.cat([torch.zeros((N - HOP, 2), dtype=torch.float32, device=dev), x]))
    X = torch.fft.fft(z.unfold(0, N, HOP) * win, dim=1)
    return (X.real * X.real + X.imag * X.imag).sum(dim=0)


acc = torch.zeros(N + 1, dtype=torch.int64, device=dev)
dst = {k: torch.empty_like(t) for k, t in caps.items()}
for k, t in caps.items():                                            # the same sums, before anything is timed
    acc.zero_()
    sc.scan_dev(t, acc=acc)
    got = acc[:N].to(torch.float64) * 2.0 ** -SHIFT
    ref = welch_torch(t).to(torch.float64)
    assert int(acc[N]) == t.shape[0] // HOP, k
    assert float((got - ref).abs().max()) <= 1e-3 * float(ref.max()), (k, float((got - ref).abs().max()), float(ref.max()))
torch.cuda.synchronize()

cases = {}
for (fs, f), t in caps.items():
    name = "%g_%s" % (fs / 1e6, f)

    def scan(t=t):
        acc.zero_()
        sc.scan_dev(t, acc=acc)
    cases["scan_" + name] = scan
    cases["copy_" + name] = lambda t=t, d=dst[(fs, f)]: d.copy_(t)
    cases["torch_" + name] = lambda t=t: welch_torch(t)

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
    s = res["cases"]["scan_" + name]
    s["vs_copy"] = round(s["ms_median"] / res["cases"]["copy_" + name]["ms_median"], 3)
    s["vs_torch"] = round(s["ms_median"] / res["cases"]["torch_" + name]["ms_median"], 3)
    s["input_gb_per_s"] = round(t.numel() * t.element_size() / s["ms_median"] / 1e6, 1)
    s["capture_seconds_per_second"] = round(a.seconds / (s["ms_median"] / 1e3), 1)
line = json.dumps(res)
print(line, flush=True)
os.makedirs(a.out, exist_ok=True)
with open(os.path.join(a.out, "scan_time_%s_%s.json" % (a.box, a.tag)), "w") as fh:
    fh.write(line + "\n")
