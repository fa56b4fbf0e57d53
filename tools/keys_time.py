#!/usr/bin/env python3
"""The keys computed on the device (docs/SPEC.md 3.0k) beside the route they replace, in one process, by tools/waterfall_time.py's
method, on the rows of its four captures (--seconds (2) at 2.5 and 10 Msps held as cf32 and u8; N = 4096, hop 2048, the designed
window, shift 16) at slots of about 10 ms: 204 / 200 rows of 4097 words.  The rule's parameters are the recommended ones.  Those
captures hold one steady tone that lies between two raster channels, so their rows yield no key: both routes do all the work of
the rule and have nothing to deliver.  A fifth capture is therefore added to them, none replaced: 2.5 Msps cf32 with the tone on
raster channel 8, keyed in five bursts of 0.1 to 0.3 s ("2.5_cf32_keyed").  Cases, per capture:
  host     what a caller does without the new calls, and the yardstick (this route is unchanged): the rows copied to the host
           (pageable memory), then Scanner.keys (p25fe_waterfall_keys);
  dev      Keys.run_dev + Keys.read: four launches, then the raw records copied back and finished;
  kernels  Keys.run_dev alone, between two device events.
host and dev contain host work, so both are wall-clock times from a synchronised start to the moment the keys are in host memory;
kernels is device time.  Before anything is timed the two routes' keys are compared byte for byte.  The cases alternate round by
round, so a drift of the machine falls on all of them alike; 3 warm-up rounds.  Per case: median / min / max in ms; per capture
dev / host and kernels / dev.  One JSON line, also written to <out>/keys_time_<box>_<tag>.json.
Not measured here: a caller in C (both routes then lose the interpreter's share), and pinned host rows for the host route.
usage: keys_time.py [--seconds 2] [--reps 20] [--out profiles] [--box NAME] [--tag run1]"""
import argparse, json, os, socket, statistics, sys, time
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
N, HOP, SHIFT, SLOT_MS = 4096, 2048, 16, 10
fe = FrontEnd(device=0)
sc = Scanner(fe, N, HOP, shift=SHIFT)

rows, plans, n_keys = {}, {}, {}
gen = torch.Generator(device=dev)
gen.manual_seed(7)
for fs in (2500000, 10000000):                                       # tools/waterfall_time.py's captures
    n = int(fs * a.seconds) // HOP * HOP
    x = 0.15 * torch.randn((n, 2), generator=gen, device=dev, dtype=torch.float32)
    ph = 2.0 * np.pi * 0.0371 * torch.arange(n, device=dev, dtype=torch.float64)
    x += 0.3 * torch.stack([torch.cos(ph), torch.sin(ph)], dim=1).to(torch.float32)
    B = max(1, int(round(SLOT_MS * fs / 1000.0 / HOP)))
    for f, t in (("cf32", x.contiguous()), ("u8", torch.clamp(torch.round((x + 1.0) * 127.5), 0, 255).to(torch.uint8).contiguous())):
        name = "%g_%s" % (fs / 1e6, f)
        rows[name] = sc.waterfall_dev(t, B)
        plans[name] = sc.keys_plan(fs, max_rows=rows[name].shape[0], max_keys=1024)
    if fs == 2500000:                                                # the added capture: the tone on channel 8 (100 kHz), five bursts
        gate = torch.zeros(n, device=dev, dtype=torch.float32)
        for s0, s1 in ((10, 40), (60, 90), (100, 130), (150, 160), (170, 200)):
            gate[s0 * B * HOP:s1 * B * HOP] = 1.0
        ph = 2.0 * np.pi * 0.04 * torch.arange(n, device=dev, dtype=torch.float64)
        x += (0.3 * gate[:, None]) * (torch.stack([torch.cos(ph), torch.sin(ph)], dim=1).to(torch.float32) -
                                      torch.stack([torch.cos(ph * (0.0371 / 0.04)), torch.sin(ph * (0.0371 / 0.04))], dim=1).to(torch.float32))
        rows["2.5_cf32_keyed"] = sc.waterfall_dev(x.contiguous(), B)
        plans["2.5_cf32_keyed"] = sc.keys_plan(fs, max_rows=rows["2.5_cf32_keyed"].shape[0], max_keys=1024)
        del gate
    del x, ph


def host(name):
    return Scanner.keys(rows[name].cpu().numpy(), FS[name])


def on_device(name):
    plans[name].run_dev(rows[name])
    return plans[name].read()


FS = {name: (2500000 if name.startswith("2.5") else 10000000) for name in rows}
for name in rows:                                                    # the same bytes, before anything is timed
    ref, got = host(name), on_device(name)
    assert len(got) == len(ref), (name, len(got), len(ref))
    assert got.tobytes() == ref.tobytes(), (name, got, ref)
    assert len(ref) >= 5 or not name.endswith("keyed"), (name, ref)
    n_keys[name] = len(ref)

wall = {"host": host, "dev": on_device}
ms = {"%s_%s" % (k, name): [] for k in ("host", "dev", "kernels") for name in rows}
for r in range(3 + a.reps):
    for name in rows:
        for k, call in wall.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(name)
            t1 = time.perf_counter()
            ms["%s_%s" % (k, name)].append((t1 - t0) * 1e3)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        plans[name].run_dev(rows[name])
        e1.record()
        torch.cuda.synchronize()
        ms["kernels_" + name].append(e0.elapsed_time(e1))
res = {"box": a.box, "tag": a.tag, "seconds": a.seconds, "N": N, "hop": HOP, "reps": a.reps, "warmup": 3, "slot_ms": SLOT_MS, "cases": {}}
for k, v in ms.items():
    v = v[3:]
    res["cases"][k] = {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
for name in rows:
    d, h, kn = (res["cases"]["%s_%s" % (k, name)] for k in ("dev", "host", "kernels"))
    d["n_rows"], d["n_keys"] = rows[name].shape[0], n_keys[name]
    d["vs_host"] = round(d["ms_median"] / h["ms_median"], 4)
    kn["vs_dev"] = round(kn["ms_median"] / d["ms_median"], 4)
line = json.dumps(res)
print(line, flush=True)
os.makedirs(a.out, exist_ok=True)
with open(os.path.join(a.out, "keys_time_%s_%s.json" % (a.box, a.tag)), "w") as fh:
    fh.write(line + "\n")
