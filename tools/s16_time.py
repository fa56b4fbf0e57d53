#!/usr/bin/env python3
"""s16 beside cf32 and u8 in one process, on configs[1]'s 600 s capture generated once and held in all three formats:
K1 alone (its own dispatch events, as bench.py reads them), the pipelined step (interleaved, median of 20 after a 150 ms settle)
and p25fe_run_host_windows for cf32 and s16 beside the host-to-device copy rate measured here.  The s16 dibits are checked against
the cf32 dibits of the converted capture before anything is printed.  One JSON line, also written to <out>/s16_time_<box>.json.
usage: s16_time.py [--seconds 600] [--out profiles] [--box NAME]      (P25FE_LIB / P25FE_SUBS: measurement builds and knobs)"""
import argparse, json, os, socket, statistics, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from p25rx_amd import c4fm
from p25rx_amd.frontend import FrontEnd, parse_results

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=600.0)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"))
ap.add_argument("--box", default=socket.gethostname())
ap.add_argument("--no-windows", action="store_true", help="skip the host-window part (kernel A/B runs)")
a = ap.parse_args()
dev = torch.device("cuda", 0)
n = int(a.seconds * 240000) // 8 * 8
iq, _ = c4fm.synth_torch(n, seed=1003, device=dev, snr_db=30.0)
iq = iq[:n].contiguous()
caps = {"s16": torch.clamp(torch.round(iq * 32767.0), -32768, 32767).to(torch.int16),
        "u8": torch.clamp(torch.round((iq + 1.0) * 127.5), 0, 255).to(torch.uint8)}
caps["cf32"] = iq
conv = caps["s16"].to(torch.float32) * (2.0 ** -15)                   # the cf32 stream the s16 capture IS
fe = FrontEnd()
outs = {f: fe.run_dev(t) for f, t in caps.items()}
dc, rc = FrontEnd().run_dev(conv)
torch.cuda.synchronize()
nd = int(parse_results(rc)[0]["n_dibits"])
assert parse_results(outs["s16"][1])[0].tobytes() == parse_results(rc)[0].tobytes() and torch.equal(outs["s16"][0][0, :nd], dc[0, :nd]), \
    "s16 dibits differ from the cf32 dibits of the converted capture"
del conv, dc, rc
res = {"box": a.box, "seconds": a.seconds, "n_samples": n, "n_dibits_s16": nd, "subs_env": os.environ.get("P25FE_SUBS", ""),
       "lib": os.path.basename(os.environ.get("P25FE_LIB", "libp25fe.so"))}

# K1 alone: events attached to its own dispatch, 40 calls per format, three interleaved rounds
k1 = {f: [] for f in caps}
for f, t in caps.items():
    for _ in range(20):
        fe.run_dev(t, dibits=outs[f][0], result=outs[f][1])
torch.cuda.synchronize()
fe.profile_enable(2)
for rnd in range(3):
    for f, t in caps.items():
        fe.profile_read()
        for _ in range(40):
            fe.run_dev(t, dibits=outs[f][0], result=outs[f][1])
        torch.cuda.synchronize()
        ms, calls = fe.profile_read()
        k1[f].append(ms[0] / max(calls, 1))
fe.profile_enable(0)
res["k1_ms"] = {f: [round(v, 5) for v in k1[f]] for f in k1}

# pipelined step, interleaved, median of 20 measurements of 50 steps each after a 150 ms settle
step = {f: [] for f in caps}
for f, t in caps.items():
    for _ in range(100):
        fe.run_dev_pipelined(t, dibits=outs[f][0], result=outs[f][1])
fe.join_dev(); torch.cuda.synchronize()
for rnd in range(20):
    for f, t in caps.items():
        for _ in range(10):
            fe.run_dev_pipelined(t, dibits=outs[f][0], result=outs[f][1])
        fe.join_dev(); torch.cuda.synchronize()
        time.sleep(0.15)
        t0 = time.perf_counter()
        for _ in range(50):
            fe.run_dev_pipelined(t, dibits=outs[f][0], result=outs[f][1])
        fe.join_dev(); torch.cuda.synchronize()
        step[f].append((time.perf_counter() - t0) / 50 * 1e3)
res["step_ms_median"] = {f: round(statistics.median(v), 5) for f, v in step.items()}
res["step_ms_min_max"] = {f: [round(min(v), 5), round(max(v), 5)] for f, v in step.items()}

if not a.no_windows:
    # the bus: pinned host -> device copy of the cf32 capture, best of 5
    host = {f: caps[f].cpu().pin_memory() for f in ("cf32", "s16")}
    dst = torch.empty_like(caps["cf32"])
    best = 1e9
    for _ in range(5):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        dst.copy_(host["cf32"], non_blocking=True); torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    h2d = host["cf32"].numel() * 4 / best
    res["h2d_GBps"] = round(h2d / 1e9, 2)
    del dst
    win = {}
    for f in ("cf32", "s16", "cf32", "s16", "cf32", "s16"):
        w = FrontEnd()
        eb = 8 if f == "cf32" else 4
        d, st = w.run_host_windows(host[f])
        assert len(d) == nd or f == "cf32"
        sps = n / (st["ms_total"] * 1e-3)
        win.setdefault(f, []).append(dict(Msps=round(sps / 1e6, 1), bus_fraction=round(sps * eb / h2d, 3), ms_total=round(st["ms_total"], 2),
                                          ms_h2d=round(st["ms_h2d"], 2), ms_compute=round(st["ms_compute"], 2), n_windows=st["n_windows"]))
        w.close()
    res["windows"] = win
line = json.dumps(res)
print(line, flush=True)
os.makedirs(a.out, exist_ok=True)
with open(os.path.join(a.out, "s16_time_%s.json" % a.box), "w") as fh:
    fh.write(line + "\n")
