#!/usr/bin/env python3
"""K0 (pre-decimator) and K6 (channeliser) on cf32, s16 and u8 input in one process, on configs[2]'s shape: one channel of
60 s at 2.4 Msps = 1.44e8 samples, generated once (bench.py's recipe: seeded C4FM at 240 ksps, zero-order hold x 10) and held
in all three formats.  Every kernel call sits between its own pair of device events; the formats alternate call by call
(cf32, s16, u8, cf32, ...), so a drift of the machine falls on all of them alike.  Before anything is timed the narrow outputs
are compared bit for bit with the cf32 kernel's output on the converted samples.
Per stage and format: median / min / max of the kernel time, achieved bytes per second over the algorithmic bytes
(K0: sample bytes + 0.8 B written per input sample; K6: sample bytes + 153.6 B), and the one condition of the feature:
a narrow format's median may exceed the cf32 median of the same run by no more than that run's spread (max - min) of the cf32 time.
One JSON line, also written to <out>/wide_fmt_time_<box>.json.
usage: wide_fmt_time.py [--seconds 60] [--reps-k0 30] [--reps-k6 8] [--out profiles] [--box NAME]"""
import argparse, json, os, socket, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from p25rx_amd import c4fm
from p25rx_amd.frontend import FrontEnd

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=60.0)
ap.add_argument("--reps-k0", type=int, default=30)
ap.add_argument("--reps-k6", type=int, default=8)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"))
ap.add_argument("--box", default=socket.gethostname())
a = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = torch.device("cuda", 0)
n240 = int(a.seconds * 240000) // 8 * 8
iq240, _ = c4fm.synth_torch(n240, seed=31, device=dev, snr_db=30.0)
wide = iq240[:n240].repeat_interleave(10, dim=0).contiguous()
del iq240
n = wide.shape[0]
BPS = {"cf32": 8, "s16": 4, "u8": 2}
caps = {"cf32": wide,
        "s16": torch.clamp(torch.round(wide * 32767.0), -32768, 32767).to(torch.int16),
        "u8": torch.clamp(torch.round((wide + 1.0) * 127.5), 0, 255).to(torch.uint8)}
fe = FrontEnd(device=0)

# the narrow outputs ARE the cf32 kernel's on the converted samples (whole capture for K0, the first 1e6 samples for K6)
nc = min(n, 1000000) // 8 * 8
for f in ("s16", "u8"):
    if f == "s16":
        cv = caps[f].to(torch.float32) * (2.0 ** -15)
    else:
        scale = float(torch.tensor(2.0 / 255.0, dtype=torch.float32))     # SPEC 3.1's numbers; in float64 the product and the sum
        cv = (caps[f].to(torch.float64) * scale - 1.0).to(torch.float32)  # are exact, so this is fmaf((float)b, 2/255, -1)
    y, no = fe.predecim_dev(caps[f])
    yc, _ = fe.predecim_dev(cv)
    assert torch.equal(y[:, :no].view(torch.int32), yc[:, :no].view(torch.int32)), "K0 %s differs from cf32 on the converted samples" % f
    z, nz = fe.channelise_dev(caps[f][:nc])
    zc, _ = fe.channelise_dev(cv[:nc])
    assert torch.equal(z[:, :nz].contiguous().view(torch.int32), zc[:, :nz].contiguous().view(torch.int32)), \
        "K6 %s differs from cf32 on the converted samples" % f
    del cv, y, yc, z, zc
torch.cuda.synchronize()


def interleaved(call, reps, warm):
    """{format: [ms per call]}: `reps` rounds of (cf32, s16, u8), each call between its own events"""
    out = None
    for _ in range(warm):
        for f in caps:
            out, _ = call(caps[f], out)
    torch.cuda.synchronize()
    ev = {f: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for f in caps}
    for r in range(reps):
        for f in caps:
            e0, e1 = ev[f][r]
            e0.record()
            out, _ = call(caps[f], out)
            e1.record()
    torch.cuda.synchronize()
    del out
    return {f: [e0.elapsed_time(e1) for e0, e1 in ev[f]] for f in caps}


def report(ms, out_bytes):
    med = {f: statistics.median(v) for f, v in ms.items()}
    spread = max(ms["cf32"]) - min(ms["cf32"])
    rep = {}
    for f, v in ms.items():
        rep[f] = {"ms_median": round(med[f], 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                  "bytes_per_input_sample": round(BPS[f] + out_bytes, 2),
                  "achieved_GBps": round((BPS[f] + out_bytes) * n / (med[f] * 1e-3) / 1e9, 1),
                  "vs_cf32": round(med[f] / med["cf32"], 4)}
    rep["cf32_spread_ms"] = round(spread, 4)
    rep["narrow_within_cf32_spread"] = {f: bool(med[f] <= med["cf32"] + spread) for f in ("s16", "u8")}
    return rep


res = {"box": a.box, "seconds": a.seconds, "n_samples": n, "reps": {"k0": a.reps_k0, "k6": a.reps_k6},
       "lib": os.path.basename(os.environ.get("P25FE_LIB", "libp25fe.so"))}
res["k_predecim"] = report(interleaved(lambda t, o: fe.predecim_dev(t, out=o), a.reps_k0, 3), 0.8)
res["k_channelise"] = report(interleaved(lambda t, o: fe.channelise_dev(t, out=o), a.reps_k6, 2), 192 * 8 / 10.0)
line = json.dumps(res)
print(line, flush=True)
os.makedirs(a.out, exist_ok=True)
with open(os.path.join(a.out, "wide_fmt_time_%s.json" % a.box), "w") as fh:
    fh.write(line + "\n")
