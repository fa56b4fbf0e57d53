#!/usr/bin/env python3
"""The frequency measure (k_afc_measure, docs/SPEC.md 3.0f) beside p25fe_resample_dev at 1 / D with the same T taps on the same
rows, in one process: the same FIR, which existed before the measure did (it writes its decimated rows; the measure sums products
and writes 32 bytes per row).  K rows of 240 ksps cf32 noise, device-resident -- what the samples are does not matter to a FIR.
Cases: the recommended prefilter (D 10, T 240) with K = 1, 8 and 32 rows, and the limits' corners (D 3, T 7) and (D 64, T 512) with
K = 8.  Every case sits between its own pair of device events and the cases alternate round by round, so a drift of the machine
falls on all of them alike.  Before anything is timed, one range of the measure is compared with the sum over two halves.
Per case: median / min / max in ms, input samples per second, and for the measure its time against the resampler call.
One JSON line, also written to <out>/afc_time_<box>_<tag>.json.
usage: afc_time.py [--samples 8000000] [--reps 20] [--out profiles] [--box NAME] [--tag run1]"""
import argparse, json, os, socket, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from p25rx_amd.frontend import Afc, FrontEnd, Resampler

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=8000000)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
ap.add_argument("--box", default=socket.gethostname())
ap.add_argument("--tag", default="run")
a = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = torch.device("cuda", 0)
n = a.samples // 64 * 64
KMAX = 32
gen = torch.Generator(device=dev)
gen.manual_seed(5)
rows = torch.randn((KMAX, n, 2), generator=gen, device=dev, dtype=torch.float32) * 0.25
SHAPES = ((10, 240, (1, 8, 32)), (3, 7, (8,)), (64, 512, (8,)))
fes = {K: FrontEnd(device=0, n_channels=K) for K in (1, 8, 32)}
out = torch.empty((KMAX, (n // 3 + 8) // 2 * 2, 2), dtype=torch.float32, device=dev)

cases = {}
for D, T, Ks in SHAPES:
    taps = Afc.design(D, T, 240000.0 / D / 3.4)
    for K in Ks:
        afc = Afc(fes[K], K, D, T, taps=taps)
        rs = Resampler(fes[K], 1, D, T, taps)
        acc = afc.new_acc()
        # any split of a range gives the same record
        whole = Afc.records(afc.measure(rows[:K]))
        half = afc.measure(rows[:K], n=n // 2 + 7)
        half = Afc.records(afc.measure(rows[:K], n_hist=T - 1 + D, abs0=n // 2 + 7, offset=n // 2 + 7, acc=half))
        assert (whole == half).all() and int(whole["n"][0]) == n // D, (D, T, K)
        cases["afc_D%d_T%d_K%d" % (D, T, K)] = (lambda afc=afc, K=K, acc=acc: afc.measure(rows[:K], acc=acc), K, D)
        cases["rs_D%d_T%d_K%d" % (D, T, K)] = (lambda rs=rs, K=K: rs.resample_dev(rows[:K], out=out[:K]), K, D)

for _ in range(3):
    for k, (call, _K, _D) in cases.items():
        call()
torch.cuda.synchronize()
ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)] for k in cases}
for r in range(a.reps):
    for k, (call, _K, _D) in cases.items():
        e0, e1 = ev[k][r]
        e0.record()
        call()
        e1.record()
torch.cuda.synchronize()
res = {"box": a.box, "tag": a.tag, "n_samples_per_row": n, "reps": a.reps, "cases": {}}
for k, (_call, K, _D) in cases.items():
    ms = [e0.elapsed_time(e1) for e0, e1 in ev[k]]
    med = statistics.median(ms)
    res["cases"][k] = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                       "gsamples_per_s": round(K * n / med / 1e6, 3)}
for k in list(res["cases"]):
    if k.startswith("afc_"):
        res["cases"][k]["vs_resampler"] = round(res["cases"][k]["ms_median"] / res["cases"]["rs_" + k[4:]]["ms_median"], 3)
line = json.dumps(res)
print(line, flush=True)
os.makedirs(a.out, exist_ok=True)
with open(os.path.join(a.out, "afc_time_%s_%s.json" % (a.box, a.tag)), "w") as fh:
    fh.write(line + "\n")
