#!/usr/bin/env python3
"""What the AFC loop costs (docs/SPEC.md 3.0g): p25fe_track_run_dev over a device-resident 2.5 Msps cf32 capture in 50 ms windows,
beside the same capture through the calls that existed before it -- p25fe_tune_dev + p25fe_afc_measure_dev per window, no update --
and beside ONE whole-range p25fe_tune_dev, in one process, for K = 1, 8 and 32 NCO channels.  Noise, device-resident: what the
samples are does not matter to the tuner or the measure (the loop's gate then rejects most windows, which costs the update kernel
the same launch).  Every case sits between its own pair of device events and the cases alternate round by round, so a drift of the
machine falls on all of them alike (tools/tune_time.py's method).  Before anything is timed, the tracked call is compared with the
same range split in two.
Per case: median / min / max in ms and input samples per second; for the two windowed forms their time against the whole-range call.
One JSON line, also written to <out>/afc_loop_time_<box>_<tag>.json.
usage: afc_loop_time.py [--seconds 2.0] [--reps 20] [--out profiles] [--box NAME] [--tag run1]"""
import argparse, json, os, socket, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from p25rx_amd.frontend import Afc, AfcLoop, FrontEnd, Tuner

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=2.0)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
ap.add_argument("--box", default=socket.gethostname())
ap.add_argument("--tag", default="run")
a = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = torch.device("cuda", 0)
FS, WINDOW = 2500000, 125000
n_win = max(1, int(a.seconds * FS) // WINDOW)
n = n_win * WINDOW
gen = torch.Generator(device=dev)
gen.manual_seed(6)
iq = torch.randn((n, 2), generator=gen, device=dev, dtype=torch.float32) * 0.25
fe = FrontEnd(device=0)

cases = {}
for K in (1, 8, 32):
    offs = [12500.0 * (k - K // 2) + 311.7 for k in range(K)]
    L, M, T, taps, steps = Tuner.design_nco(FS, offs)
    n_out = n * L // M
    out = torch.empty((K, (n_out + 3) // 2 * 2, 2), dtype=torch.float32, device=dev)
    tn, afc = Tuner.nco(fe, L, M, T, taps, steps), Afc(fe, K)
    loop = AfcLoop(tn, afc)
    # any split of a range gives the same rows and states
    loop.tune_tracked_dev(iq, WINDOW, out=out)
    whole, st = out.clone(), loop.read()
    tn2 = Tuner.nco(fe, L, M, T, taps, steps)
    loop2 = AfcLoop(tn2, afc)
    cut = WINDOW // 2 + 8 if n_win == 1 else WINDOW + 4096
    _, no1 = loop2.tune_tracked_dev(iq[:cut], WINDOW, out=out)
    loop2.tune_tracked_dev(iq, WINDOW, n_hist=cut, abs0=cut, offset=cut, out=out, out_offset=no1, n_hist_out=no1)
    assert torch.equal(out[:, :n_out].view(torch.int32), whole[:, :n_out].view(torch.int32)) and (loop2.read() == st).all(), K
    loop2.close()
    tn3 = Tuner.nco(fe, L, M, T, taps, steps)
    acc = afc.new_acc()

    def windows(tn3=tn3, afc=afc, acc=acc, out=out, L=L, M=M):       # the calls of the parent commit: tune + measure per window
        for w in range(n_win):
            a0, o0 = w * WINDOW, w * WINDOW * L // M
            _, no = tn3.tune_dev(iq[:a0 + WINDOW], n_hist=a0, abs0=a0, offset=a0, out=out[:, o0:])
            afc.measure(out, n_hist=min(o0, 249), abs0=o0, offset=o0, n=no, acc=acc)
    cases["tracked_K%d" % K] = (lambda loop=loop, out=out: loop.tune_tracked_dev(iq, WINDOW, out=out), K)
    cases["windows_K%d" % K] = (windows, K)
    cases["whole_K%d" % K] = (lambda tn3=tn3, out=out: tn3.tune_dev(iq, out=out), K)

for _ in range(3):
    for k, (call, _K) in cases.items():
        call()
torch.cuda.synchronize()
ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)] for k in cases}
for r in range(a.reps):
    for k, (call, _K) in cases.items():
        e0, e1 = ev[k][r]
        e0.record()
        call()
        e1.record()
torch.cuda.synchronize()
res = {"box": a.box, "tag": a.tag, "fs": FS, "window": WINDOW, "n_windows": n_win, "n_samples": n, "reps": a.reps, "cases": {}}
for k, (_call, K) in cases.items():
    ms = [e0.elapsed_time(e1) for e0, e1 in ev[k]]
    med = statistics.median(ms)
    res["cases"][k] = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                       "msamples_in_per_s": round(n / med / 1e3, 1)}
for k in list(res["cases"]):
    if not k.startswith("whole_"):
        res["cases"][k]["vs_whole"] = round(res["cases"][k]["ms_median"] / res["cases"]["whole_" + k.split("_")[1]]["ms_median"], 3)
line = json.dumps(res)
print(line, flush=True)
os.makedirs(a.out, exist_ok=True)
with open(os.path.join(a.out, "afc_loop_time_%s_%s.json" % (a.box, a.tag)), "w") as fh:
    fh.write(line + "\n")
