#!/usr/bin/env python3
"""The tuner (k_tune, docs/SPEC.md 3.0c) beside the resampler and the channeliser in one process, on tools/resample_time.py's
device-resident capture (at least 1e8 samples, held as cf32, s16 and u8; what the samples are does not matter to a mixer and a FIR).
Cases, per input format:
  (i)   2.5 Msps (12/125, designed table, channels on the 12.5 kHz raster: den 200) and 2.048 Msps (15/128, den 4096): the tuner with
        K = 1, 8 and 32 channels, beside K calls of p25fe_resample_dev on the same capture -- which tune nothing, but are the only
        path to K rows that the library had before, and move the same bytes; and the tuner of NCO channels (k_tune_nco, SPEC
        3.0d) with the same K at p25fe_nco_step of the same offsets, beside the rational tuner;
  (ii)  2.4 Msps (1/10, T = 80, SPEC 3.0's taps, den 192): the tuner with K = 32 beside p25fe_channelise_dev (all 192 channels of the
        raster) on the capture's first fifth (the channeliser's 192 rows of the whole capture would not be a fair buffer to hold).
Every case sits between its own pair of device events and the cases alternate round by round, so a drift of the machine falls on
all of them alike.  Before anything is timed, the centre channel of every tuner is compared bit for bit with the resampler's output.
Per case: median / min / max in ms, ms per channel, for the tuner its time against K resampler calls and for the NCO tuner its time
against the rational tuner of the same K.
One JSON line, also written to <out>/tune_time_<box>_<tag>.json.
usage: tune_time.py [--samples 120000000] [--reps 20] [--out profiles] [--box NAME] [--tag run1]"""
import argparse, json, os, socket, statistics, sys
from math import gcd
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from p25rx_amd import c4fm
from p25rx_amd.frontend import FrontEnd, Resampler, Tuner

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=120000000)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
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
caps = {"cf32": wide,
        "s16": torch.clamp(torch.round(wide * 32767.0), -32768, 32767).to(torch.int16),
        "u8": torch.clamp(torch.round((wide + 1.0) * 127.5), 0, 255).to(torch.uint8)}
fe = FrontEnd(device=0)
KS = (1, 8, 32)


def raster(fs, K):
    """K channels 12.5 kHz apart around the centre, the centre first"""
    return [Tuner.freq(fs, 12500 * ((k + 1) // 2) * (-1 if k % 2 else 1)) for k in range(K)]


def raster_nco(fs, K):
    """the same offsets as steps of the NCO"""
    return [Tuner.nco_step(fs, 12500.0 * ((k + 1) // 2) * (-1 if k % 2 else 1)) for k in range(K)]


rates, ncos = {}, {}
for fs in (2500000, 2048000):
    L, M, T, taps = Resampler.design(fs)
    rates["%d/%d" % (L, M)] = (Resampler(fe, L, M, T, taps), {K: Tuner(fe, L, M, T, taps, raster(fs, K)) for K in KS}, L, M)
    ncos["%d/%d" % (L, M)] = {K: Tuner.nco(fe, L, M, T, taps, raster_nco(fs, K)) for K in KS}
spec = json.load(open(os.path.join(ROOT, "tests", "golden", "spec.json")))
pre = np.array(spec["pre_taps"], dtype=np.float32)
tn24 = Tuner(fe, 1, 10, 80, pre, raster(2400000, 32))
n5 = n // 40 * 8

# one output buffer for every case: 32 rows of the longest row any of them writes (the stream orders the calls)
rows = max(n * L // M for _rs, _tn, L, M in rates.values()) + 8
out = torch.empty((32, rows // 2 * 2, 2), dtype=torch.float32, device=dev)
out_chz = None

for name, (rs, tns, L, M) in rates.items():                          # the centre channel IS the resampler
    for f in caps:
        y, no = tns[8].tune_dev(caps[f], out=out[:8])
        r, nr = rs.resample_dev(caps[f])
        assert no == nr and torch.equal(y[0, :no].view(torch.int32), r[0, :nr].view(torch.int32)), (name, f)
        assert not torch.equal(y[1, :no].view(torch.int32), r[0, :nr].view(torch.int32)), (name, f)
        z, nz = ncos[name][8].tune_dev(caps[f], out=out[8:16])         # ... and so is the NCO's
        assert nz == nr and torch.equal(z[0, :nz].view(torch.int32), r[0, :nr].view(torch.int32)), (name, f)
        assert not torch.equal(z[1, :nz].view(torch.int32), r[0, :nr].view(torch.int32)), (name, f)
        del r
torch.cuda.synchronize()

cases = {}                                                           # name -> (call, channels)
for name, (rs, tns, L, M) in rates.items():
    for f in caps:
        for K in KS:
            cases["tune_%s_K%d_%s" % (name, K, f)] = (lambda tn=tns[K], f=f, K=K: tn.tune_dev(caps[f], out=out[:K]), K)
            cases["nco_%s_K%d_%s" % (name, K, f)] = (lambda tn=ncos[name][K], f=f, K=K: tn.tune_dev(caps[f], out=out[:K]), K)

            def k_calls(rs=rs, f=f, K=K):
                for k in range(K):
                    rs.resample_dev(caps[f], out=out[k:k + 1])
            cases["rs_x%d_%s_%s" % (K, name, f)] = (k_calls, K)
for f in caps:
    cases["tune_1/10_K32_fifth_%s" % f] = (lambda f=f: tn24.tune_dev(caps[f][:n5], out=out), 32)

    def chz(f=f):
        global out_chz
        out_chz, _ = fe.channelise_dev(caps[f][:n5], out=out_chz)
    cases["channelise_192_fifth_%s" % f] = (chz, 192)

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
res = {"box": a.box, "tag": a.tag, "n_samples": n, "n_fifth": n5, "reps": a.reps, "cases": {}}
for k, (_call, K) in cases.items():
    ms = [e0.elapsed_time(e1) for e0, e1 in ev[k]]
    med = statistics.median(ms)
    res["cases"][k] = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                       "ms_per_channel": round(med / K, 4)}
for name in rates:
    for f in caps:
        for K in KS:
            t = res["cases"]["tune_%s_K%d_%s" % (name, K, f)]
            t["vs_k_resampler_calls"] = round(t["ms_median"] / res["cases"]["rs_x%d_%s_%s" % (K, name, f)]["ms_median"], 3)
            o = res["cases"]["nco_%s_K%d_%s" % (name, K, f)]
            o["vs_rational_tuner"] = round(o["ms_median"] / t["ms_median"], 3)
line = json.dumps(res)
print(line, flush=True)
os.makedirs(a.out, exist_ok=True)
with open(os.path.join(a.out, "tune_time_%s_%s.json" % (a.box, a.tag)), "w") as fh:
    fh.write(line + "\n")
