"""The tuner's cuts of docs/SPEC.md 3.0j in Python integers and numpy (a model, not a test): keys -> cuts (p25fe_cuts_from_keys), the
slice a cut is of the whole-range row, the host plan's workgroup counts, the model's row of a cut, and the gated scene of the
end-to-end test.

A cut {abs_first, n, step, ph0} has no arithmetic of its own: its output is the slice [m0, m0 + cnt) of the row an NCO channel
(step, ph0) gives over the call's whole range, m0 = n_resample(L, M, call_first, cut_first - call_first), cnt = n_resample(L, M,
cut_first, cut_n).  The row is tests/afc_model.py's (3.0e: the mixer with a phase offset, then tests/resample_model.py)."""
import math

import numpy as np

import afc_model as AM
import resample_model as RM
from resample_shapes import RS_NIN, RS_R, RS_SUBS, WV, plan          # the kernel's window, register block, sub-tiles and wave

MASK = (1 << 32) - 1
CUTS_MAX = 4096


def nco_step(fs, offset_hz):
    """p25fe_nco_step: nearbyint(offset / fs * 2^32) in double, ties to even, wrapped to 32 bits; None where it refuses"""
    if fs == 0 or not math.isfinite(offset_hz) or 2.0 * abs(offset_hz) > float(fs):
        return None
    q = int(np.rint(math.ldexp(offset_hz / float(fs), 32)))
    return (q + (1 << 31)) % (1 << 32) - (1 << 31)


def from_keys(keys, N, hop, B, fs, margin, range_first, range_n):
    """keys: (raster_index, first_slot, n_slots, centre_hz, offset_hz, ...) tuples -> [(abs_first, n, step, ph0)], cut j for key j.
    Frame f spans [f hop + hop - N, f hop + hop - 1], so a key owns [first_slot B hop + hop - N - margin, (first_slot + n_slots) B
    hop + hop - 1 + margin], clipped to [range_first, range_first + range_n); a key clipped away is n = 0 at the range's nearer end"""
    r0, r1 = range_first, range_first + range_n
    out = []
    for k in keys:
        first_slot, n_slots, centre, off = int(k[1]), int(k[2]), float(k[3]), float(k[4])
        a = first_slot * B * hop + hop - N - margin
        b = (first_slot + n_slots) * B * hop + hop + margin          # one past the last
        a, b = min(max(a, r0), r1), min(max(b, r0), r1)
        out.append((a, max(b - a, 0), nco_step(fs, centre + off), 0))
    return out


def slice_of(L, M, call_first, cut_first, cut_n):
    """(m0, cnt): where the cut's outputs sit in the row of a call that starts at call_first"""
    return RM.n_resample(L, M, call_first, cut_first - call_first), RM.n_resample(L, M, cut_first, cut_n)


def tile(L, M, T):
    """outputs per sub-tile: the host plan's fit of the sub-tile to the window (rs_fill_args)"""
    return plan(L, M, T)[3]


def wg_counts(L, M, T, cuts):
    """workgroups per cut: ceil(cnt / (tile RS_SUBS)); their exclusive prefix is the kernel's first_wg"""
    per = tile(L, M, T) * RS_SUBS
    return [-(-RM.n_resample(L, M, c[0], c[1]) // per) for c in cuts]


def cut_row(x, x_first, L, M, T, taps, cut, C, S):
    """the model's output of one cut: x (complex64) holds the stream from the absolute index x_first on, zero before it.  The model's
    stream starts on the output grid, at the multiple of M at or below x_first, so its output m is the stream's output s0 L / M + m"""
    a, n, step, ph0 = (int(v) for v in cut)
    s0 = x_first // M * M
    z = np.concatenate([np.zeros(x_first - s0, dtype=np.complex64), np.asarray(x, dtype=np.complex64)])
    row = RM.resample(AM.mix_nco(z, step, ph0, s0, C, S), L, M, T, taps)
    first, cnt = RM.n_resample(L, M, s0, a - s0), RM.n_resample(L, M, a, n)
    assert a >= x_first and first + cnt <= len(row)
    return row[first:first + cnt]


# ---- the gated scene of the end-to-end test: 0.25 s at 2.5 Msps, the survey's N 4096, hop 2048, B 6 (51 slots of 12288 samples) -----
# tests/waterfall_model.py's keyed scene with sources that carry a frame sync every 216 dibits (45 ms) instead of every 864, so that
# every keying of 20 slots (98 ms) holds at least one: (raster index, offset from it in Hz, first keyed sample, first sample after
# the keying; None: from the start / to the end), source k is c4fm.synth(0.25, seed = SCENE_SEED0 + k, snr_db = 25, frame_dibits = 216).
# Rasters 11 and 12 are neighbours; raster 11 is keyed twice.
SCENE_FS, SCENE_N, SCENE_HOP, SCENE_B, SCENE_SHIFT = 2500000, 4096, 2048, 6, 16
SCENE_UP, SCENE_DOWN = 125, 12
SCENE_SLOT = SCENE_HOP * SCENE_B
SCENE_SEED0 = 12
SCENE_SOURCES = ((-33, 1871.3, None, None),
                 (11, -2210.7, 2 * SCENE_SLOT + 5, 25 * SCENE_SLOT + 700),
                 (12, -2411.6, 8 * SCENE_SLOT + 300, 34 * SCENE_SLOT + 900),
                 (40, 733.1, 14 * SCENE_SLOT + 50, 44 * SCENE_SLOT + 1200),
                 (11, -2210.7, 27 * SCENE_SLOT + 1300, 49 * SCENE_SLOT + 100))
_SCENE = {}


def gated_scene():
    """(capture complex64 [625000], [the generators' symbols per source]), made once per process: every source resampled and
    shifted as tests/tune_model.py's site_capture does, hard-gated as tests/waterfall_model.py's KEY_SOURCES are, white noise of
    keyed_scene's density (variance P_src 10^-2.5 fs / 240000, default_rng(5)), the largest component scaled to 0.9"""
    if "x" not in _SCENE:
        from scipy import signal as sps
        from p25rx_amd import c4fm
        wide, p_src, truths = None, None, []
        for k, (r, off, a, b) in enumerate(SCENE_SOURCES):
            iq, truth, _ = c4fm.synth(0.25, seed=SCENE_SEED0 + k, snr_db=25.0, frame_dibits=216)
            w = sps.resample_poly(iq.astype(np.complex128), SCENE_UP, SCENE_DOWN)
            w = w * np.exp(2j * np.pi * ((r * 12500.0 + off) / float(SCENE_FS)) * np.arange(len(w)))
            if p_src is None:
                p_src = np.mean(np.abs(w) ** 2)
            if a is not None:
                w[:a] = 0.0
                w[b:] = 0.0
            wide = w if wide is None else wide + w
            truths.append(truth)
        var = p_src * 10.0 ** -2.5 * SCENE_FS / 240000.0
        g = np.random.default_rng(5).standard_normal((len(wide), 2))
        x = wide + np.sqrt(var / 2.0) * (g[:, 0] + 1j * g[:, 1])
        x *= 0.9 / max(np.abs(x.real).max(), np.abs(x.imag).max())
        x = x.astype(np.complex64)
        x.setflags(write=False)
        _SCENE["x"], _SCENE["truths"] = x, truths
    return _SCENE["x"], _SCENE["truths"]


def gated_truth():
    """[(raster index, first slot, last slot, true offset in Hz, source index)] by first slot, then raster index: the slots whose
    own SCENE_SLOT samples the keying touches (tests/waterfall_model.py's keyed_truth)"""
    n = len(gated_scene()[0])
    n_slots = n // SCENE_HOP // SCENE_B + (1 if n // SCENE_HOP % SCENE_B else 0)
    out = []
    for k, (r, off, a, b) in enumerate(SCENE_SOURCES):
        out.append((r, 0 if a is None else a // SCENE_SLOT, n_slots - 1 if b is None else (b - 1) // SCENE_SLOT, off, k))
    return sorted(out, key=lambda t: (t[1], t[0]))
