"""The survey over time of docs/SPEC.md 3.0i in numpy (a model, not a test): the rows -- tests/scan_model.py's spectra and Q, grouped
by slot floor(f / B) as wrapping uint64 sums --, the rule that turns rows into keyed intervals, and the keyed scene the tests share.

    row[f // B - slot0][b] += Q(P_f[b]);   row[f // B - slot0][N] += 1          f absolute: the frame that ends at f hop + hop - 1

Keyed intervals: per row t with frames, pow[t][r] and the floor are p25fe_scan_channels'; channel r turns on where pow > 0 and
pow >= floor 10^(on_db / 10) and stays on while pow >= floor 10^(off_db / 10); a row of zero frames and the end of the rows end
every interval; intervals shorter than min_slots are dropped."""
import numpy as np

import scan_model as SM


def slots(hop, B, first, n):
    """the slots the frames of [first, first + n) fall into -> (first_slot, n_slots); n_slots = 0 when the range owns no frame"""
    f0, f1 = first // hop, (first + n) // hop
    return f0 // B, ((f1 - 1) // B - f0 // B + 1) if f1 > f0 else 0


def group(frames, f0, B):
    """per-frame records [frames, N + 1] of the frames f0, f0 + 1, ... -> (slot0, rows [n_slots, N + 1]): wrapping sums per slot"""
    frames = np.asarray(frames, dtype=np.uint64)
    k = frames.shape[0]
    slot0 = f0 // B
    n_rows = ((f0 + k - 1) // B - slot0 + 1) if k else 0
    rows = np.zeros((n_rows, frames.shape[1]), dtype=np.uint64)
    for i in range(k):
        rows[(f0 + i) // B - slot0] += frames[i]
    return slot0, rows


def batch(N, hop, n_frames):
    """F, the consecutive frames one workgroup of a launch over n_frames frames takes: sc_batch of
    p25rx_amd/csrc/p25fe_scan.inc, min(2^20, max(8, 4 N / H, ceil(n_frames / 1024)))"""
    return min(1 << 20, max(8, 4 * (N // hop), -(-n_frames // 1024)))


def contributors(fa, k, F, B):
    """a launch over the frames fa .. fa + k - 1 in batches of F: per row (row i: slot fa // B + i), the set of workgroup indices
    (f - fa) // F whose frames land in it -> [set] of the length group() gives the rows"""
    slot0 = fa // B
    out = [set() for _ in range(((fa + k - 1) // B - slot0 + 1) if k else 0)]
    for f in range(fa, fa + k):
        out[f // B - slot0].add((f - fa) // F)
    return out


def rows(x, N, hop, w, shift, B, first=0, n=None, n_hist=None):
    """the rows of one range of the stream x (converted samples, from position 0) -> (slot0, uint64 [n_slots, N + 1])"""
    X = SM.spectra(x, N, hop, w, first, n, n_hist)
    return group(SM.frame_records(X, shift), first // hop, B)


def keys(rows_, N, fs, slot0=0, raster_hz=12500.0, half_bw_hz=4000.0, on_db=20.0, off_db=14.0, min_slots=2):
    """p25fe_waterfall_keys: [(raster_index, first_slot, n_slots, centre_hz, offset_hz, peak_db_over_floor)], by first slot, then
    raster index"""
    rows_ = np.asarray(rows_, dtype=np.uint64)
    fb = SM.bin_hz(N, fs)
    rmax = int(np.floor((fs / 2.0 - raster_hz / 2.0) / raster_hz))
    chans = []
    for r in range(-rmax, rmax + 1):
        fc = r * raster_hz
        if abs(fc) + raster_hz / 2.0 > fs / 2.0:
            continue
        d = np.abs(fb - fc)
        order = np.argsort(fb, kind="stable")                        # bins in order of signed frequency
        chans.append((r, fc, order[(d <= half_bw_hz)[order]], order[(d <= raster_hz / 2.0)[order]]))
    if not chans:
        return []
    on, off = 10.0 ** (on_db / 10.0), 10.0 ** (off_db / 10.0)
    live = {}                                                        # channel index -> [first row, s, sf, peak]
    out = []

    def close(c, end):
        first, s, sf, peak = live.pop(c)
        if end - first >= min_slots:
            r, fc = chans[c][0], chans[c][1]
            out.append((r, slot0 + first, end - first, fc, sf / s - fc if s > 0 else 0.0, peak))
    for t in range(rows_.shape[0]):
        if int(rows_[t, N]) == 0:
            for c in sorted(live):
                close(c, t)
            continue
        pw = rows_[t, :N].astype(np.float64)
        pows = [pw[bw].sum() for _r, _fc, bw, _cell in chans]
        floor = sorted(pows)[(len(pows) - 1) // 2]
        for c, (r, fc, bw, cell) in enumerate(chans):
            p = pows[c]
            if c in live and not p >= floor * off:
                close(c, t)
            if c not in live and p > 0 and p >= floor * on:
                live[c] = [t, 0.0, 0.0, -np.inf]
            if c in live:
                st = live[c]
                st[1] += pw[cell].sum()
                st[2] += (pw[cell] * fb[cell]).sum()
                st[3] = max(st[3], 10.0 * np.log10(p / floor) if floor > 0 else np.inf)
    for c in sorted(live):
        close(c, rows_.shape[0])
    return sorted(out, key=lambda k: (k[1], k[0]))


def channel_db(rows_, N, fs, raster_hz=12500.0, half_bw_hz=4000.0):
    """every row's channel powers over that row's floor, dB -> ({raster index: column}, float64 [n_rows, channels])"""
    rows_ = np.asarray(rows_, dtype=np.uint64)
    fb = SM.bin_hz(N, fs)
    rmax = int(np.floor((fs / 2.0 - raster_hz / 2.0) / raster_hz))
    rs = [r for r in range(-rmax, rmax + 1) if abs(r * raster_hz) + raster_hz / 2.0 <= fs / 2.0]
    pw = rows_[:, :N].astype(np.float64)
    pows = np.stack([pw[:, np.abs(fb - r * raster_hz) <= half_bw_hz].sum(axis=1) for r in rs], axis=1)
    floor = np.sort(pows, axis=1)[:, (len(rs) - 1) // 2]
    return {r: i for i, r in enumerate(rs)}, 10.0 * np.log10(pows / floor[:, None])


# ---- the keyed scene: 0.25 s at 2.5 Msps, N 4096, hop 2048, B 6 (305 frames, 51 slots of 12288 samples), shift 16 -----------------
KEY_FS, KEY_N, KEY_HOP, KEY_B, KEY_SHIFT = SM.SCENE_FS, 4096, 2048, 6, 16
KEY_SLOT = KEY_HOP * KEY_B                                           # samples per slot
# (raster index, offset from it in Hz, first keyed sample, first sample after the keying; None: from the start / to the end):
# tests/tune_model.py's C4FM sources (constant-envelope 4-level FM), one per line, hard-gated at slot boundaries plus 5 .. 1300.
# Every keying lasts at least 20 slots (98 ms, 470 symbols): the centroid of ONE slot of such a source wanders by about 300 Hz rms
# with the symbols it happens to carry, and over fewer than 16 slots the mean can still be more than 200 Hz off the carrier
KEY_SOURCES = ((-33, 1871.3, None, None),
               (11, -2210.7, 2 * KEY_SLOT + 5, 23 * KEY_SLOT + 700),
               (12, -2411.6, 8 * KEY_SLOT + 300, 34 * KEY_SLOT + 900),
               (40, 733.1, 14 * KEY_SLOT + 50, 44 * KEY_SLOT + 1200),
               (11, -2210.7, 27 * KEY_SLOT + 1300, 49 * KEY_SLOT + 100))
_KEYED = {}


def keyed_scene():
    """the capture, made once per process: the five sources of KEY_SOURCES (site_capture's source k by itself, gated), white noise
    of the 3.0h scene's density (variance P_src 10^-2.5 fs / 240000, P_src one source's mean power, default_rng(5)), the largest
    component scaled to 0.9 -> complex64 [625000]"""
    if "x" not in _KEYED:
        from tune_model import site_capture
        wide, p_src = None, None
        for k, (r, off, a, b) in enumerate(KEY_SOURCES):
            w, _truth = site_capture(KEY_FS, SM.SCENE_UP, SM.SCENE_DOWN, (r * 12500.0 + off,), seed0=12 + k)
            w = w.astype(np.complex128)
            if p_src is None:
                p_src = np.mean(np.abs(w) ** 2)
            if a is not None:
                w[:a] = 0.0
                w[b:] = 0.0
            wide = w if wide is None else wide + w
        var = p_src * 10.0 ** -2.5 * KEY_FS / 240000.0
        g = np.random.default_rng(5).standard_normal((len(wide), 2))
        x = wide + np.sqrt(var / 2.0) * (g[:, 0] + 1j * g[:, 1])
        x *= 0.9 / max(np.abs(x.real).max(), np.abs(x.imag).max())
        _KEYED["x"] = x.astype(np.complex64)
    return _KEYED["x"]


def keyed_truth():
    """[(raster index, first slot, last slot, true offset in Hz)] by first slot, then raster index: the slots whose own
    KEY_SLOT samples the keying touches"""
    n_slots = len(keyed_scene()) // KEY_HOP // KEY_B + (1 if len(keyed_scene()) // KEY_HOP % KEY_B else 0)
    out = []
    for r, off, a, b in KEY_SOURCES:
        out.append((r, 0 if a is None else a // KEY_SLOT, n_slots - 1 if b is None else (b - 1) // KEY_SLOT, off))
    return sorted(out, key=lambda k: (k[1], k[0]))
