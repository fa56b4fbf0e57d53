"""The survey of docs/SPEC.md 3.0h in numpy (a model, not a test): the double-precision DFT of the converted samples, P rounded
to float32, Q, Python-integer sums, and the channel list; and the scene the survey's tests share.

    X_f[b] = sum_j w[j] x[n_f - N + 1 + j] e^{-2 pi i b j / N},   n_f = f hop + hop - 1,   x[n] = 0 for n < 0
    P_f[b] = |X_f[b]|^2 (rounded to float32);   Q(v) = rint(min(v 2^shift, 2^62));   acc[b] += Q(P_f[b]);   acc[N] += 1

The oracle has no entry point for this stage (as for 3.0f): the kernel's DFT is fp32 and factored, so its sums agree with these
within the bound of 3.0h, not bit for bit."""
import numpy as np

F = np.float32
TRUE_OFFSETS_HZ = (-412500 + 1871.3, 137500 - 2210.7, 150000 - 2411.6, 733.1)       # raster channels -33, 11, 12, 0
SCENE_FS, SCENE_UP, SCENE_DOWN = 2500000, 125, 12
SCENE_CHANNELS = {-33: 1871.3, 11: -2210.7, 12: -2411.6, 0: 733.1}                   # raster index -> true offset from it, Hz


def window(N):
    """the designed window: periodic Hann in double, rounded once"""
    j = np.arange(N, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * j / N)).astype(F)


def to_u8(x):
    """complex -> interleaved uint8 pairs [2 n], the offset-binary of an RTL-SDR"""
    v = np.stack([x.real, x.imag], axis=1).astype(np.float64)
    return np.clip(np.rint((v + 1.0) * 127.5), 0, 255).astype(np.uint8).reshape(-1)


def to_s16(x):
    v = np.stack([x.real, x.imag], axis=1).astype(np.float64)
    return np.clip(np.rint(v * 32767.0), -32768, 32767).astype(np.int16).reshape(-1)


def convert_u8(raw, scale=None, offset=None, lut=None):
    """SPEC 3.1: byte b -> fma(b, scale, offset) in float32 (or a table's entry) -> complex64"""
    raw = np.asarray(raw, dtype=np.uint8).reshape(-1, 2)
    if lut is not None:
        v = np.asarray(lut, dtype=F)[raw]
    else:
        v = (raw.astype(np.float64) * np.float64(F(scale)) + np.float64(F(offset))).astype(F)   # the product is exact in double
    return (v[:, 0] + 1j * v[:, 1]).astype(np.complex64)


def convert_s16(raw):
    """SPEC 3.0: an int16 v is v 2^-15, exactly"""
    v = np.asarray(raw, dtype=np.int16).reshape(-1, 2).astype(F) * F(2.0 ** -15)
    return (v[:, 0] + 1j * v[:, 1]).astype(np.complex64)


def n_frames(hop, first, n):
    return (first + n) // hop - first // hop


def spectra(x, N, hop, w, first=0, n=None, n_hist=None):
    """the stream x (converted samples, from position 0) -> X [frames, N] complex128 of the frames the range [first, first + n)
    owns; n_hist: valid samples in front of the range (None: all of them), what is missing reads as zero"""
    x = np.asarray(x, dtype=np.complex128)
    n = len(x) - first if n is None else n
    lo = 0 if n_hist is None else max(0, first - n_hist)
    xp = np.concatenate([np.zeros(N, dtype=np.complex128), x])
    xp[:N + lo] = 0.0
    f = np.arange(first // hop, (first + n) // hop, dtype=np.int64)
    idx = (f * hop + hop - 1 - (N - 1) + N)[:, None] + np.arange(N, dtype=np.int64)[None, :]
    fr = xp[idx] * np.asarray(w, dtype=np.float64)[None, :]
    return np.fft.fft(fr, axis=1)


def quantise(X, shift):
    """X [frames, N] -> Q(P) as float64 holding integers <= 2^62 (exact)"""
    P = (X.real * X.real + X.imag * X.imag).astype(F).astype(np.float64)
    v = np.minimum(np.ldexp(P, shift), 2.0 ** 62)
    v[np.isnan(v)] = 0.0
    return np.rint(v)


def record(x, N, hop, w, shift, first=0, n=None, n_hist=None):
    """the record of one range: uint64 [N + 1] (integer sums, wrapping)"""
    q = quantise(spectra(x, N, hop, w, first, n, n_hist), shift)
    acc = np.zeros(N + 1, dtype=np.uint64)
    acc[:N] = q.astype(np.uint64).sum(axis=0, dtype=np.uint64)     # every value is an integer <= 2^62: the conversion is exact
    acc[N] = q.shape[0]
    return acc


def frame_records(X, shift):
    """X [frames, N] -> one record per frame, uint64 [frames, N + 1]: Q(P_f) and a frame count of 1"""
    q = quantise(X, shift)
    rec = np.ones((q.shape[0], q.shape[1] + 1), dtype=np.uint64)
    rec[:, :-1] = q.astype(np.uint64)
    return rec


def wrapping_sum(rec):
    """records [k, N + 1] -> their sum as uint64 words, modulo 2^64"""
    return np.asarray(rec, dtype=np.uint64).sum(axis=0, dtype=np.uint64)


def delta(N, w, x):
    """3.0h's bound on |X|: 8 log2(N) 2^-24 sum|w| max|x|"""
    return 8.0 * np.log2(N) * 2.0 ** -24 * np.abs(np.asarray(w, dtype=np.float64)).sum() * np.abs(np.asarray(x, dtype=np.complex128)).max()


def frame_bound(X, d, shift):
    """the bound on |acc - Q(P)| of every frame and bin, [frames, N]: |dP| <= 2 |X| d + d^2, times 2^shift, plus one unit for
    the rounding of Q"""
    return (2.0 * np.abs(X) * d + d * d) * 2.0 ** shift + 1.0


def as_ints(a):
    """uint64 words or float64 holding integers -> Python integers (an object array): differences above 2^53 stay exact"""
    return np.array([int(v) for v in np.asarray(a).reshape(-1)], dtype=object).reshape(np.shape(a))


def shifted(x, d):
    """the stream that begins d samples earlier: d zero samples in front of x, so that sample k of x stands at position k + d"""
    return np.concatenate([np.zeros(d, dtype=np.complex128), np.asarray(x, dtype=np.complex128)])


def scan_frames(sc, iq, f0, frames):
    """the GPU's record of every frame by itself: one Scanner.scan_dev call per frame f = f0 .. f0 + frames - 1 into a fresh record,
    n_hist = N - 1, n = hop, the range [f hop, f hop + hop) of a device capture that starts at position 0 (f0 hop >= N - 1)
    -> uint64 [frames, N + 1]"""
    import torch
    assert f0 * sc.hop >= sc.N - 1 and (f0 + frames) * sc.hop <= iq.shape[0]
    rec = torch.zeros((frames, sc.N + 1), dtype=torch.int64, device=iq.device)
    for k in range(frames):
        at = (f0 + k) * sc.hop
        sc.scan_dev(iq, n_hist=sc.N - 1, abs0=at, offset=at, n=sc.hop, acc=rec[k])
    return rec.cpu().numpy().view(np.uint64).copy()


# ---- the saturating scene of the tests of Q's edges: one strong tone on a bin under a caller's window 8 x Hann at shift 40
SAT_N, SAT_HOP, SAT_SHIFT, SAT_BIN, SAT_GAIN = 1024, 256, 40, 100, 8.0
_SAT = {}


def saturating_capture(n=None):
    """0.75 e^{2 pi i 100 t / N} plus noise of sigma 0.01 per component (default_rng(77)), n samples (None: 4 N + 16), made once per
    length -> {format: raw samples}: bin 100's power times 2^40 passes 2^62 in every frame with full history"""
    n = 4 * SAT_N + 16 if n is None else int(n)
    if n not in _SAT:
        t = np.arange(n, dtype=np.float64)
        g = np.random.default_rng(77).standard_normal((n, 2))
        x = (0.75 * np.exp(2j * np.pi * SAT_BIN * t / SAT_N) + 0.01 * (g[:, 0] + 1j * g[:, 1])).astype(np.complex64)
        _SAT[n] = {"cf32": x, "s16": to_s16(x), "u8": to_u8(x)}
    return _SAT[n]


def saturating_window():
    return (window(SAT_N).astype(np.float64) * SAT_GAIN).astype(F)   # (a power of two: exact)


def bin_hz(N, fs):
    b = np.arange(N)
    return np.where(b < N // 2, b, b - N).astype(np.float64) * float(fs) / N


def channels(acc, fs, raster_hz=12500.0, half_bw_hz=4000.0, thr_db=20.0):
    """p25fe_scan_channels: [(r, centre_hz, db_over_floor, offset_hz)], strongest first, ties to the smaller r"""
    acc = np.asarray(acc, dtype=np.uint64)
    N = len(acc) - 1
    if int(acc[N]) == 0:
        return []
    pw, fb = acc[:N].astype(np.float64), bin_hz(N, fs)
    rmax = int(np.floor((fs / 2.0 - raster_hz / 2.0) / raster_hz))
    rows = []
    for r in range(-rmax, rmax + 1):
        fc = r * raster_hz
        if abs(fc) + raster_hz / 2.0 > fs / 2.0:
            continue
        d = np.abs(fb - fc)
        cell = d <= raster_hz / 2.0
        s = pw[cell].sum()
        rows.append((r, pw[d <= half_bw_hz].sum(), (pw[cell] * fb[cell]).sum() / s - fc if s > 0 else 0.0))
    if not rows:
        return []
    pows = sorted(p for _r, p, _o in rows)
    floor = pows[(len(pows) - 1) // 2]
    thr = floor * 10.0 ** (thr_db / 10.0)
    act = sorted((row for row in rows if row[1] > 0 and row[1] >= thr), key=lambda row: (-row[1], row[0]))
    return [(r, r * raster_hz, 10.0 * np.log10(p / floor) if floor > 0 else np.inf, off) for r, p, off in act]


_SCENE = {}


def scene():
    """The survey's scene, made once per process: tests/tune_model.py's site_capture at 2.5 Msps with a C4FM source at each of
    TRUE_OFFSETS_HZ, plus white noise of the sources' own density across the whole band (variance P_src 10^-2.5 fs / 240000 with
    P_src = mean |x|^2 / 4, from default_rng(5)), scaled so that the largest component is 0.9 (it fits u8 and s16).
    -> (complex64 capture, [the generators' symbols per source])"""
    if not _SCENE:
        from tune_model import site_capture
        x, truths = site_capture(SCENE_FS, SCENE_UP, SCENE_DOWN, TRUE_OFFSETS_HZ)
        x = x.astype(np.complex128)
        p_src = np.mean(np.abs(x) ** 2) / 4.0
        var = p_src * 10.0 ** -2.5 * SCENE_FS / 240000.0
        g = np.random.default_rng(5).standard_normal((len(x), 2))
        x = x + np.sqrt(var / 2.0) * (g[:, 0] + 1j * g[:, 1])
        x *= 0.9 / max(np.abs(x.real).max(), np.abs(x.imag).max())
        _SCENE["x"], _SCENE["truths"] = x.astype(np.complex64), truths
    return _SCENE["x"], _SCENE["truths"]
