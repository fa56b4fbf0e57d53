"""The channeliser of docs/SPEC.md 3.11 in numpy (a model, not a test), its per-output error bound, and the inputs that
tests/test_chz_model.py (CPU) and tests/test_gpu_chz_terms.py (GPU) share.

    y_c[m] = sum_{p<80} h[p] x[n_m - p] e^{-j 2 pi c (n_m - p) / 192}
           = e^{-j 2 pi c n_m / 192} * sum_p x[n_m - p] * (h[p] e^{+j 2 pi c p / 192}),        n_m = 10 m + 9 in absolute indices,

in float64 with twiddles from np.exp (never from the library's table P25FE_CHZ_W), one matrix product per call.  The yardstick of an
output at instant n is the sum of the moduli of ITS terms,

    T(n) = sum over p < 80, sample present, of |h[p]| |x[n - p]|        (float64, on the converted fp32 samples; the same for all c)

and an implementation's output must lie within 2e-6 * T(n) of the model's: 3.11's constant, applied per output.  Where T = 0 that says
the output is an exact zero, of either sign."""
import numpy as np

from test_gpu_wide_fmt import _monotone_table, conv, conv_s16, dev, noise  # noqa: F401  (dev: for the files that use this one)

M, T0, PD, WV = 192, 80, 10, 64                  # channels, taps, decimation, instants per workgroup (one lane each)
K_SPEC = 2e-6                                    # SPEC 3.11's constant (= 33.5 * 2^-24)
U = 2.0 ** -24                                   # unit roundoff of fp32: what the ratios are reported in


def taps():
    """SPEC 3.0's 80 taps as the fp32 numbers every implementation uses, in float64"""
    from oracle import oracle as O
    h = np.array(O.load_spec()["pre_taps"], dtype=np.float32).astype(np.float64)
    assert h.shape == (T0,)
    return h


def o0_of(abs0):
    """owned index of the first instant (absolute index = 9 mod 10) of a range whose first owned sample is at abs0"""
    return (PD - 1 - int(abs0) % PD) % PD


def n_out_of(abs0, n):
    o0 = o0_of(abs0)
    return (n - o0 - 1) // PD + 1 if n > o0 else 0


def instants(n, abs0):
    """absolute instants of the outputs of an owned range of n samples at abs0: int64 [n_out]"""
    return int(abs0) + o0_of(abs0) + PD * np.arange(n_out_of(abs0, n), dtype=np.int64)


def windows(x, n_hist, abs0):
    """x = n_hist samples of history followed by the owned range -> (complex128 [n_out, 80]: column p = x[n_m - p], zero where the
    sample is absent; bool [n_out, 80]: present)"""
    x = np.asarray(x).astype(np.complex128)
    n = len(x) - n_hist
    i = o0_of(abs0) + PD * np.arange(n_out_of(abs0, n), dtype=np.int64)          # owned index of each instant
    j = i[:, None] - np.arange(T0, dtype=np.int64)[None, :] + n_hist            # index into x
    have = j >= 0
    return np.where(have, x[np.where(have, j, 0)], 0.0), have


def model(x, n_hist, abs0, h=None):
    """SPEC 3.11 in float64 -> complex128 [192, n_out]; h: other taps than 3.0's (for the tests of the yardstick itself)"""
    xw, _ = windows(x, n_hist, abs0)
    n = instants(len(x) - n_hist, abs0)
    c = np.arange(M, dtype=np.int64)
    p = np.arange(T0, dtype=np.int64)
    h = taps() if h is None else np.asarray(h, dtype=np.float64)
    g = h[None, :] * np.exp(2j * np.pi * ((c[:, None] * p[None, :]) % M) / M)                # [192, 80]: h[p] e^{+j 2 pi c p / 192}
    rot = np.exp(-2j * np.pi * ((c[:, None] * (n % M)[None, :]) % M) / M)                   # [192, n_out]
    with np.errstate(invalid="ignore", over="ignore"):
        return rot * (g @ xw.T)


def bound(x, n_hist, abs0):
    """T of every output instant -> float64 [n_out]"""
    xw, _ = windows(x, n_hist, abs0)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs(xw) @ np.abs(taps())


def within(got, x, n_hist, abs0, k=K_SPEC, ref=None, cap=None, what=""):
    """Asserts that got (complex [192, n_out]) is non-finite exactly where the reference is and lies within min(k T, cap) of it
    everywhere else; ref = the model unless given (the oracle's output, for the tests that keep it).  Returns the largest
    |got - ref| / (2^-24 T) over the outputs with T > 0."""
    got = np.asarray(got).astype(np.complex128)
    ref = model(x, n_hist, abs0) if ref is None else np.asarray(ref).astype(np.complex128)
    T = bound(x, n_hist, abs0)
    assert got.shape == ref.shape == (M, len(T)), (what, got.shape, ref.shape, len(T))
    if got.shape[1] == 0:
        return 0.0
    xw, have = windows(x, n_hist, abs0)
    n = instants(len(x) - n_hist, abs0)

    def where(c, m):
        ps = np.nonzero(have[m] & (xw[m] != 0))[0]
        return "%s: channel %d, output %d (instant %d, n mod 192 = %d, lane %d), p in %s" % (
            what, c, m, n[m], n[m] % M, m % WV, "[%d, %d]" % (ps[0], ps[-1]) if len(ps) else "[]")
    fin = np.isfinite(ref)
    odd = np.isfinite(got) != fin
    if odd.any():
        c, m = np.argwhere(odd)[0]
        raise AssertionError("%s: got %r where the reference has %r" % (where(c, m), got[c, m], ref[c, m]))
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.where(fin, np.abs(np.where(fin, got - ref, 0.0)), 0.0)
        lim = np.broadcast_to(k * T[None, :], err.shape)
        if cap is not None:
            lim = np.minimum(lim, cap)
        ratio = np.where(fin & (T[None, :] > 0), err / (U * np.where(T > 0, T, 1.0))[None, :], 0.0)
    over = fin & ~(err <= lim)
    if over.any():
        excess = np.where(over, np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), np.inf), 0.0)
        c, m = np.unravel_index(np.argmax(excess), excess.shape)
        raise AssertionError("%s: |got - ref| = %.6g, T = %.6g: %.3f x 2^-24 T (allowed %.3f), %d outputs over; got %r, ref %r" % (
            where(c, m), err[c, m], T[m], ratio[c, m], lim[c, m] / (U * T[m]) if T[m] > 0 else 0.0, int(over.sum()), got[c, m], ref[c, m]))
    return float(ratio.max())


def host(y, no):
    """device [192, W, 2] float32 -> complex64 [192, no]"""
    return y[:, :no].cpu().numpy().view(np.complex64)[..., 0]


# ---- inputs: each returns the raw samples as the call takes them (complex64 [n]; int16 / uint8 [2 n]) and, for u8, the table -------
FORMATS = ("cf32", "s16", "u8")


def cgauss(rng, n, scale=0.3):
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * scale).astype(np.complex64)


def lut_table():
    """a monotone table that is nowhere near a straight line, with table[128] = +0.0: a background of bytes 128 is exact zeros"""
    t = _monotone_table()
    t = (t - t[128]).astype(np.float32)
    assert (np.diff(t) > 0).all() and np.abs(np.diff(t, 2)).max() > 1e-3 and t[128] == 0 and not np.signbit(t[128])
    return t


def converted(raw, table=None):
    return raw if raw.dtype == np.complex64 else conv(raw, table)


IMP_N, IMP_STEP, IMP_FIRST, IMP_COUNT = 2570, 83, 5, 31
IMP_RANGE = dict(offset=96, n_hist=96, abs0=(1 << 32) + 6)            # the same capture as a range, one more impulse in its history


def impulse_positions():
    return IMP_FIRST + IMP_STEP * np.arange(IMP_COUNT)


def impulses(fmt, hist=0):
    """IMP_N owned samples, all zero except sample 83 k + 5, k < 31: (24576 - 16384 j) (-1)^k 2^-(k mod 5) / 32768, exact in s16, real
    and imaginary parts distinct; u8: background 128 (the table's zero), impulses of arbitrary bytes.  hist > 0: that many samples of
    history in front, with one more impulse 40 samples before the owned range.  -> (raw, table or None)"""
    pos = impulse_positions() + hist
    if hist:
        pos = np.concatenate([pos, [hist - 40]])                        # (last: the owned impulses keep their values)
    k = np.arange(len(pos))
    n = hist + IMP_N
    if fmt == "u8":
        b = np.random.default_rng(311).permutation(np.delete(np.arange(256), 128))[:2 * len(pos)].reshape(-1, 2)   # all distinct
        raw = np.full(2 * n, 128, dtype=np.uint8)
        raw[2 * pos], raw[2 * pos + 1] = b[:, 0], b[:, 1]
        return raw, lut_table()
    sgn = 1 - 2 * (k % 2)
    re, im = sgn * (24576 >> (k % 5)), -sgn * (16384 >> (k % 5))
    raw = np.zeros(2 * n, dtype=np.int16)
    raw[2 * pos], raw[2 * pos + 1] = re, im
    return (conv_s16(raw) if fmt == "cf32" else raw), None


GRADED_N, GRADED_STEP = 2570, 107


def graded():
    """complex Gaussian noise scaled by 2^-(i // 107): from 2^0 down to 2^-24"""
    x = cgauss(np.random.default_rng(312), GRADED_N, 1.0).astype(np.complex128)
    return (x * 2.0 ** -(np.arange(GRADED_N) // GRADED_STEP)).astype(np.complex64)


GEO_OFFSET, GEO_SLACK = 2000, 64
GEOMETRY = ([(n_hist, 650, r) for n_hist in (0, 8, 72, 79, 80) for r in range(10)] +
            [(96, n, r) for n in (1, 10, 19, 20, 630, 640, 650, 1290, 1291) for r in (0, 3, 9)])       # (n_hist, n, r): abs0 = offset + r


def geometry_capture(fmt):
    """noise of the format: GEO_OFFSET samples in front of the range, the longest range, and GEO_SLACK behind it"""
    n = GEO_OFFSET + max(g[1] for g in GEOMETRY) + GEO_SLACK
    rng = np.random.default_rng(313)
    return cgauss(rng, n) if fmt == "cf32" else noise(fmt, rng, n)


NF_N, NF_INF, NF_NAN = 1290, 400, 805


def nonfinite():
    x = cgauss(np.random.default_rng(314), NF_N)
    x[NF_INF] = complex(np.inf, x[NF_INF].imag)
    x[NF_NAN] = complex(x[NF_NAN].real, np.nan)
    return x
