"""The tuner of docs/SPEC.md 3.0c in numpy (a model, not a test): the mixer on tests/spec_model.py's fma, then
tests/resample_model.py's resample.

    i = ((num mod D) (n mod D)) mod D;  c = C[i];  s = S[i]
    v[n].re = fma(x[n].im, s, x[n].re * c);  v[n].im = fma(-x[n].re, s, x[n].im * c)        (num = 0: v = x)

C and S are the rotator table of the denominator D and are passed in: the library's getter p25fe_tuner_rotator defines them."""
import numpy as np

import resample_model as RM
from spec_model import fma

F = np.float32


def mix(x, num, den, C, S, abs0=0):
    """x (complex64) whose first sample has the absolute index abs0 -> v (complex64)"""
    x = np.ascontiguousarray(x, dtype=np.complex64)
    if num == 0:
        return x.copy()
    C, S = np.asarray(C, dtype=F), np.asarray(S, dtype=F)
    assert C.shape == S.shape == (den,)
    n = (int(abs0) % den + np.arange(len(x), dtype=np.int64)) % den
    i = ((num % den) * n) % den
    c, s = C[i], S[i]
    re, im = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
    v = np.empty(len(x), dtype=np.complex64)
    v.real = fma(im, s, (re * c).astype(F))
    v.imag = fma(-re, s, (im * c).astype(F))
    return v


def tune(x, L, M, T, taps, num, den, C, S):
    """one channel of the whole stream x from position 0"""
    return RM.resample(mix(x, num, den, C, S), L, M, T, taps)


def tune_double(x, L, M, T, taps, num, den):
    """the formula of 3.0c in double precision, the exact rotator: what the fp32 stage approximates"""
    x = np.asarray(x, dtype=np.complex128)
    n = np.arange(len(x), dtype=np.int64) % den
    v = x * np.exp(-2j * np.pi * (((num % den) * n) % den) / den)
    h = np.asarray(taps, dtype=np.float64)
    n_out = RM.n_resample(L, M, 0, len(x))
    m = np.arange(n_out, dtype=np.int64)
    u = m * M + M - 1
    nm, pm = u // L, u % L
    vp = np.concatenate([np.zeros(T - 1, dtype=np.complex128), v])
    y = np.zeros(n_out, dtype=np.complex128)
    for j in range(T):
        y += h[j * L + pm] * vp[nm - j + T - 1]
    return y


def site_capture(fs, up, down, offsets_hz, seed0=12):
    """One capture at fs (= 240000 up / down) holding a C4FM source per offset (c4fm.synth(0.25, seed=seed0 + k, snr_db=25.0),
    resampled and shifted to its offset, all summed) -> (complex64 capture, [the generators' symbols per source])"""
    from scipy import signal as sps
    from p25rx_amd import c4fm
    wide, truths = None, []
    for k, off in enumerate(offsets_hz):
        iq, truth, _ = c4fm.synth(0.25, seed=seed0 + k, snr_db=25.0)
        w = sps.resample_poly(iq.astype(np.complex128), up, down)
        w = w * np.exp(2j * np.pi * (float(off) / float(fs)) * np.arange(len(w)))
        wide = w if wide is None else wide + w
        truths.append(truth)
    return wide.astype(np.complex64), truths
