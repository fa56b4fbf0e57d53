"""The tuner's NCO channels of docs/SPEC.md 3.0d in numpy (a model, not a test): the mixer on tests/spec_model.py's fma with
Python-integer positions, then tests/resample_model.py's resample.

    ph = (step mod 2^32)(n mod 2^32) mod 2^32;  a = ((ph + 2^23) mod 2^32) >> 24;  r = (int32)(ph - (a << 24))
    t = (float)r K;  t2 = t t;  cf = fma(t2, -0.5, 1);  sf = fma(t2 t, -1/6, t)
    c = fma(-S[a], sf, C[a] cf);  s = fma(C[a], sf, S[a] cf)
    v[n].re = fma(x[n].im, s, x[n].re * c);  v[n].im = fma(-x[n].re, s, x[n].im * c)        (step = 0: v = x)

C and S are the rotator table of denominator 256 and are passed in: the library's getter p25fe_tuner_rotator defines them."""
import numpy as np

import resample_model as RM
from spec_model import fma

F = np.float32
K = F(2.0 * np.pi / 2.0 ** 32)
SIXTH = F(-1.0 / 6.0)
MASK = (1 << 32) - 1


def phase(step, abs0, n):
    """the phases of the n samples from the absolute index abs0 (a Python integer of any size) on, uint64 holding 32-bit values"""
    s = int(step) & MASK
    p0 = (s * (int(abs0) & MASK)) & MASK
    return (np.uint64(p0) + np.uint64(s) * np.arange(n, dtype=np.uint64)) & np.uint64(MASK)   # s n < 2^64 for n < 2^32


def factor(step, abs0, n, C, S):
    """(c, s), float32 [n] each"""
    C, S = np.asarray(C, dtype=F), np.asarray(S, dtype=F)
    assert C.shape == S.shape == (256,)
    ph = phase(step, abs0, n).astype(np.int64)
    a = ((ph + (1 << 23)) & MASK) >> 24
    r = ((ph - (a << 24)) & MASK)
    r = np.where(r >= (1 << 31), r - (1 << 32), r)
    assert r.min(initial=0) >= -(1 << 23) and r.max(initial=0) < (1 << 23)
    t = (r.astype(F) * K).astype(F)
    t2 = (t * t).astype(F)
    cf = fma(t2, F(-0.5), F(1.0))
    sf = fma((t2 * t).astype(F), SIXTH, t)
    Ca, Sa = C[a], S[a]
    return fma(-Sa, sf, (Ca * cf).astype(F)), fma(Ca, sf, (Sa * cf).astype(F))


def mix_nco(x, step, abs0, C, S):
    """x (complex64) whose first sample has the absolute index abs0 -> v (complex64)"""
    x = np.ascontiguousarray(x, dtype=np.complex64)
    if int(step) & MASK == 0:
        return x.copy()
    c, s = factor(step, abs0, len(x), C, S)
    re, im = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
    v = np.empty(len(x), dtype=np.complex64)
    v.real = fma(im, s, (re * c).astype(F))
    v.imag = fma(-re, s, (im * c).astype(F))
    return v


def tune_nco(x, L, M, T, taps, step, C, S):
    """one channel of the whole stream x from position 0"""
    return RM.resample(mix_nco(x, step, 0, C, S), L, M, T, taps)


def tune_nco_double(x, L, M, T, taps, step):
    """the formula of 3.0d in double precision with the exact phasor of the integer phase: what the fp32 stage approximates"""
    x = np.asarray(x, dtype=np.complex128)
    ph = phase(step, 0, len(x)).astype(np.float64)
    v = x * np.exp(-2j * np.pi * (ph / 2.0 ** 32))
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
