"""AFC of docs/SPEC.md 3.0e and 3.0f in numpy (a model, not a test).

3.0e, an NCO channel's phase offset: ph = (ph0 + step n) mod 2^32, everything after ph as in 3.0d (tests/tune_nco_model.py); the
product is skipped only when step = 0 and ph0 = 0.  set_step is Python-integer arithmetic.

3.0f, the frequency measure: w = tests/resample_model.py's resample with L = 1, M = D; the lag-1 product on tests/spec_model.py's
fma; Q; sums in Python integers (wrapped to 64 bits by the caller where a test asks for that).

    p.re = fma(w[m].im, w[m-1].im, w[m].re w[m-1].re);  p.im = fma(-w[m].re, w[m-1].im, w[m].im w[m-1].re)
    e = fma(w[m].im, w[m].im, w[m].re w[m].re);  Q(v) = (int32) rint(clamp(v 2^shift, +-2147483520)), NaN -> 0"""
import math

import numpy as np

import resample_model as RM
import tune_nco_model as NM
from spec_model import fma

F = np.float32
MASK = NM.MASK
QMAX = 2147483520.0


# ---- 3.0e ---------------------------------------------------------------------------------------------------------------------
def factor(step, ph0, abs0, n, C, S):
    """(c, s), float32 [n] each, of the n samples from the absolute index abs0 on.  The phase ph0 + step (abs0 + i) is the phase of
    3.0d at a shifted start: NM.factor takes the start's phase from step * abs0, so the offset goes in as a start of its own."""
    C, S = np.asarray(C, dtype=F), np.asarray(S, dtype=F)
    s = int(step) & MASK
    p0 = (int(ph0) + s * (int(abs0) & MASK)) & MASK
    ph = ((np.uint64(p0) + np.uint64(s) * np.arange(n, dtype=np.uint64)) & np.uint64(MASK)).astype(np.int64)
    a = ((ph + (1 << 23)) & MASK) >> 24
    r = (ph - (a << 24)) & MASK
    r = np.where(r >= (1 << 31), r - (1 << 32), r)
    t = (r.astype(F) * NM.K).astype(F)
    t2 = (t * t).astype(F)
    cf = fma(t2, F(-0.5), F(1.0))
    sf = fma((t2 * t).astype(F), NM.SIXTH, t)
    Ca, Sa = C[a], S[a]
    return fma(-Sa, sf, (Ca * cf).astype(F)), fma(Ca, sf, (Sa * cf).astype(F))


def mix_nco(x, step, ph0, abs0, C, S):
    """x (complex64) whose first sample has the absolute index abs0 -> v (complex64)"""
    x = np.ascontiguousarray(x, dtype=np.complex64)
    if int(step) & MASK == 0 and int(ph0) & MASK == 0:
        return x.copy()
    c, s = factor(step, ph0, abs0, len(x), C, S)
    re, im = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
    v = np.empty(len(x), dtype=np.complex64)
    v.real = fma(im, s, (re * c).astype(F))
    v.imag = fma(-re, s, (im * c).astype(F))
    return v


def set_step(step, ph0, new_step, abs_at):
    """(step, ph0) of a channel retuned to new_step at the absolute index abs_at: the phase at abs_at stays"""
    return int(new_step), (int(ph0) + (int(step) - int(new_step)) * int(abs_at)) & MASK


def tune(x, L, M, T, taps, step, ph0, C, S):
    """one channel of the whole stream x from position 0 with ONE (step, ph0)"""
    return RM.resample(mix_nco(x, step, ph0, 0, C, S), L, M, T, taps)


# ---- 3.0f ---------------------------------------------------------------------------------------------------------------------
def Q(v, shift):
    with np.errstate(over="ignore", invalid="ignore"):
        s = (np.asarray(v, dtype=F) * F(2.0 ** shift)).astype(F)
        s = np.where(np.isnan(s), F(0.0), s)
        s = np.clip(s, F(-QMAX), F(QMAX))
    return np.rint(s).astype(np.int64)


def raw_products(x, D, T, g):
    """the whole stream x (complex64, position 0, x[n < 0] = 0) -> (p.re, p.im, e), float32 [n_out] each; element m belongs to the
    range that holds n_m = m D + D - 1"""
    with np.errstate(over="ignore", invalid="ignore"):
        w = RM.resample(x, 1, D, T, np.asarray(g, dtype=F))
        wr, wi = np.ascontiguousarray(w.real), np.ascontiguousarray(w.imag)
        pr, pi = np.concatenate([[F(0)], wr[:-1]]).astype(F), np.concatenate([[F(0)], wi[:-1]]).astype(F)
        re = fma(wi, pi, (wr * pr).astype(F))
        im = fma(-wr, pi, (wi * pr).astype(F))
        e = fma(wi, wi, (wr * wr).astype(F))
    return re, im, e


def quantise(raw, shift):
    return tuple(Q(v, shift) for v in raw)


def products(x, D, T, g, shift):
    """(Q(p.re), Q(p.im), Q(e)), int64 [n_out] each"""
    return quantise(raw_products(x, D, T, g), shift)


def record(prod, first=0, count=None):
    """(re, im, pow, n) in Python integers: the sums over elements [first, first + count) of products()'s arrays"""
    end = len(prod[0]) if count is None else first + count
    return tuple(int(a[first:end].sum(dtype=object)) if end > first else 0 for a in prod) + (max(end - first, 0),)


def measure(x, D, T, g, shift, first=0, count=None):
    return record(products(x, D, T, g, shift), first, count)


def wrap64(v):
    """a Python integer as the int64 a wrapping accumulator holds"""
    return (int(v) + (1 << 63)) % (1 << 64) - (1 << 63)


def hz(rec, D):
    """(hz, coherence) of a record"""
    re, im, pw = int(rec[0]), int(rec[1]), int(rec[2])
    if pw <= 0:
        return 0.0, 0.0
    return math.atan2(float(im), float(re)) / (2.0 * math.pi) * 240000.0 / D, math.hypot(float(re), float(im)) / float(pw)


def design(D, cutoff_hz, T, beta=7.0):
    """p25fe_afc_design restated in float64: T points, Kaiser(beta), cutoff at 240 ksps, sum 1"""
    k = np.arange(T, dtype=np.float64) - (T - 1) / 2.0
    fc = float(cutoff_hz) / 240000.0
    h = 2.0 * fc * np.sinc(2.0 * fc * k) * np.kaiser(T, beta)
    return h / h.sum()


def hz_double(x, D, g):
    """the estimate in double precision, nothing quantised"""
    x = np.asarray(x, dtype=np.complex128)
    T = len(g)
    xp = np.concatenate([np.zeros(T - 1, dtype=np.complex128), x])
    n_out = len(x) // D
    idx = np.arange(n_out) * D + D - 1 + T - 1
    w = np.zeros(n_out, dtype=np.complex128)
    for j in range(T):
        w += float(g[j]) * xp[idx - j]
    p = (w[1:] * np.conj(w[:-1])).sum()
    return math.atan2(p.imag, p.real) / (2.0 * math.pi) * 240000.0 / D
