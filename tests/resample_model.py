"""The rational resampler of docs/SPEC.md 3.0b in numpy, built on tests/spec_model.py's fma / _fir (a model, not a test).

    u = m M + (M - 1);  n_m = u div L;  p_m = u mod L;  y[m] = sum_{j < T} h[j L + p_m] x[n_m - j]   (one fp32 fma chain, j ascending)

The outputs m = r (mod L) share the phase p = (r M + M - 1) mod L and sit M input samples apart, starting at
(r M + M - 1) div L: each residue class is one plain decimating FIR, run on re and im separately, and the classes are interleaved
afterwards."""
import numpy as np

from spec_model import _fir

F = np.float32


def n_resample(L, M, abs_first, n):
    """outputs whose n_m lies in [abs_first, abs_first + n), in Python integers"""
    return (abs_first + n) * L // M - abs_first * L // M


def resample(x, L, M, T, taps):
    """the whole stream x (complex64, x[n < 0] = 0) -> complex64"""
    x = np.ascontiguousarray(x, dtype=np.complex64)
    h = np.asarray(taps, dtype=F)
    assert h.shape == (L * T,)
    n_out = n_resample(L, M, 0, len(x))
    y = np.zeros(n_out, dtype=np.complex64)
    xr, xi = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
    for r in range(min(L, n_out)):
        u = r * M + M - 1
        first, p = u // L, u % L
        re = _fir(xr, h[p::L], M, first)
        im = _fir(xi, h[p::L], M, first)
        k = len(y[r::L])
        assert len(re) == k, (r, len(re), k)
        y.real[r::L] = re
        y.imag[r::L] = im
    return y


def phases(L, M, n_out):
    """p_m of the first n_out outputs"""
    m = np.arange(n_out, dtype=np.int64)
    return (m * M + M - 1) % L


def design(fs_in, beta=7.0):
    """the design rule of p25fe_resampler_design restated in float64: (L, M, T, float64 prototype of L T points, sum = L)"""
    from math import gcd
    g = gcd(240000, int(fs_in))
    L, M = 240000 // g, int(fs_in) // g
    T = -(-int(fs_in) // 30000)
    N = L * T
    k = np.arange(N, dtype=np.float64) - (N - 1) / 2.0
    fc = 60000.0 / (L * float(fs_in))
    h = 2.0 * fc * np.sinc(2.0 * fc * k) * np.kaiser(N, beta)
    return L, M, T, h * (L / h.sum())
