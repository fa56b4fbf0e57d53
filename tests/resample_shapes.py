"""The launch plan of the resampler's kernel body as a model, and the shapes at which tests/test_gpu_resample_shapes.py runs it (a
model and a table, not a test).

resample_body (k_resample, k_tune, k_tune_nco, k_tune_cuts) is parametrised by what rs_fill_args makes of a shape (L, M, T), not by
the ratio as such: a sub-tile of `tile` outputs on `gl` lanes with R outputs per lane, fitted to the window of RS_NIN positions.

    fit = 1 + (RS_NIN - T) L div M;  gl = 64 - 64 mod L;  fit >= gl: R = min(fit div gl, 4), tile = gl R;  else R = 1, tile = fit

SHAPES holds the designed rates of docs/SPEC.md 3.0b that the other files do not run and the corners of 3.0b's limits; what the
table has to cover is asserted by tests/test_resample_shapes_model.py, so that it cannot shrink unnoticed."""
from math import gcd

import resample_model as RM

RS_NIN, RS_R, RS_SUBS, WV = 2040, 4, 4, 64                           # the kernel's window, register block, sub-tiles and wave
MAX_L, MAX_M, MAX_T, MAX_TABLE = 32, 1024, 1024, 4096                # docs/SPEC.md 3.0b, "Limits"


def shape_ok(L, M, T):
    return 1 <= L <= MAX_L and L < M <= MAX_M and 1 <= T <= MAX_T and L * T <= MAX_TABLE and gcd(L, M) == 1


def plan(L, M, T):
    """(fit, gl, R, tile): rs_fill_args restated"""
    fit = 1 + (RS_NIN - T) * L // M
    gl = WV - WV % L
    if fit >= gl:
        R = min(fit // gl, RS_R)
        return fit, gl, R, gl * R
    return fit, gl, 1, fit


# designed rates (p25fe_resampler_design: L / M in lowest terms, T = ceil(fs / 30000)): 0.96, 1.024, 1.92, 2, 2.88, 3.2, 4, 5, 6, 8,
# 12, 16 and 30.72 Msps
DESIGNED = ((1, 4, 32), (15, 64, 35), (1, 8, 64), (3, 25, 67), (1, 12, 96), (3, 40, 107), (3, 50, 134), (6, 125, 167), (1, 25, 200),
            (3, 100, 267), (1, 50, 400), (3, 200, 534), (1, 128, 1024))
# corners of the limits
CORNERS = ((1, 2, 1), (1, 2, 2), (1, 2, 3), (7, 8, 5), (5, 6, 6), (1, 2, 7), (1, 2, 8), (1, 2, 15), (1, 1024, 1024), (1, 1024, 1),
           (4, 1023, 1024), (32, 33, 128), (32, 1023, 128), (31, 32, 132), (17, 64, 240), (3, 4, 1024), (13, 1024, 315), (32, 63, 1),
           (9, 1000, 455), (11, 12, 372), (21, 22, 195))
SHAPES = DESIGNED + CORNERS


def shape_id(s):
    return "%d_%d_%d" % tuple(s[:3])


def outputs_for(L, M, T):
    """two full workgroups, one more full sub-tile and a partial one of 3 outputs"""
    return (2 * RS_SUBS + 1) * plan(L, M, T)[3] + 3


def size_for(L, M, T):
    """the smallest n for which the range [0, n) owns outputs_for outputs"""
    want = outputs_for(L, M, T)
    n = -(-want * M // L)                                            # floor(n L / M) >= want  <=>  n >= ceil(want M / L)
    assert RM.n_resample(L, M, 0, n) == want and RM.n_resample(L, M, 0, n - 1) == want - 1
    return n
