"""The AFC loop of docs/SPEC.md 3.0g in Python integers (a model, not a test), on top of tests/afc_model.py.

One channel's update at the absolute input index abs_at, from its record (re, im, pow, n), its (step, ph0), the tuner's L / M, the
measure's D and a configuration: SHORT, REJECT or APPLY in that order.  Every value the 64-bit implementation holds in a signed
register is checked to stay within 63 bits (S below); the wrapping ones are reduced modulo 2^32 where the SPEC says so."""
from fractions import Fraction

import afc_model as AM

MASK = AM.MASK
NONE, SHORT, REJECT, APPLY = 0, 1, 2, 3
CORDIC_N, CORDIC_NORM, CORDIC_FRAC = 32, 60, 48
STATE_FIELDS = ("step", "ph0", "last_theta", "last_dstep", "n_applied", "n_rejected", "n_short", "status")
RECOMMENDED = dict(shift=24, min_products=600, coh_min_q15=24576, gain_q16=65536, max_pull=1 << 24, max_dev=1 << 24)


def S(v):
    """v as a signed 64-bit intermediate: it must fit 63 bits and a sign"""
    assert -(1 << 63) <= v < (1 << 63), v
    return v


def U(v):
    """v as an unsigned 64-bit intermediate of the gate: at most 63 bits"""
    assert 0 <= v < (1 << 63), v
    return v


def _atan_inv(q, bits=120):
    """atan(1 / q), q >= 2, from the alternating series (truncation error below the first omitted term)"""
    s, k, x = Fraction(0), 0, Fraction(1, q)
    while True:
        t = x ** (2 * k + 1) / (2 * k + 1)
        if t < Fraction(1, 1 << bits):
            return s
        s += t if k % 2 == 0 else -t
        k += 1


def atan_table():
    """round(atan(2^-i) / (2 pi) 2^48), i < 32, exactly: Machin's pi = 16 atan(1/5) - 4 atan(1/239)"""
    two_pi = 2 * (16 * _atan_inv(5) - 4 * _atan_inv(239))
    out = [1 << (CORDIC_FRAC - 3)]
    for i in range(1, CORDIC_N):
        out.append(int(_atan_inv(1 << i) / two_pi * (1 << CORDIC_FRAC) + Fraction(1, 2)))
    return out


ATAN = atan_table()


def angle(re, im):
    """the angle of (re, im) in 2^-32 turns as a signed 32-bit integer (a half turn is -2^31); (0, 0) -> 0"""
    re, im = int(re), int(im)
    big = max(abs(re), abs(im))
    if big == 0:
        return 0
    b = big.bit_length()
    if b > CORDIC_NORM:
        x, y = re >> (b - CORDIC_NORM), im >> (b - CORDIC_NORM)      # arithmetic shifts: floor
    else:
        x, y = re << (CORDIC_NORM - b), im << (CORDIC_NORM - b)
    S(x), S(y)
    z = 0
    if x < 0:
        if y >= 0:
            x, y, z = y, -x, 1 << (CORDIC_FRAC - 2)
        else:
            x, y, z = -y, x, -(1 << (CORDIC_FRAC - 2))
    for i in range(CORDIC_N):
        xs, ys = x >> i, y >> i
        if y >= 0:
            x, y, z = S(x + ys), S(y - xs), z + ATAN[i]
        else:
            x, y, z = S(x - ys), S(y + xs), z - ATAN[i]
    fr = CORDIC_FRAC - 32
    t = (S(z + (1 << (fr - 1))) >> fr) & MASK
    return t - (1 << 32) if t >= (1 << 31) else t


def coherent(re, im, pw, c):
    """hypot(re, im) / pw >= c / 32768 on the magnitudes shifted right until the largest has 16 bits; pw > 0"""
    ar, ai, ap = abs(int(re)), abs(int(im)), int(pw)
    b = max(ar, ai, ap).bit_length()
    s = max(b - 16, 0)
    r, i, g = ar >> s, ai >> s, U(int(c) * (ap >> s))
    return U(U(r * r + i * i) << 30) >= U(g * g)


def clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def new_state(step, ph0=0):
    return dict(step=int(step), ph0=int(ph0) & MASK, last_theta=0, last_dstep=0, n_applied=0, n_rejected=0, n_short=0, status=NONE)


def step(cfg, L, M, D, step_ref, acc, state, abs_at):
    """(acc', state'): acc = (re, im, pow, n) as the int64 / uint64 the record holds, state a dict of STATE_FIELDS"""
    re, im, pw, n = (int(v) for v in acc)
    st = dict(state)
    if n < cfg["min_products"]:
        st["n_short"] = (st["n_short"] + 1) & MASK
        st["status"] = SHORT
        return (re, im, pw, n), st
    if pw <= 0 or not coherent(re, im, pw, cfg["coh_min_q15"]):
        st["n_rejected"] = (st["n_rejected"] + 1) & MASK
        st["status"] = REJECT
        return (0, 0, 0, 0), st
    theta = angle(re, im)
    num, den = S(theta * L), S(M * D)
    e = S(2 * abs(num) + den) // (2 * den)
    e = -e if num < 0 else e
    d = clamp(S(e * cfg["gain_q16"] + 32768) >> 16, -cfg["max_pull"], cfg["max_pull"])
    ns = clamp(st["step"] + d, step_ref - cfg["max_dev"], step_ref + cfg["max_dev"])
    ns = clamp(ns, -(1 << 31), (1 << 31) - 1)
    st["step"], st["ph0"] = AM.set_step(st["step"], st["ph0"], ns, int(abs_at) & MASK)    # only abs_at mod 2^32 matters
    st["last_theta"], st["last_dstep"] = theta, d
    st["n_applied"] = (st["n_applied"] + 1) & MASK
    st["status"] = APPLY
    return (0, 0, 0, 0), st


def hz(state, D):
    return state["last_theta"] / 2.0 ** 32 * 240000.0 / D


def pieces(abs_first, n, window):
    """the sequencer's cuts: [(a, b, update?)] of the range [abs_first, abs_first + n) at the absolute multiples of window"""
    out, a, end = [], int(abs_first), int(abs_first) + int(n)
    while a < end:
        b = min(end, (a // window + 1) * window)
        out.append((a, b, b % window == 0))
        a = b
    return out


def tune_piece(x, a, b, L, M, T, taps, step, ph0, C, S):
    """the rows' samples that the input range [a, b) of the stream x owns, with ONE (step, ph0): bit for bit the slice
    [a L // M, b L // M) of afc_model.tune on the whole stream, from a start that is a multiple of M (so that every output keeps its
    polyphase branch) far enough back that every tap of an owned output lies inside the cut"""
    import resample_model as RM
    s0 = max(0, (a - (T - 1)) // M - 1) * M
    y = RM.resample(AM.mix_nco(x[s0:b], step, ph0, s0, C, S), L, M, T, taps)
    o = s0 * L // M
    return y[a * L // M - o:b * L // M - o]


def drifting_capture(seconds=0.75, fs=2500000, up=125, down=12, f0_hz=137500 + 1871.3, drift_hz_s=3000.0, seed=13, snr_db=25.0):
    """one C4FM source (c4fm.synth(seconds, seed, snr_db)) resampled to fs and placed at f0_hz with a linear drift:
    -> (complex64 capture, the generator's symbols)"""
    import numpy as np
    from scipy import signal as sps
    from p25rx_amd import c4fm
    iq, truth, _ = c4fm.synth(seconds, seed=seed, snr_db=snr_db)
    w = sps.resample_poly(iq.astype(np.complex128), up, down)
    t = np.arange(len(w)) / float(fs)
    w = w * np.exp(2j * np.pi * (f0_hz * t + 0.5 * drift_hz_s * t * t))
    return w.astype(np.complex64), truth


def track(x, L, M, T, taps, step0, C, S, D, Tg, g, cfg, window):
    """the sequencer on the whole stream x from position 0 for ONE channel: -> (row, [state after every boundary], [records judged])"""
    import numpy as np
    st = new_state(step0)
    row = np.zeros(0, dtype=np.complex64)
    states, judged, acc, done = [], [], (0, 0, 0, 0), 0
    for a, b, upd in pieces(0, len(x), window):
        row = np.concatenate([row, tune_piece(x, a, b, L, M, T, taps, st["step"], st["ph0"], C, S)])
        # products whose n_m lies in the new samples; the prefilter's history reaches back T - 1 + D samples
        h0 = max(0, (done * D - (Tg - 1 + D)) // D) * D
        prod = AM.products(row[h0:], D, Tg, g, cfg["shift"])
        new = AM.record(prod, done - h0 // D, len(row) // D - done)
        acc = tuple(AM.wrap64(p + q) for p, q in zip(acc[:3], new[:3])) + (acc[3] + new[3],)
        done = len(row) // D
        if upd:
            judged.append(acc)
            acc, st = step(cfg, L, M, D, step0, acc, st, b)
            states.append(dict(st))
    return row, states, judged
