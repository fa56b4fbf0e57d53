"""tests/chz_model.py on the CPU: the float64 model of the channeliser (docs/SPEC.md 3.11) against the oracle, and what the shared
inputs of tests/test_gpu_chz_terms.py must have for that file to test what it says -- asked of the inputs alone."""
import numpy as np
import pytest

import chz_model as CM


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


# ---- the model against the oracle ---------------------------------------------------------------------------------------------
# (the oracle indexes absolute positions from 0, so history needs abs0 >= n_hist)
PLACES = [(0, 0), (0, 2003), (40, 2003), (96, 2003), (0, (1 << 32) + 6), (40, (1 << 32) + 6), (96, (1 << 32) + 6)]


@pytest.mark.parametrize("n_hist,abs0", PLACES)
@pytest.mark.parametrize("kind", ["noise", "impulses"])
def test_model_against_oracle(O, kind, n_hist, abs0):
    """The oracle sums the formula as written in double and rounds each component once to fp32: |re|, |im| <= |y| <= T, so it lies
    within 2^-24 T of the model (the two double evaluations differ by ~1e-16 T).  Impulses: one term per output, |y| = T."""
    if kind == "noise":
        x = CM.cgauss(np.random.default_rng(31), n_hist + 1291)
    else:
        x = CM.impulses("cf32", hist=n_hist)[0]
    ref = O.channelise(x, n_hist=n_hist, abs0=abs0)
    assert ref.shape == (CM.M, CM.n_out_of(abs0, len(x) - n_hist))
    worst = CM.within(ref, x, n_hist, abs0, k=CM.U, what="oracle")
    assert 0 < worst <= 1.0


def test_model_nonfinite_where_the_window_holds_one(O):
    """an infinity or a NaN in a window makes all 192 outputs of that instant non-finite and touches no other instant; the oracle's
    outputs are non-finite in the same places"""
    x = CM.nonfinite()
    y = CM.model(x, 0, 0)
    n = CM.instants(len(x), 0)
    hit = np.zeros(len(n), dtype=bool)
    for s in (CM.NF_INF, CM.NF_NAN):
        hit |= (n >= s) & (n - s < CM.T0)
    assert hit.sum() == 16 and np.array_equal(~np.isfinite(y), np.broadcast_to(hit[None, :], y.shape))
    assert np.array_equal(np.isfinite(CM.bound(x, 0, 0)), ~hit)
    assert CM.within(O.channelise(x), x, 0, 0, k=CM.U, what="oracle") <= 1.0


# ---- the yardstick is sharp where the global tolerance is not -------------------------------------------------------------------
@pytest.mark.parametrize("fault", ["h0 x 1.3", "h79 x 0.7", "h1 x 1.05"])
def test_small_tap_faults_pass_globally_and_fail_per_output(fault):
    """a channeliser whose smallest taps are wrong stays within 2e-6 sum|h| max|x| of the truth on noise; on the impulse capture its
    outputs with p = that tap are off by the whole fault, and `within` says so"""
    h = CM.taps()
    bad = h.copy()
    p, f = {"h0 x 1.3": (0, 1.3), "h79 x 0.7": (79, 0.7), "h1 x 1.05": (1, 1.05)}[fault]
    bad[p] *= f
    x = CM.cgauss(np.random.default_rng(21), 30008)
    assert np.abs(CM.model(x, 0, 0, h=bad) - CM.model(x, 0, 0)).max() <= 2e-6 * np.abs(h).sum() * float(np.abs(x).max())
    imp = CM.impulses("cf32")[0]
    with pytest.raises(AssertionError, match=r"p in \[%d, %d\]" % (p, p)):
        CM.within(CM.model(imp, 0, 0, h=bad), imp, 0, 0)


def test_error_must_follow_the_local_signal():
    """3e-6 added to one output of the graded capture where the samples are of size 2^-20: inside the global tolerance, 1e5 T here"""
    x = CM.graded()
    y = CM.model(x, 0, 0)
    assert CM.within(y, x, 0, 0) == 0.0
    m = 20 * CM.GRADED_STEP // CM.PD + 8
    y[17, m] += 3e-6
    assert 3e-6 <= 2e-6 * np.abs(CM.taps()).sum() * float(np.abs(x).max())
    with pytest.raises(AssertionError, match="channel 17, output %d " % m):
        CM.within(y, x, 0, 0)


# ---- conditions on the inputs -------------------------------------------------------------------------------------------------
def test_impulse_capture_reaches_every_term():
    """Every output of the impulse capture has at most one term, and between them the outputs see every tap, every rotation phase
    that exists, every lane, and every tap in both lanes of a store pair.  Instants are always = 9 mod 10, hence odd, so of the 192
    residues n mod 192 only the 96 odd ones exist."""
    pos = CM.impulse_positions()
    assert len(pos) == 31 and pos[0] == 5 and pos[-1] == 83 * 30 + 5 < CM.IMP_N
    n = CM.instants(CM.IMP_N, 0)
    assert len(n) == 257 == 4 * CM.WV + 1 and n[0] == 9                           # four tiles and one instant
    d = n[:, None] - pos[None, :]                                                 # tap index of impulse k in window m, where 0 <= d < 80
    inside = (d >= 0) & (d < CM.T0)
    assert inside.sum(axis=1).max() == 1                                          # no window holds two impulses
    m, k = np.nonzero(inside)
    p, lane = d[m, k], m % CM.WV
    assert set(p) == set(range(CM.T0))
    assert set(n[m] % CM.M) == set(range(1, CM.M, 2))
    assert set(lane) == set(range(CM.WV))
    assert len(set(zip(p, lane % 2))) == 2 * CM.T0
    assert 0 < (~inside.any(axis=1)).sum() < 16                                   # and a few windows hold none: exact zeros
    # what the windows say is what the model's yardstick sees
    x = CM.impulses("cf32")[0]
    xw, _ = CM.windows(x, 0, 0)
    mw, pw = np.nonzero(xw)
    assert np.array_equal(mw, m) and np.array_equal(pw, p) and np.array_equal(xw[mw, pw], x[pos[k]])
    assert np.array_equal(CM.bound(x, 0, 0) == 0, ~inside.any(axis=1))


def test_impulse_values_and_formats():
    """cf32 and s16 carry the same numbers, exact in s16, real and imaginary parts distinct, five sizes and both signs; the u8 form
    is zero exactly off the impulses and its table is no straight line; the range form adds one impulse 40 samples into the history"""
    cf, _ = CM.impulses("cf32")
    s16, _ = CM.impulses("s16")
    assert cf.dtype == np.complex64 and s16.dtype == np.int16 and np.array_equal(CM.conv(s16), cf)
    pos = CM.impulse_positions()
    v = cf[pos]
    k = np.arange(31)
    assert np.array_equal(v, ((24576 - 16384j) * (-1.0) ** k * 2.0 ** -(k % 5) / 32768).astype(np.complex64))
    assert (np.abs(v.real) != np.abs(v.imag)).all() and np.count_nonzero(cf) == 31
    u8, table = CM.impulses("u8")
    cu = CM.conv(u8, table)
    assert table[128] == 0 and np.array_equal(np.nonzero(cu)[0], pos)
    off = np.ones(len(cu), dtype=bool)
    off[pos] = False
    assert np.array_equal(cu[off].view(np.uint32), np.zeros(2 * off.sum(), dtype=np.uint32))          # +0.0
    assert (cu[pos].real != cu[pos].imag).all() and (cu[pos].real != 0).all() and (cu[pos].imag != 0).all()
    for fmt in CM.FORMATS:
        raw, t = CM.impulses(fmt, hist=CM.IMP_RANGE["n_hist"])
        c0, c1 = CM.converted(CM.impulses(fmt)[0], t), CM.converted(raw, t)
        h = CM.IMP_RANGE["n_hist"]
        assert len(c1) == h + CM.IMP_N and np.array_equal(np.nonzero(c1)[0], np.concatenate([[h - 40], pos + h]))
        assert np.array_equal(c1[h:], c0)
    assert CM.n_out_of(CM.IMP_RANGE["abs0"], CM.IMP_N) == 257 and CM.o0_of(CM.IMP_RANGE["abs0"]) == 7


def test_graded_terms_stay_normal():
    """the scale runs from 2^0 to 2^-24 and no product h[p] x, nor any twiddled part of one a few binades below, is subnormal"""
    x = CM.graded()
    assert len(x) == 2570 and (len(x) - 1) // CM.GRADED_STEP == 24
    parts = np.abs(np.concatenate([x.real, x.imag]).astype(np.float64))
    assert parts.min() * np.abs(CM.taps()).min() > 2.0 ** -100
    rms = [np.sqrt(np.mean(np.abs(x[s:s + CM.GRADED_STEP].astype(np.complex128)) ** 2)) * 2.0 ** (s // CM.GRADED_STEP)
           for s in range(0, len(x), CM.GRADED_STEP)]
    assert 1.0 < min(rms) and max(rms) < 2.0
    T = CM.bound(x, 0, 0)
    assert T[-1] < 2.0 ** -20 * T.max() and T[-1] < 1e-6                          # the bound falls with the signal


def test_geometry_counts():
    """the table of tests/test_gpu_chz_terms.py's geometry sweeps: output counts 0, 1, 63, 64, 65, 129 (whole tiles, one instant
    more and less, odd last pairs), all ten o0, histories below, at and above the 79 samples a window reaches back"""
    counts = {CM.n_out_of(CM.GEO_OFFSET + r, n) for _, n, r in CM.GEOMETRY}
    assert {0, 1, 63, 64, 65, 129} <= counts
    assert {CM.o0_of(CM.GEO_OFFSET + r) for _, _, r in CM.GEOMETRY} == set(range(10))
    assert {g[0] for g in CM.GEOMETRY} == {0, 8, 72, 79, 80, 96}
    assert len(CM.GEOMETRY) == 50 + 27 == len(set(CM.GEOMETRY))
    for fmt in CM.FORMATS:
        raw = CM.geometry_capture(fmt)
        assert len(CM.converted(raw)) == CM.GEO_OFFSET + 1291 + CM.GEO_SLACK
    # n_out_of is the oracle's count
    for n in (0, 1, 9, 10, 11, 650):
        for a in range(12):
            assert CM.n_out_of(a, n) == len(range(CM.o0_of(a), n, CM.PD)) and (a + CM.o0_of(a)) % 10 == 9
