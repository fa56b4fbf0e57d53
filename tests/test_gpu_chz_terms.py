"""The channeliser on the GPU (docs/SPEC.md 3.11: k_channelise, k_channelise_fmt) term by term.  Every output is held to ITS OWN bound,

    |got[c, m] - model[c, m]| <= 2e-6 * T(n_m),        T(n) = sum over p < 80, sample present, of |h[p]| |x[n - p]|

(tests/chz_model.py: the formula in float64 with twiddles from np.exp).  The other K6 tests feed noise, whose every output is a sum of
80 terms of similar size, and so cannot see one wrong tap, twiddle, window column or rotation index; here
  * impulses 83 samples apart give every output exactly one term: each tap, each twiddle path and each rotation by itself (cf32, s16,
    and u8 through a table that is no straight line), and once more as a range with history past 2^32;
  * graded amplitudes (2^0 down to 2^-24 within one capture) make the error follow the LOCAL signal;
  * the geometry sweeps compare ranges with short history at an offset, all ten grids, and output counts 0, 1, 63, 64, 65, 129, 130
    with the model -- the count, every output, and the columns behind the padded tile width, which keep their poison;
  * an infinity and a NaN make non-finite exactly the outputs whose window holds them.
tests/test_chz_model.py asks of the inputs, on the CPU, what these cases need of them.

Largest |got - model| / (2^-24 T) observed on an MI355X per group: docs/MEASUREMENTS.md, K6.  The bound allows 33.5."""
import numpy as np
import pytest

import chz_model as CM

pytestmark = pytest.mark.gpu

POISON = 0x7FC0DEAD                                                  # a NaN: left in a column that counts, it fails the comparison


@pytest.fixture(scope="module")
def fes():
    """the default handle and one that converts u8 through chz_model's table (looked up, not specialised)"""
    from p25rx_amd import _lib
    from p25rx_amd.frontend import FrontEnd
    return {None: FrontEnd(), "lut": FrontEnd(u8_lut=CM.lut_table(), specialize=_lib.SPECIALIZE_OFF)}


_DEV = {}


def on_device(key, raw):
    """the capture on the device, once, with 64 samples behind it that no range owns (and that are nowhere near zero)"""
    if key not in _DEV:
        pad = np.full(64 if raw.dtype == np.complex64 else 128, 77, dtype=raw.dtype)
        _DEV[key] = CM.dev(np.concatenate([raw, pad]))
    return _DEV[key]


def run(fe, key, raw, offset, n_hist, n, abs0):
    """the range [offset, offset + n) of the capture -> complex64 [192, n_out].  The output buffer is poisoned and 64 columns wider
    than the rows the kernel pads to whole tiles."""
    import torch
    t = on_device(key, raw)
    no = CM.n_out_of(abs0, n)
    assert fe.L.p25fe_n_predecim(abs0, n) == no
    W = (no + CM.WV - 1) // CM.WV * CM.WV
    out = torch.empty((CM.M, W + 64, 2), dtype=torch.float32, device="cuda")
    out.view(torch.int32).fill_(POISON)
    y, got_no = fe.channelise_dev(t[:offset + n], n_hist=n_hist, abs0=abs0, offset=offset, out=out)
    assert got_no == no and y is out
    assert bool((out.view(torch.int32)[:, W:] == POISON).all()), "written behind the padded tile width"
    return CM.host(out, no)


def report(group, worst):
    print("K6 largest |got - model| / (2^-24 T), %s: %.3f" % (group, worst))


# ---- impulses: one term per output ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", CM.FORMATS)
def test_impulses(fes, fmt):
    """2570 samples, 31 impulses, 257 outputs = four tiles and one instant: all 80 taps, all 96 rotation phases, all 64 lanes, every tap
    in both lanes of a store pair (tests/test_chz_model.py::test_impulse_capture_reaches_every_term).  Outputs whose window holds no
    impulse are exact zeros (T = 0)."""
    raw, table = CM.impulses(fmt)
    x = CM.converted(raw, table)
    got = run(fes["lut" if fmt == "u8" else None], ("imp", fmt), raw, 0, 0, CM.IMP_N, 0)
    assert got.shape == (CM.M, 257)
    empty = CM.bound(x, 0, 0) == 0
    assert 0 < empty.sum() < 16 and not got[:, empty].any()
    worst = CM.within(got, x, 0, 0, what="impulses " + fmt)
    report("impulses " + fmt, worst)


@pytest.mark.parametrize("fmt", CM.FORMATS)
def test_impulses_as_a_range_past_2_32(fes, fmt):
    """the same capture owned from offset 96 with 96 samples of history, abs0 = 2^32 + 6 (o0 = 7, the rotation phase from a 64-bit
    position), and one more impulse 40 samples inside the history: the first outputs have a term that only the history supplies"""
    g = CM.IMP_RANGE
    raw, table = CM.impulses(fmt, hist=g["n_hist"])
    x = CM.converted(raw, table)
    assert g["offset"] == g["n_hist"]
    got = run(fes["lut" if fmt == "u8" else None], ("imp_range", fmt), raw, g["offset"], g["n_hist"], CM.IMP_N, g["abs0"])
    assert got.shape == (CM.M, 257) and got[:, :3].all()                # owned samples 7, 17, 27: p = 47, 57, 67 of the history's impulse
    worst = CM.within(got, x, g["n_hist"], g["abs0"], what="impulses, range, " + fmt)
    report("impulses as a range " + fmt, worst)


# ---- graded amplitudes --------------------------------------------------------------------------------------------------------
def test_graded_amplitudes(fes):
    """noise whose scale falls from 2^0 to 2^-24 over the capture: the bound falls with it (a global tolerance would accept 3e-6 on
    samples of size 1e-7)"""
    x = CM.graded()
    got = run(fes[None], "graded", x, 0, 0, len(x), 0)
    worst = CM.within(got, x, 0, 0, what="graded")
    report("graded amplitudes cf32", worst)


# ---- geometry against the model -------------------------------------------------------------------------------------------------
def _geometry(fes, fmt, cases):
    raw = CM.geometry_capture(fmt)
    cf = CM.converted(raw)
    off = CM.GEO_OFFSET
    worst, counts = 0.0, set()
    for n_hist, n, r in cases:
        got = run(fes[None], ("geo", fmt), raw, off, n_hist, n, off + r)
        counts.add(got.shape[1])
        worst = max(worst, CM.within(got, cf[off - n_hist:off + n], n_hist, off + r, what="%s n_hist %d n %d r %d" % (fmt, n_hist, n, r)))
    return worst, counts


@pytest.mark.parametrize("fmt", CM.FORMATS)
def test_short_history_at_an_offset(fes, fmt):
    """n_hist 0, 8, 72, 79, 80 (the window reaches back 79) on all ten grids, the range 2000 samples into a buffer of noise: what lies
    in front of the history counts as absent, against the model and not only against the same kernel"""
    worst, counts = _geometry(fes, fmt, [g for g in CM.GEOMETRY if g[0] != 96])
    assert counts == {65}
    report("short history " + fmt, worst)


@pytest.mark.parametrize("fmt", CM.FORMATS)
def test_output_counts(fes, fmt):
    """0, 1 and 2 outputs, a tile less one, a tile, a tile and one, two tiles and one or two: an odd count ends in half a store pair"""
    worst, counts = _geometry(fes, fmt, [g for g in CM.GEOMETRY if g[0] == 96])
    assert {0, 1, 2, 63, 64, 65, 129, 130} <= counts
    report("output counts " + fmt, worst)


# ---- non-finite samples ---------------------------------------------------------------------------------------------------------
def test_non_finite_samples_stay_in_their_windows(fes):
    """+Inf in the real part of sample 400, NaN in the imaginary part of sample 805: the 8 + 8 instants whose window holds one are
    non-finite in all 192 channels, as the model's are, and every other output meets its bound"""
    x = CM.nonfinite()
    got = run(fes[None], "nonfinite", x, 0, 0, len(x), 0)
    bad = ~np.isfinite(CM.bound(x, 0, 0))
    assert bad.sum() == 16 and np.array_equal(~np.isfinite(got), np.broadcast_to(bad[None, :], got.shape))
    worst = CM.within(got, x, 0, 0, what="non-finite")
    report("non-finite samples cf32", worst)
