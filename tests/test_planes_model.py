"""CPU tests of the planar-layout model (tests/planes_model.py) and of the diagnostic read-out's surface (p25fe_debug_planes_size /
p25fe_debug_planes_dev in include/p25fe.h): the model round-trips, its masks are exactly the defined cells, its failure messages
name the cell, and the two new symbols are declared everywhere with the ABI version unchanged.  The GPU side is
tests/test_gpu_planes.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import planes_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"p25fe_debug_planes_size", "p25fe_debug_planes_dev"}
SPECIALS = np.array([0x80000000, 0x00000000, 0x00000001, 0x80000001, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0xff800001,
                     0x7fffffff], dtype=np.uint32)       # -0, +0, +-denormal, +-inf, +-quiet NaN, a negative signalling NaN, +NaN


def _signal(rng, n):
    """random floats of every sign with the special patterns spliced in"""
    u = rng.standard_normal(n).astype(np.float32).view(np.uint32).copy()
    if n == 0:
        return u.view(np.float32)
    k = rng.integers(0, n, size=max(1, n // 7))
    u[k] = SPECIALS[rng.integers(0, len(SPECIALS), size=len(k))]
    return u.view(np.float32)


@pytest.mark.parametrize("n", [1, 319, 320, 321, 7681])
@pytest.mark.parametrize("look", [0, PM.LOOK])
def test_model_round_trip(n, look):
    """planes back to linear equals the input bit for bit, the words equal np.signbit (raw sign bits: -0.0 and negative NaNs are
    negative), the masks hold exactly the n + hist defined cells, and every cell outside them is zero -- for no history, one
    sample, and the full HIST_BB + look"""
    rng = np.random.default_rng(1000 * n + look)
    bb = _signal(rng, n)
    for n_hist in (0, 1, PM.HIST_BB + look):
        hist = _signal(rng, n_hist)
        f, w, fmask, wmask = PM.expect(bb, hist, look)
        assert (f.size, w.size) == PM.geometry(n) and f.size % PM.BLK == 0 and w.size * 32 == f.size
        lin, sg = PM.linear(f, w, n, n_hist, look)
        ref = np.concatenate([hist, bb])
        assert np.array_equal(lin, ref.view(np.uint32))
        assert np.array_equal(sg, np.signbit(ref))
        assert int(fmask.sum()) == n + n_hist and sum(bin(int(x)).count("1") for x in wmask) == n + n_hist
        assert not f[~fmask].any() and not (w & ~wmask).any()
        # the words are the sign bits of the floats, block by block; the masks of floats and words name the same cells
        assert np.array_equal(PM.words_of_floats(f), w)
        assert np.array_equal(PM.words_of_floats(np.where(fmask, np.uint32(0x80000000), np.uint32(0))), wmask)
        assert PM.diff_report(f.view(np.float32), w.view(np.int32), (f, w, fmask, wmask), look) is None


def test_model_places_cells_as_the_layout_comment_says():
    """spot values worked out by hand from the comment at PLPAD: sample 0 is bit 0 of word 10 (plane 0 of block 1) with the fixed
    clock and plane 2 with the lookahead; the last history sample is symbol 31 of plane 9 of block 0"""
    assert [int(x) for x in PM.cell(0, 0)] == [320, 10, 0]
    assert [int(x) for x in PM.cell(0, 2)] == [320 + 2 * 32, 12, 0]
    assert [int(x) for x in PM.cell(-1, 0)] == [9 * 32 + 31, 9, 31]
    assert [int(x) for x in PM.cell(-240, 0)] == [8, 0, 8]
    assert [int(x) for x in PM.cell(-242, 2)] == [8, 0, 8]
    assert [int(x) for x in PM.cell(7679, 0)] == [24 * 320 + 9 * 32 + 31, 249, 31]
    assert PM.where(24 * 320 + 9 * 32 + 31, 0) == dict(block=24, plane=9, symbol=799, word=249, bit=31, m=7679)
    assert PM.geometry(0) == PM.geometry(1) == PM.geometry(7680) == (30 * 320, 300) and PM.geometry(7681) == (54 * 320, 540)
    # a stream's start: the zeros of SPEC 3.7 in front, all defined; a handed-over baseband: only what is there
    assert len(PM.history(None, 2)) == 242 and not PM.history(None, 2).any()
    h = PM.history(np.arange(1, 4, dtype=np.float32), 0)
    assert len(h) == 240 and list(h[-4:]) == [0.0, 1.0, 2.0, 3.0]
    assert list(PM.history(np.arange(1, 4, dtype=np.float32), 0, at_stream_start=False)) == [1.0, 2.0, 3.0]
    assert len(PM.history(np.ones(1000, np.float32), 2, at_stream_start=False)) == 242


def test_failure_messages_name_the_cell():
    """one float off in its last bit, one word bit flipped, one word that disagrees with its own float: each is reported with
    block, plane, symbol and both bit patterns; a difference outside the mask is not"""
    rng = np.random.default_rng(5)
    bb, hist = _signal(rng, 700), _signal(rng, 240)
    exp = PM.expect(bb, hist, 0)
    f, w = exp[0].copy(), exp[1].copy()
    k = int(PM.cell(333, 0)[0])
    f[k] ^= 1                                                        # last bit of the mantissa: the sign stays
    msg = PM.diff_report(f.view(np.float32), w.view(np.int32), exp, 0, "case")
    c = PM.where(k, 0)
    assert c["m"] == 333 and "case: 1 floats, 0 words" in msg
    assert "float block %d plane %d symbol %d (m = 333): got %08x, expected %08x" % (c["block"], c["plane"], c["symbol"], f[k], exp[0][k]) in msg
    f = exp[0].copy()
    _, wi, bit = (int(x) for x in PM.cell(-240, 0))
    w[wi] ^= np.uint32(1 << bit)
    msg = PM.diff_report(f.view(np.float32), w.view(np.int32), exp, 0, "case")
    assert "0 floats, 1 words differ from the model, 1 words from their own floats" in msg
    assert "word %d (block 0 plane 0) first wrong bit 8 (symbol 8, m = -240)" % wi in msg and "disagrees with the sign of its own float" in msg
    w = exp[1].copy()
    f[int(PM.cell(700, 0)[0])] = 0x3f800000                          # past the range: not a defined cell
    w[int(PM.cell(-241, 0)[1])] ^= np.uint32(1 << 7)
    assert PM.diff_report(f.view(np.float32), w.view(np.int32), exp, 0) is None


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from p25rx_amd import _lib
    return _lib


def test_abi_surface(lib):
    """header, ctypes, the Rust text and the wrapper name the two diagnostic functions; the header says it is a diagnostic and points
    at PLPAD / planar_index; the ABI version has not moved (an additive call, like the ones before it)"""
    hdr = open(os.path.join(ROOT, "include", "p25fe.h")).read()
    assert re.search(r"#define P25FE_ABI_VERSION 6\b", hdr) and lib.ABI_VERSION == 6
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(p25fe_[a-z0-9_]+)\s*\(", code))
    assert {s for s in declared if "debug" in s} == NEW and NEW <= set(lib.SYMBOLS)
    comment = hdr[:hdr.index("int p25fe_debug_planes_size")]
    comment = comment[comment.rindex("/*"):]
    assert "DIAGNOSTIC" in comment and "PLPAD" in comment and "planar_index" in comment
    rs = open(os.path.join(ROOT, "bindings", "p25fe.rs")).read()
    assert NEW <= set(re.findall(r"pub fn (p25fe_[a-z0-9_]+)\(", rs))
    L = lib.load()
    assert len(L.p25fe_debug_planes_size.argtypes) == 4 and len(L.p25fe_debug_planes_dev.argtypes) == 7
    from p25rx_amd.frontend import FrontEnd
    assert callable(FrontEnd.debug_planes)


def test_refusals_that_need_no_device(lib):
    """a null handle and null out-parameters are argument errors, and nothing is written"""
    L = lib.load()
    nf, nw = C.c_size_t(77), C.c_size_t(78)
    assert L.p25fe_debug_planes_size(None, 100, C.byref(nf), C.byref(nw)) == lib.ERR_ARG and (nf.value, nw.value) == (77, 78)
    buf = np.zeros(16, np.uint32)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.p25fe_debug_planes_dev(None, 100, p, 1 << 20, p, 1 << 20, None) == lib.ERR_ARG and not buf.any()
