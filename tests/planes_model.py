"""A plain numpy model of the blocked polyphase ("planar") baseband and its sign words, written from the layout's description at
PLPAD in p25rx_amd/csrc/p25fe_kernels.hip -- not from any kernel's store code:

  sample m of a call's range sits at planar position p = m + PLPAD + look   (look: 0 with the fixed clock, the clock's lookahead
                                                                             with the tracking ones)
  position p is plane r = p % 10 of symbol i = p // 10
  its float is element  (i // 32) * 320 + r * 32 + i % 32                   (a block = 32 symbols of all ten planes)
  its sign is bit i % 32 of word (i // 32) * 10 + r                         (the RAW sign bit: -0.0 and negative NaNs are negative)

A call defines the cells m in [-hist, n): hist = min(available history, HIST_BB + look).  In front of a stream the history is zeros
(docs/SPEC.md 3.7: b[n] = 0 for n < 0), so a call at the start of a stream defines all HIST_BB + look cells, as +0.0 / bit 0.
tests/test_gpu_planes.py pushes the oracle's linear baseband through `expect` and compares the GPU's scratch with it cell by cell.
"""
import json
import os

import numpy as np

_SPEC = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spec.json")))
SPS = int(_SPEC["sps"])                          # 10 planes
SYM_BLK = 32                                     # symbols per block
BLK = SYM_BLK * SPS                              # floats per block
PLPAD = 320                                      # positions in front of sample 0 (look = 0)
HIST_BB = 240                                    # the receiver's history: a 24-symbol sync window
LOOK = int(_SPEC["clk_lookahead"])               # P25FE_CLK_LOOKAHEAD
TILE = 7680                                      # baseband samples per receiver tile (24 blocks)
assert SPS == 10 and PLPAD % BLK == 0 and PLPAD >= HIST_BB + LOOK


def look_of(symbol_clock):
    return 0 if (symbol_clock & 0xff) == 0 else LOOK


def geometry(n_bb):
    """(floats, words) per channel of the scratch of a call with n_bb baseband samples: whole tiles (at least one), six blocks
    on top (one in front for the pad, the rest behind for what the kernels round up to)"""
    n_tiles = max(1, -(-int(n_bb) // TILE))
    n_blocks = (TILE // BLK) * n_tiles + 6
    return n_blocks * BLK, n_blocks * SPS


def cell(m, look):
    """sample index (array or scalar, may be negative) -> (float index, word index, bit)"""
    p = np.asarray(m, dtype=np.int64) + PLPAD + look
    assert np.all(p >= 0)
    r, i = p % SPS, p // SPS
    return (i // SYM_BLK) * BLK + r * SYM_BLK + i % SYM_BLK, (i // SYM_BLK) * SPS + r, i % SYM_BLK


def where(fidx, look):
    """float index -> dict(block, plane, symbol, word, bit, m): the names a failure message gives a cell"""
    fidx = int(fidx)
    blk, rest = divmod(fidx, BLK)
    r, s = divmod(rest, SYM_BLK)
    i = blk * SYM_BLK + s
    return dict(block=blk, plane=r, symbol=i, word=blk * SPS + r, bit=s, m=i * SPS + r - PLPAD - look)


def history(prev_bb, look, at_stream_start=True):
    """The history a call sees, oldest first: the last HIST_BB + look samples of `prev_bb` (what the stream held before the call's
    range), with the zeros of SPEC 3.7 in front if the stream starts inside them -- or, with at_stream_start False (a baseband
    handed over with n_hist_bb valid samples and nothing known about what was before), only the samples there are."""
    want = HIST_BB + look
    prev = np.zeros(0, np.float32) if prev_bb is None else np.ascontiguousarray(prev_bb, dtype=np.float32)[-want:]
    if at_stream_start and len(prev) < want:
        prev = np.concatenate([np.zeros(want - len(prev), np.float32), prev])
    return prev


def expect(bb, hist, look, n_floats=None, n_words=None):
    """bb: the call's n linear baseband samples (float32); hist: the defined history in front of it, oldest first (see `history`).
    -> (floats uint32 [n_floats]: the expected bit patterns, words uint32 [n_words], fmask bool [n_floats], wmask uint32 [n_words]:
    the defined cells).  Undefined cells are 0 in the first two."""
    bb = np.ascontiguousarray(bb, dtype=np.float32)
    hist = np.ascontiguousarray(hist, dtype=np.float32)
    assert len(hist) <= HIST_BB + look
    n = len(bb)
    gf, gw = geometry(n)
    n_floats = gf if n_floats is None else n_floats
    n_words = gw if n_words is None else n_words
    lin = np.concatenate([hist, bb]).view(np.uint32)
    m = np.arange(-len(hist), n, dtype=np.int64)
    fi, wi, bit = cell(m, look)
    f = np.zeros(n_floats, np.uint32)
    fmask = np.zeros(n_floats, bool)
    f[fi] = lin
    fmask[fi] = True
    w = np.zeros(n_words, np.uint32)
    wmask = np.zeros(n_words, np.uint32)
    one = np.uint32(1) << bit.astype(np.uint32)
    np.bitwise_or.at(w, wi, np.where(lin >> 31 != 0, one, np.uint32(0)))
    np.bitwise_or.at(wmask, wi, one)
    return f, w, fmask, wmask


def linear(f, words, n, n_hist, look):
    """the inverse: planes -> (the n_hist + n linear samples as uint32 bit patterns, their sign bits from the words)"""
    fi, wi, bit = cell(np.arange(-n_hist, n, dtype=np.int64), look)
    f = np.ascontiguousarray(f).view(np.uint32)
    words = np.ascontiguousarray(words).view(np.uint32)
    return f[fi], ((words[wi] >> bit.astype(np.uint32)) & 1).astype(bool)


def words_of_floats(f):
    """the sign words a block-complete float array implies: word (blk, r) bit s = sign bit of float blk * 320 + r * 32 + s"""
    u = np.ascontiguousarray(f).view(np.uint32)
    assert u.size % BLK == 0
    b = (u >> 31).reshape(-1, SYM_BLK).astype(np.uint64)
    return (b << np.arange(SYM_BLK, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def diff_report(got_f, got_w, exp, look, what="", limit=6):
    """None if the GPU's planes (float32 / int32 arrays of one channel) equal the model's under the masks, and the words under the
    mask are the sign bits of the GPU's own floats; else a message naming the first few cells."""
    ef, ew, fmask, wmask = exp
    gf = np.ascontiguousarray(got_f).view(np.uint32)
    gw = np.ascontiguousarray(got_w).view(np.uint32)
    assert gf.shape == ef.shape and gw.shape == ew.shape, (gf.shape, ef.shape, gw.shape, ew.shape)
    lines = []
    bad = np.flatnonzero((gf != ef) & fmask)
    for k in bad[:limit]:
        c = where(k, look)
        lines.append("float block %(block)d plane %(plane)d symbol %(symbol)d (m = %(m)d)" % c + ": got %08x, expected %08x" % (gf[k], ef[k]))
    wbad = np.flatnonzero(((gw ^ ew) & wmask) != 0)
    for k in wbad[:limit]:
        x = int((gw[k] ^ ew[k]) & wmask[k])
        s = (x & -x).bit_length() - 1
        blk, r = divmod(int(k), SPS)
        lines.append("word %d (block %d plane %d) first wrong bit %d (symbol %d, m = %d): got %08x, expected %08x under mask %08x"
                     % (k, blk, r, s, blk * SYM_BLK + s, (blk * SYM_BLK + s) * SPS + r - PLPAD - look, gw[k], ew[k], wmask[k]))
    # independent of the oracle: the words against the sign bits of the floats that came back
    own = words_of_floats(gf)
    cbad = np.flatnonzero(((gw ^ own) & wmask) != 0)
    for k in cbad[:limit]:
        x = int((gw[k] ^ own[k]) & wmask[k])
        s = (x & -x).bit_length() - 1
        blk, r = divmod(int(k), SPS)
        lines.append("word %d (block %d plane %d) bit %d (symbol %d) disagrees with the sign of its own float: word %08x, floats' signs %08x"
                     % (k, blk, r, s, blk * SYM_BLK + s, gw[k], own[k]))
    if not lines:
        return None
    return "%s: %d floats, %d words differ from the model, %d words from their own floats\n  " % (what, len(bad), len(wbad), len(cbad)) + "\n  ".join(lines)
