"""k_frontend_pair from a gfx950 cross-compile (needs no GPU): its budget -- at most 128 VGPRs (four waves per SIMD), no scratch,
at most 20 480 B of LDS per workgroup (eight workgroups = 16 waves per CU), no violation of the hand-issued LDS reads' invariant --
and the text of every k_frontend / k_chunk kernel beside it, which must be what it was before the pair kernel existed, and the pair
kernel's own, which must be what it was before stages of the sub-tile became functions shared with frontend_body:
tests/golden/k1_isa_text.json holds, per mangled name, the line count and SHA-256 of the normalised text (tools/isa_text.py) of the
commit in front of that change.  (A compiler update changes those hashes: regenerate the file from the parent commit's build then.)
The text is pinned because equal instruction counts are not enough: a commuted v_add_f32 picks the other operand's NaN payload."""
import json
import os
import re
import subprocess
import sys

from test_isa_resample import _remarks
from test_isa_wide import _usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
ASM = "/tmp/p25fe_api-hip-amdgcn-amd-amdhsa-gfx950.s"
PAIR = "_ZN4p25k15k_frontend_pairE"


def test_pair_kernel_budget():
    use = {n: u for n, u in _usage(_remarks()).items() if n.startswith(PAIR)}
    assert len(use) == 1, sorted(use)
    (name, u), = use.items()
    print(name, u)
    assert u["vgpr"] <= 128 and u["occ"] >= 4 and u["scratch"] == 0, u
    assert u["lds"] == 0                                             # (all of it is dynamic: the host's figure is PairGeo::LDS)
    src = open(os.path.join(ROOT, "p25rx_amd", "csrc", "p25fe_kernels.hip")).read()
    geo = src[src.index("struct PairGeo {"):]
    geo = geo[:geo.index("};")]
    assert "LDS <= 20480" in geo and "XIN_B + 2 * DBUF_B + sizeof(float) * G::SUB" in geo
    # the same sum with the build's numbers (Geo<5>: XIN_N 1632, D_N 360, SUB 320)
    assert 8 * 1632 + 2 * 8 * 360 + 4 * 320 == 20096


def test_pair_kernel_lint_and_barriers():
    import isa_lint
    _remarks()
    bad, warn, nk, nr = isa_lint.lint(ASM)
    assert not bad and nk >= 42, (bad[:5], nk)
    src = open(ASM).read()
    m = re.search(r"^%s\w+:" % PAIR, src, re.M)
    body = src[m.end():src.index(".Lfunc_end", m.end())]
    assert "scratch_" not in body
    # one barrier each for P and B(t) on the consumer; P, B(0) of the peeled first sub-tile and B(t) on the producer at most
    n_bar = len(re.findall(r"^\s*s_barrier\b", body, re.M))
    assert 4 <= n_bar <= 6, n_bar
    # every barrier is the helper's: the wave's LDS operations have landed, nothing else is waited for
    assert len(re.findall(r"s_waitcnt lgkmcnt\(0\)\n\s*s_barrier\b", body)) == n_bar


def test_one_wave_kernels_text_is_unchanged():
    import isa_text
    _remarks()
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "k1_isa_text.json")))
    got = isa_text.functions(ASM, isa_text.K1_PREFIXES + (PAIR,))
    assert sorted(got) == sorted(want), (sorted(set(got) ^ set(want)))
    diff = [n for n in want if got[n] != want[n]]
    assert not diff, diff
