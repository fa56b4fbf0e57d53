"""Resource usage of the kernel of the tuner's NCO channels (k_tune_nco, docs/SPEC.md 3.0d and 3.0e) for every input format, from
a gfx950 cross-compile with -Rpass-analysis=kernel-resource-usage, as tests/test_isa_tune.py does for k_tune: no scratch, static
plus the largest dynamic LDS of an accepted tuner within 64 KB, and the registers and occupancy DESIGN.md section 4 (K0c) records
-- the waves per SIMD are k_tune's for every format.  Resource usage only; needs no GPU."""
import os
import re

from test_isa_resample import CSRC, VGPR_STEP, WAVES, WINDOW_BYTES, _remarks
from test_isa_wide import _usage

# instantiation (mangled template arguments: format, table looked up) -> VGPRs of the kernel as committed: a regression guard, not a
# budget (the launch bound is 2 waves per SIMD = 256 registers)
VGPRS = {"Li0ELb0E": 182, "Li2ELb0E": 156, "Li1ELb0E": 134, "Li1ELb1E": 138}
# the largest dynamic LDS p25fe_nco_create can ask for: L * (T | 1) <= 4096 + 32 floats of taps, rounded up to a pair, and the ONE
# rotator table (TN_NCO_DEN pairs of floats)
NCO_DEN = int(re.search(r"constexpr int TN_NCO_DEN = (\d+);", open(os.path.join(CSRC, "p25fe_kernels.hip")).read()).group(1))
DYNAMIC_MAX = 4 * (4096 + 32) + 8 * NCO_DEN
PREFIX = "_ZN4p25k10k_tune_ncoI"


def test_tuner_nco_kernels_use_no_scratch_and_fit_the_lds():
    use = {n: u for n, u in _usage(_remarks()).items() if n.startswith(PREFIX + "Li")}
    # cf32, s16, u8 with the table as arithmetic, u8 with the table looked up
    assert len(use) == 4 and sum("Lb1E" in n for n in use) == 1, sorted(use)
    assert NCO_DEN == 256 and DYNAMIC_MAX == 4 * (4096 + 32) + 2048
    for name, u in sorted(use.items()):
        print(name, u)
        key = name[len(PREFIX):][:8]
        assert u["scratch"] == 0, (name, u)
        assert u["lds"] == WINDOW_BYTES + (1024 if "Lb1E" in name else 0), (name, u)
        assert u["lds"] + DYNAMIC_MAX <= 65536
        assert u["occ"] == WAVES[key] and u["vgpr"] <= VGPR_STEP[key], (name, u)
        assert u["vgpr"] == VGPRS[key], (name, u)


def test_the_lint_walks_the_nco_kernels():
    """tools/isa_lint.py follows the hand-issued LDS reads of rs_fir in the four new kernels too, and finds nothing"""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("isa_lint", os.path.join(root, "tools", "isa_lint.py"))
    lint = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lint)
    _remarks()
    asm = "/tmp/p25fe_api-hip-amdgcn-amd-amdhsa-gfx950.s"
    src = open(asm).read()
    assert len(re.findall(r"^%sLi\w+:" % PREFIX, src, re.M)) == 4
    assert re.search(r"10k_tune_nco", open(os.path.join(root, "tools", "isa_lint.py")).read())
    bad, warn, nk, nr = lint.lint(asm)
    assert not bad and nr > 0, bad[:5]
