"""Resource usage of the kernel of the tuner's cuts (k_tune_cuts, docs/SPEC.md 3.0j) for every input format, from a gfx950
cross-compile with -Rpass-analysis=kernel-resource-usage, in tests/test_isa_tune_nco.py's form: no scratch, k_tune_nco's static LDS,
static plus the largest dynamic LDS within 64 KB, k_tune_nco's waves per SIMD, and the registers as committed.  Resource usage and
the existing lint only; needs no GPU."""
import os
import re

from test_isa_resample import VGPR_STEP, WAVES, _remarks
from test_isa_tune_nco import DYNAMIC_MAX, PREFIX as NCO_PREFIX
from test_isa_wide import _usage

# instantiation (mangled template arguments: format, table looked up) -> VGPRs of the kernel as committed: a regression guard, not a
# budget.  The entry's search and the 64-bit offset cost k_tune_nco's count 1, 6, 2 and 2 registers (cf32, s16, u8, u8 looked up)
VGPRS = {"Li0ELb0E": 183, "Li2ELb0E": 162, "Li1ELb0E": 136, "Li1ELb1E": 140}
PREFIX = "_ZN4p25k11k_tune_cutsI"


def test_cut_kernels_use_no_scratch_and_keep_the_nco_kernels_occupancy():
    use = _usage(_remarks())
    cuts = {n: u for n, u in use.items() if n.startswith(PREFIX + "Li")}
    nco = {n[len(NCO_PREFIX):][:8]: u for n, u in use.items() if n.startswith(NCO_PREFIX + "Li")}
    # cf32, s16, u8 with the table as arithmetic, u8 with the table looked up
    assert len(cuts) == 4 and sum("Lb1E" in n for n in cuts) == 1 and len(nco) == 4, sorted(cuts)
    for name, u in sorted(cuts.items()):
        print(name, u)
        key = name[len(PREFIX):][:8]
        assert u["scratch"] == 0, (name, u)
        assert u["lds"] == nco[key]["lds"], (name, u, nco[key])
        assert u["lds"] + DYNAMIC_MAX <= 65536
        assert u["occ"] == nco[key]["occ"] == WAVES[key] and u["vgpr"] <= VGPR_STEP[key], (name, u, nco[key])
        assert u["vgpr"] == VGPRS[key], (name, u)


def test_the_lint_walks_the_cut_kernels():
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
    assert re.search(r"11k_tune_cuts", open(os.path.join(root, "tools", "isa_lint.py")).read())
    bad, warn, nk, nr = lint.lint(asm)
    assert not bad and nr > 0, bad[:5]
    # the walk reaches them: the file's kernels without the four are four fewer
    without = re.sub(r"^%sLi(\w+):" % PREFIX, r"_ZN4p25k9not_cutsILi\1:", src, flags=re.M)
    tmp = asm + ".without_cuts.s"
    with open(tmp, "w") as f:
        f.write(without)
    try:
        assert lint.lint(tmp)[2] == nk - 4
    finally:
        os.remove(tmp)
