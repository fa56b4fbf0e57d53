"""Resource usage of the survey-over-time kernel (docs/SPEC.md 3.0i: k_waterfall<FMT, LUTM, N>) from a gfx950 cross-compile with
-Rpass-analysis=kernel-resource-usage, by tests/test_isa_scan.py's method: for both N and every input format no scratch, static LDS
within 80 KB and exactly k_scan's (the body is shared), at least one workgroup per CU -- in fact two everywhere, as for k_scan --
and the registers as committed.  Resource usage only; needs no GPU."""
import os
import subprocess

from test_isa_resample import CSRC, REMARKS, _remarks
from test_isa_scan import LDS
from test_isa_wide import _usage

WATERFALL = "_ZN4p25k11k_waterfallILi"
# instantiation (mangled template arguments: format, table looked up, N) -> VGPRs of the kernel as committed: a regression guard,
# not a budget (the launch bound is 2 waves per SIMD = 256 registers; k_scan's registers plus at most two: the row pointer is
# uniform, the per-slot delivery re-uses the sums' registers)
VGPRS = {"Li0ELb0ELi4096E": 256, "Li2ELb0ELi4096E": 230, "Li1ELb0ELi4096E": 214, "Li1ELb1ELi4096E": 216,
         "Li0ELb0ELi1024E": 98, "Li2ELb0ELi1024E": 100, "Li1ELb0ELi1024E": 100, "Li1ELb1ELi1024E": 98}


def _waterfall_remarks():
    """this tree's remarks: test_isa_resample's, compiled afresh when the survey's sources are newer than they are"""
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in ("p25fe_scan.inc", "p25fe_waterfall.inc"))
    if os.path.exists(REMARKS) and os.path.getmtime(REMARKS) < newest:
        subprocess.check_call(["make", "-s", "-C", CSRC, "asm"], env=dict(os.environ, HIPCC=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))
    return _remarks()


def test_waterfall_kernels_use_no_scratch_and_fit_a_cu():
    use = {n[len(WATERFALL) - 2:][:15]: u for n, u in _usage(_waterfall_remarks()).items() if n.startswith(WATERFALL)}
    # cf32, s16, u8 with the table as arithmetic, u8 with the table looked up, for N = 1024 and 4096
    assert sorted(use) == sorted(VGPRS), sorted(use)
    for key, u in sorted(use.items()):
        print(key, u)
        N = 4096 if "Li4096E" in key else 1024
        assert u["scratch"] == 0, (key, u)
        assert u["lds"] == LDS[N] + (1024 if "Lb1E" in key else 0) and u["lds"] <= 80 * 1024, (key, u)
        assert u["occ"] >= 2, (key, u)                               # one is needed; two is what the launch bound asks for
        assert u["vgpr"] == VGPRS[key], (key, u)
