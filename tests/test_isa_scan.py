"""Resource usage of the survey kernel (docs/SPEC.md 3.0h: k_scan<FMT, LUTM, N>) from a gfx950 cross-compile with
-Rpass-analysis=kernel-resource-usage, as tests/test_isa_afc.py does for k_afc_measure: for both N and every input format no
scratch, static LDS within 80 KB and two waves per SIMD (a workgroup is four waves, one per SIMD: two workgroups per CU), and the
registers as committed.  Resource usage only; needs no GPU."""
import os
import subprocess

from test_isa_resample import CSRC, REMARKS, _remarks
from test_isa_wide import _usage

SCAN = "_ZN4p25k6k_scanILi"
# instantiation (mangled template arguments: format, table looked up, N) -> VGPRs of the kernel as committed: a regression guard,
# not a budget (the launch bound is 2 waves per SIMD = 256 registers; radix 16 holds 16 complex values, 16 64-bit sums and the next
# hop's vectors -- 9 for cf32, 5 for s16, 3 for u8 -- and cf32 sits at the bound)
VGPRS = {"Li0ELb0ELi4096E": 256, "Li2ELb0ELi4096E": 228, "Li1ELb0ELi4096E": 214, "Li1ELb1ELi4096E": 214,
         "Li0ELb0ELi1024E": 98, "Li2ELb0ELi1024E": 98, "Li1ELb0ELi1024E": 98, "Li1ELb1ELi1024E": 98}
# static LDS: the ring and the transpose buffer of N + N / 16 complex entries each, radix 16's 240 twiddles of pass 1, and the
# 256-entry table where it is looked up
LDS = {4096: 2 * (4096 + 256) * 8 + 240 * 8, 1024: 2 * (1024 + 64) * 8}


def _scan_remarks():
    """this tree's remarks: test_isa_resample's, compiled afresh when the survey's source is newer than they are"""
    inc = os.path.join(CSRC, "p25fe_scan.inc")
    if os.path.exists(REMARKS) and os.path.getmtime(REMARKS) < os.path.getmtime(inc):
        subprocess.check_call(["make", "-s", "-C", CSRC, "asm"], env=dict(os.environ, HIPCC=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))
    return _remarks()


def test_scan_kernels_use_no_scratch_and_run_two_workgroups_per_cu():
    use = {n[len(SCAN) - 2:][:15]: u for n, u in _usage(_scan_remarks()).items() if n.startswith(SCAN)}
    # cf32, s16, u8 with the table as arithmetic, u8 with the table looked up, for N = 1024 and 4096
    assert sorted(use) == sorted(VGPRS), sorted(use)
    for key, u in sorted(use.items()):
        print(key, u)
        N = 4096 if "Li4096E" in key else 1024
        assert u["scratch"] == 0, (key, u)
        assert u["lds"] == LDS[N] + (1024 if "Lb1E" in key else 0) and u["lds"] <= 80 * 1024, (key, u)
        assert u["occ"] >= 2, (key, u)
        assert u["vgpr"] == VGPRS[key], (key, u)
