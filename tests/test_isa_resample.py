"""Resource usage of the rational resampler's kernel (k_resample, docs/SPEC.md 3.0b) for every input format, from a gfx950
cross-compile with -Rpass-analysis=kernel-resource-usage, as tests/test_isa_wide.py does for K0 and K6: no scratch, static LDS
within 64 KB, and the registers and occupancy DESIGN.md section 4 records.  Resource usage only; needs no GPU."""
import os
import subprocess

from test_isa_wide import _usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "p25rx_amd", "csrc")
REMARKS = "/tmp/p25fe_resource.txt"

# instantiation (mangled template arguments: format, table looked up) -> VGPRs of the kernel as committed: a regression guard, not a
# budget (the launch bound is 2 waves per SIMD = 256 registers; the cf32 instance holds 16 prefetched vectors, s16 8, u8 4)
VGPRS = {"Li0ELb0E": 180, "Li2ELb0E": 160, "Li1ELb0E": 132, "Li1ELb1E": 136}
# what the register pin stands for: the compiler's waves per SIMD, and the register count at which an instance would lose one
# (168 registers are three waves' share; cf32 runs two at anything up to the launch bound's 256).  k_tune's are the same
WAVES = {"Li0ELb0E": 2, "Li2ELb0E": 3, "Li1ELb0E": 3, "Li1ELb1E": 3}
VGPR_STEP = {"Li0ELb0E": 256, "Li2ELb0E": 168, "Li1ELb0E": 168, "Li1ELb1E": 168}
WINDOW_BYTES = 2040 * 8                                              # RS_NIN complex samples; the table is dynamic LDS (<= 16.5 KB)


def _remarks():
    """this tree's remarks: compiled afresh unless the file is newer than every source it is made from"""
    srcs = [os.path.join(CSRC, f) for f in ("p25fe_api.hip", "p25fe_kernels.hip", "p25fe_recv.hip", "Makefile")]
    srcs += [os.path.join(ROOT, "include", f) for f in ("p25fe.h", "p25fe_spec.h")]
    if not os.path.exists(REMARKS) or os.path.getmtime(REMARKS) < max(os.path.getmtime(s) for s in srcs) or "Function Name" not in open(REMARKS).read():
        subprocess.check_call(["make", "-s", "-C", CSRC, "asm"], env=dict(os.environ, HIPCC=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))
    return open(REMARKS).read()


def test_resampler_kernels_use_no_scratch_and_fit_the_lds():
    use = {n: u for n, u in _usage(_remarks()).items() if n.startswith("_ZN4p25k10k_resampleILi")}
    # cf32, s16, u8 with the table as arithmetic, u8 with the table looked up
    assert len(use) == 4 and sum("Lb1E" in n for n in use) == 1, sorted(use)
    for name, u in sorted(use.items()):
        print(name, u)
        key = name[len("_ZN4p25k10k_resampleI"):][:8]
        assert u["scratch"] == 0, (name, u)
        assert u["lds"] == WINDOW_BYTES + (1024 if "Lb1E" in name else 0), (name, u)
        assert u["lds"] + 4 * (4096 + 32) <= 65536                   # with the largest table in dynamic LDS
        assert u["occ"] == WAVES[key] and u["vgpr"] <= VGPR_STEP[key], (name, u)
        assert u["vgpr"] == VGPRS[key], (name, u)
