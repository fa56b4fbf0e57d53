"""Resource usage of the tuner's kernel (k_tune, docs/SPEC.md 3.0c) for every input format, from a gfx950 cross-compile with
-Rpass-analysis=kernel-resource-usage, as tests/test_isa_resample.py does for k_resample: no scratch, static plus the largest
dynamic LDS of an accepted tuner within 64 KB, and the registers and occupancy DESIGN.md section 4 (K0c) records.  Resource usage
only; needs no GPU."""
import os
import re

from test_isa_resample import CSRC, VGPR_STEP, WAVES, WINDOW_BYTES, _remarks
from test_isa_wide import _usage

# instantiation (mangled template arguments: format, table looked up) -> VGPRs of the kernel as committed: a regression guard, not a
# budget (the launch bound is 2 waves per SIMD = 256 registers)
VGPRS = {"Li0ELb0E": 183, "Li2ELb0E": 162, "Li1ELb0E": 138, "Li1ELb1E": 140}
# the largest dynamic LDS p25fe_tuner_create can ask for: L * (T | 1) <= 4096 + 32 floats of taps, rounded up to a pair, and the
# rotator of the largest denominator that is copied to LDS (TN_ROT_LDS_DEN pairs); larger ones are gathered from global memory
ROT_LDS_DEN = int(re.search(r"constexpr int TN_ROT_LDS_DEN = (\d+);", open(os.path.join(CSRC, "p25fe_kernels.hip")).read()).group(1))
DYNAMIC_MAX = 4 * (4096 + 32) + 8 * ROT_LDS_DEN


def test_tuner_kernels_use_no_scratch_and_fit_the_lds():
    use = {n: u for n, u in _usage(_remarks()).items() if n.startswith("_ZN4p25k6k_tuneILi")}
    # cf32, s16, u8 with the table as arithmetic, u8 with the table looked up
    assert len(use) == 4 and sum("Lb1E" in n for n in use) == 1, sorted(use)
    for name, u in sorted(use.items()):
        print(name, u)
        key = name[len("_ZN4p25k6k_tuneI"):][:8]
        assert u["scratch"] == 0, (name, u)
        assert u["lds"] == WINDOW_BYTES + (1024 if "Lb1E" in name else 0), (name, u)
        assert ROT_LDS_DEN == 512 and u["lds"] + DYNAMIC_MAX <= 65536
        assert u["occ"] == WAVES[key] and u["vgpr"] <= VGPR_STEP[key], (name, u)
        assert u["vgpr"] == VGPRS[key], (name, u)
