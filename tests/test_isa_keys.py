"""Resource usage of the kernels that compute the keys on the device (docs/SPEC.md 3.0k: k_keys_pow, k_keys_walk, k_keys_cell) from
a gfx950 cross-compile with -Rpass-analysis=kernel-resource-usage, by tests/test_isa_waterfall.py's method: no scratch, static LDS
within 64 KB -- k_keys_pow's is the sort's 8 bytes for each of the 4096 channels the object admits --, at least one workgroup per
CU, and the registers as committed.  Resource usage only; needs no GPU."""
import os
import subprocess

from test_isa_resample import CSRC, REMARKS, _remarks
from test_isa_wide import _usage

PREFIX = "_ZN4p25k"
# kernel -> (VGPRs as committed: a regression guard, not a budget; static LDS in bytes; waves per workgroup).  k_keys_walk holds 16
# rows' powers and floors in registers before it looks at the first: 64 of its registers are those loads in flight
KERNELS = {"10k_keys_pow": (14, 8 * 4096, 4), "11k_keys_walk": (88, 0, 1), "11k_keys_cell": (24, 2 * 64 * 16, 1)}


def _keys_remarks():
    """this tree's remarks: test_isa_resample's, compiled afresh when the kernels' source is newer than they are"""
    newest = os.path.getmtime(os.path.join(CSRC, "p25fe_keys.inc"))
    if os.path.exists(REMARKS) and os.path.getmtime(REMARKS) < newest:
        subprocess.check_call(["make", "-s", "-C", CSRC, "asm"], env=dict(os.environ, HIPCC=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))
    return _remarks()


def test_keys_kernels_use_no_scratch_and_fit_a_cu():
    use = {n[len(PREFIX):].split("ENS_")[0]: u for n, u in _usage(_keys_remarks()).items() if n.startswith(PREFIX) and "k_keys_" in n}
    assert sorted(use) == sorted(KERNELS), sorted(use)
    for key, u in sorted(use.items()):
        print(key, u)
        vgpr, lds, waves = KERNELS[key]
        assert u["scratch"] == 0, (key, u)
        assert u["lds"] == lds and u["lds"] <= 64 * 1024, (key, u)
        # a workgroup fits a CU: its waves within the four SIMDs' occupancy, its LDS within the CU's (checked above)
        assert u["occ"] >= 1 and 4 * u["occ"] >= waves, (key, u)
        assert u["vgpr"] == vgpr, (key, u)
