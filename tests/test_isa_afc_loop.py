"""Resource usage of the AFC loop's kernel (docs/SPEC.md 3.0g: k_afc_loop) from a gfx950 cross-compile with
-Rpass-analysis=kernel-resource-usage, as tests/test_isa_afc.py does for k_afc_measure: one kernel of that name, no scratch, no
LDS, and the registers as committed.  Resource usage only; needs no GPU."""
from test_isa_resample import _remarks
from test_isa_wide import _usage

LOOP = "_ZN4p25k10k_afc_loopE"
# VGPRs of the kernel as committed: a regression guard, not a budget
LOOP_VGPRS = 88


def test_loop_kernel_uses_no_scratch_and_no_lds():
    use = {n: u for n, u in _usage(_remarks()).items() if n.startswith(LOOP)}
    assert len(use) == 1, sorted(use)
    (name, u), = use.items()
    print(name, u)
    assert u["scratch"] == 0 and u["lds"] == 0, u
    assert u["vgpr"] == LOOP_VGPRS, u
