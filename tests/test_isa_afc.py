"""Resource usage of the AFC measure kernel (docs/SPEC.md 3.0f: k_afc_measure) from a gfx950 cross-compile with
-Rpass-analysis=kernel-resource-usage, as tests/test_isa_tune_nco.py does for k_tune_nco (which is also the kernel of 3.0e, the NCO
tuner with a phase offset): no scratch, the static LDS within 64 KB, and the registers as committed.  Resource usage only; needs
no GPU."""
import os
import re

from test_isa_resample import CSRC, WINDOW_BYTES, _remarks
from test_isa_wide import _usage

# VGPRs of the kernel as committed: a regression guard, not a budget
MEASURE = "_ZN4p25k13k_afc_measureE"
MEASURE_VGPRS = 94


def test_measure_kernel_uses_no_scratch_and_fits_the_lds():
    use = {n: u for n, u in _usage(_remarks()).items() if n.startswith(MEASURE)}
    assert len(use) == 1, sorted(use)
    (name, u), = use.items()
    print(name, u)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(CSRC)), "include", "p25fe.h")).read()
    max_t = int(re.search(r"#define P25FE_AFC_MAX_T (\d+)", hdr).group(1))
    # static only (the kernel is launched with no dynamic LDS): the window, the taps, one w per slot of the tile
    assert u["scratch"] == 0 and u["lds"] == WINDOW_BYTES + 4 * max_t + 8 * 256 and u["lds"] <= 65536, u
    assert u["vgpr"] == MEASURE_VGPRS and u["occ"] >= 2, u


def test_the_lint_walks_the_afc_kernels():
    """tools/isa_lint.py follows the hand-issued LDS reads of rs_fir in k_afc_measure too, and finds nothing"""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("isa_lint", os.path.join(root, "tools", "isa_lint.py"))
    lint = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lint)
    _remarks()
    asm = "/tmp/p25fe_api-hip-amdgcn-amd-amdhsa-gfx950.s"
    src = open(asm).read()
    assert len(re.findall(r"^%s\w+:" % MEASURE, src, re.M)) == 1
    text = open(os.path.join(root, "tools", "isa_lint.py")).read()
    assert re.search(r"13k_afc_measure", text)
    bad, warn, nk, nr = lint.lint(asm)
    assert not bad and nr > 0, bad[:5]
