"""Resource usage of the AFC kernels (docs/SPEC.md 3.0e: k_tune_nco_ph, the NCO tuner with a phase offset, in four formats; 3.0f:
k_afc_measure) from a gfx950 cross-compile with -Rpass-analysis=kernel-resource-usage, as tests/test_isa_tune_nco.py does for
k_tune_nco: no scratch, static plus the largest dynamic LDS within 64 KB, k_tune_nco's waves per SIMD for the phase-offset kernels,
and the registers as committed.  Resource usage only; needs no GPU."""
import os
import re

from test_isa_resample import CSRC, VGPR_STEP, WAVES, WINDOW_BYTES, _remarks
from test_isa_tune_nco import DYNAMIC_MAX
from test_isa_tune_nco import PREFIX as NCO_PREFIX
from test_isa_wide import _usage

# instantiation (mangled template arguments: format, table looked up) -> VGPRs of the kernel as committed: a regression guard, not a
# budget (the launch bound is 2 waves per SIMD = 256 registers)
VGPRS = {"Li0ELb0E": 182, "Li2ELb0E": 156, "Li1ELb0E": 134, "Li1ELb1E": 138}
PREFIX = "_ZN4p25k13k_tune_nco_phI"
MEASURE = "_ZN4p25k13k_afc_measureE"
MEASURE_VGPRS = 94


def test_phase_offset_kernels_use_no_scratch_and_fit_the_lds():
    all_use = _usage(_remarks())
    use = {n: u for n, u in all_use.items() if n.startswith(PREFIX + "Li")}
    nco = {n[len(NCO_PREFIX):][:8]: u for n, u in all_use.items() if n.startswith(NCO_PREFIX + "Li")}
    # cf32, s16, u8 with the table as arithmetic, u8 with the table looked up
    assert len(use) == 4 and sum("Lb1E" in n for n in use) == 1 and len(nco) == 4, sorted(use)
    for name, u in sorted(use.items()):
        print(name, u)
        key = name[len(PREFIX):][:8]
        assert u["scratch"] == 0, (name, u)
        assert u["lds"] == WINDOW_BYTES + (1024 if "Lb1E" in name else 0), (name, u)
        assert u["lds"] + DYNAMIC_MAX <= 65536                       # the dynamic part is k_tune_nco's: the same object launches both
        assert u["occ"] == nco[key]["occ"] == WAVES[key] and u["vgpr"] <= VGPR_STEP[key], (name, u)
        assert u["vgpr"] == VGPRS[key], (name, u)


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
    """tools/isa_lint.py follows the hand-issued LDS reads of rs_fir in the five new kernels too, and finds nothing"""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("isa_lint", os.path.join(root, "tools", "isa_lint.py"))
    lint = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lint)
    _remarks()
    asm = "/tmp/p25fe_api-hip-amdgcn-amd-amdhsa-gfx950.s"
    src = open(asm).read()
    assert len(re.findall(r"^%sLi\w+:" % PREFIX, src, re.M)) == 4 and len(re.findall(r"^%s\w+:" % MEASURE, src, re.M)) == 1
    text = open(os.path.join(root, "tools", "isa_lint.py")).read()
    assert re.search(r"13k_tune_nco_ph", text) and re.search(r"13k_afc_measure", text)
    bad, warn, nk, nr = lint.lint(asm)
    assert not bad and nr > 0, bad[:5]
