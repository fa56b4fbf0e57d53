"""Resource usage of K0 (k_predecim, k_predecim_fmt) and K6 (k_channelise, k_channelise_fmt) for every wideband input format,
from a gfx950 cross-compile with -Rpass-analysis=kernel-resource-usage: no scratch, and the occupancy and LDS the stages are built
for (docs/MEASUREMENTS.md records the numbers).  Resource usage only; needs no GPU."""
import os
import re
import subprocess
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _usage(text):
    out = {}
    for blk in text.split("Function Name: ")[1:]:
        name = blk.split()[0]

        def num(pat):
            return int(re.search(pat, blk).group(1))
        out[name] = dict(vgpr=num(r"VGPRs: (\d+)"), sgpr=num(r"SGPRs: (\d+)"), scratch=num(r"ScratchSize \[bytes/lane\]: (\d+)"),
                         lds=num(r"LDS Size \[bytes/block\]: (\d+)"), occ=num(r"Occupancy \[waves/SIMD\]: (\d+)"))
    return out


def test_wide_format_kernels_use_no_scratch():
    t0 = time.time()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "p25rx_amd", "csrc"), "asm"],
                          env=dict(os.environ, HIPCC=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))
    assert os.path.getmtime("/tmp/p25fe_resource.txt") >= t0 - 1.0        # this compile's remarks, not an earlier one's
    use = _usage(open("/tmp/p25fe_resource.txt").read())
    k0 = {n: u for n, u in use.items() if n.startswith(("_ZN4p25k10k_predecimE", "_ZN4p25k14k_predecim_fmtILi"))}
    k6 = {n: u for n, u in use.items() if n.startswith(("_ZN4p25k12k_channeliseE", "_ZN4p25k16k_channelise_fmtILi"))}
    # per stage: cf32, s16, u8 with the table as arithmetic, u8 with the table looked up
    assert len(k0) == 4 and len(k6) == 4, (sorted(k0), sorted(k6))
    # the recorded numbers of the stages: K0 is built for 2 waves per SIMD with 17936 B of LDS, K6 for 3 with 7696 B
    for fam, occ, lds in ((k0, 2, 17936), (k6, 3, 7696)):
        assert sum("Lb1E" in n for n in fam) == 1, sorted(fam)
        for name, u in fam.items():
            assert u["scratch"] == 0, (name, u)
            assert u["occ"] >= occ, (name, u)
            assert u["lds"] == lds + (1024 if "Lb1E" in name else 0), (name, u)   # the 256-entry table only where it is looked up
