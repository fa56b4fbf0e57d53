"""Resource usage of the u8 / s16 forms of K0 (k_predecim_fmt) and K6 (k_channelise_fmt), from a gfx950 cross-compile with
-Rpass-analysis=kernel-resource-usage: no scratch, and no more registers or LDS than the occupancy the cf32 kernels are built for
allows.  Resource usage only; needs no GPU."""
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
    k0 = {n: u for n, u in use.items() if n.startswith("_ZN4p25k14k_predecim_fmtILi")}
    k6 = {n: u for n, u in use.items() if n.startswith("_ZN4p25k16k_channelise_fmtILi")}
    # per stage: s16, u8 with the table as arithmetic, u8 with the table looked up
    assert len(k0) == 3 and len(k6) == 3, (sorted(k0), sorted(k6))
    ref0, ref6 = use["_ZN4p25k10k_predecimENS_6K0ArgsE"], use["_ZN4p25k12k_channeliseENS_7ChzArgsE"]
    assert ref0["scratch"] == 0 and ref6["scratch"] == 0
    for fam, ref in ((k0, ref0), (k6, ref6)):
        for name, u in fam.items():
            assert u["scratch"] == 0, (name, u)
            assert u["occ"] >= ref["occ"], (name, u, ref)                 # as many waves per SIMD as the cf32 kernel
            assert u["lds"] <= ref["lds"] + 1024, (name, u, ref)          # the same rows, plus the 256-entry table where it is looked up
