"""The host-only functions of the tuner's cuts (p25fe_cuts_from_keys, p25fe_cuts_create's checks; docs/SPEC.md 3.0j) under
AddressSanitizer + UBSan: a stand-alone program (tests/native/tune_cuts_host_driver.cpp) linked against the host-side sanitizer
build of the library, exactly as tests/test_tune_nco_sanitizers.py does.  Host code only; no GPU."""
import os
import subprocess

from test_sanitizers import ROOT, run_clean


def test_tuner_cuts_host_functions_under_asan_ubsan():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "p25rx_amd", "csrc"), "asan"], env=dict(os.environ, HIPCC=hipcc))
    exe = os.path.join(ROOT, "build", "tune_cuts_host_asan")
    # host code only is instrumented (the driver has no device code), as for tests/native/tune_nco_host_driver.cpp
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "tune_cuts_host_driver.cpp"), "-L" + os.path.join(ROOT, "build"),
                           "-lp25fe_asan", "-Wl,-rpath," + os.path.join(ROOT, "build"), "-Wl,-rpath,/opt/rocm/lib"])
    assert "tune cuts host driver ok" in run_clean(exe)
