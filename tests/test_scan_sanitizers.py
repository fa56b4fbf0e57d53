"""The host-only functions of the survey (p25fe_scan_window, p25fe_scan_channels and the refusals of p25fe_scan_create,
p25fe_scan_dev, p25fe_scan, p25fe_scan_read, p25fe_scan_reset; docs/SPEC.md 3.0h) under AddressSanitizer + UBSan: a stand-alone
program (tests/native/scan_host_driver.cpp) linked against the host-side sanitizer build of the library, exactly as
tests/test_afc_sanitizers.py does.  Host code only; no GPU."""
import os
import subprocess

from test_sanitizers import ROOT, run_clean


def test_scan_host_functions_under_asan_ubsan():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "p25rx_amd", "csrc"), "asan"], env=dict(os.environ, HIPCC=hipcc))
    exe = os.path.join(ROOT, "build", "scan_host_asan")
    # host code only is instrumented (the driver has no device code), as for tests/native/afc_host_driver.cpp
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "scan_host_driver.cpp"), "-L" + os.path.join(ROOT, "build"),
                           "-lp25fe_asan", "-Wl,-rpath," + os.path.join(ROOT, "build"), "-Wl,-rpath,/opt/rocm/lib"])
    assert "scan host driver ok" in run_clean(exe)
