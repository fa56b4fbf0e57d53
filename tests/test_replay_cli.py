"""p25fe_replay's command line, without a GPU: every usage error is reported -- exit status 2, the usage text -- before the input is
opened, before any output is created or truncated and before p25fe_create, so each of these cases ends the same way with or without
a device.

Before the driver parsed its options in one place, the -W combinations, -r with bb and the unknown mode were found only after
p25fe_create: without a device those invocations ended in the handle's abort instead, and with one the unknown mode had already
truncated the output.  That they now end here like every other usage error is the point of these cases."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "p25fe_replay")

W = ["-W", "1M"]
USAGE_ERRORS = {
    # (options, mode); None: the positional arguments are part of the options
    "option without its value": (["-b"], None),
    "unknown option": (["-x", "1"], "u8"),
    "-b 0": (["-b", "0"], "u8"),
    "-r 0": (["-r", "0"], "u8"),
    "-r 4294967296": (["-r", "4294967296"], "u8"),
    "-f without -r": (["-f", "137500"], "cf32"),
    "-F without -r": (["-F", "135289.3"], "cf32"),
    "-f then -F": (["-r", "2500000", "-f", "137500", "-F", "135289.3"], "cf32"),
    "-F then -f": (["-r", "2500000", "-F", "135289.3", "-f", "137500"], "cf32"),
    "-a without -F": (["-r", "2500000", "-a", "50"], "cf32"),
    "-a with -f": (["-r", "2500000", "-f", "137500", "-a", "50"], "cf32"),
    "-a 0": (["-r", "2500000", "-F", "137500", "-a", "0"], "cf32"),
    "-a 60001": (["-r", "2500000", "-F", "137500", "-a", "60001"], "cf32"),
    "-a 5x": (["-r", "2500000", "-F", "137500", "-a", "5x"], "cf32"),
    "-F 1e3x": (["-r", "2500000", "-F", "1e3x"], "cf32"),
    "two positional arguments": (["u8", "IN"], None),
    "four positional arguments": (["u8", "IN", "OUT", "extra"], None),
    "unknown mode": ([], "u16"),
    "-r with bb": (["-r", "2500000"], "bb"),
    "-W with bb": (W, "bb"),
    "-W with -w": (W + ["-w", "BB"], "u8"),
    "-W with -j": (W + ["-j", "EVENTS"], "u8"),
    "-W with -r": (W + ["-r", "2500000"], "u8"),
    "-W with -f": (W + ["-f", "137500"], "u8"),
    "-W with -F": (W + ["-F", "135289.3"], "u8"),
    "-W with -a": (W + ["-a", "50"], "u8"),
}


def replay(args):
    assert os.path.exists(EXE), "run __graft_entry__.build()"
    return subprocess.run([EXE] + args, capture_output=True, text=True, timeout=100)


@pytest.fixture
def files(tmp_path):
    src = tmp_path / "in.bin"
    src.write_bytes(bytes(64))
    return src, tmp_path / "dibits.out"


@pytest.mark.parametrize("case", sorted(USAGE_ERRORS))
def test_usage_error_before_anything_is_opened(files, tmp_path, case):
    src, out = files
    opts, mode = USAGE_ERRORS[case]
    named = {"IN": str(src), "OUT": str(out), "BB": str(tmp_path / "bb.f32le"), "EVENTS": str(tmp_path / "ev.jsonl")}
    args = [named.get(a, a) for a in opts] + ([mode, str(src), str(out)] if mode is not None else [])
    r = replay(args)
    assert r.returncode == 2 and "usage" in r.stderr, (args, r.returncode, r.stderr[-500:])
    assert "no usable HIP device" not in r.stderr
    assert not out.exists()
    assert os.listdir(tmp_path) == ["in.bin"]                         # nor a -w recording, nor -j events


def test_missing_input(tmp_path):
    """a valid command line gets past the parser: the missing input is what ends it, before any output exists"""
    out = tmp_path / "dibits.out"
    r = replay(["-b", "1", "u8", str(tmp_path / "none.u8"), str(out)])
    assert r.returncode == 1 and "unable to open" in r.stderr and "usage" not in r.stderr
    assert not out.exists()


def test_valid_command_line_reaches_the_handle(files):
    """a valid command line with an existing input goes on to p25fe_create: without a device that is the abort of Handle (the
    reference's panic = abort); with one the 32 samples give no dibit"""
    import torch
    src, out = files
    r = replay(["-b", "1", "u8", str(src), str(out)])
    assert "usage" not in r.stderr
    if torch.cuda.is_available():
        assert r.returncode == 0 and out.read_bytes() == b"", r.stderr[-500:]
    else:
        assert r.returncode != 0 and "no usable HIP device" in r.stderr
