"""p25fe_replay -r RATE_HZ -T MS: the survey over time (docs/SPEC.md 3.0i) from the command line.  The usage errors need no GPU and
end as every other one does (tests/test_replay_cli.py): status 2 and the usage text before anything is opened.  On the GPU the keyed
scene of tests/waterfall_model.py, written as a u8 file, gives one `activity` event with the five intervals and status 0."""
import json
import os

import pytest

import scan_model as SM
import waterfall_model as WM
from test_replay_cli import replay

RATE = ["-r", "2500000"]
USAGE_ERRORS = {
    "-T without -r": ["-T", "5"],
    "-T 0": RATE + ["-T", "0"],
    "-T -1": RATE + ["-T", "-1"],
    "-T 60001": RATE + ["-T", "60001"],
    "-T 5x": RATE + ["-T", "5x"],
    "-T nan": RATE + ["-T", "nan"],
    "-T without its value": RATE + ["-T"],
    "-T with -S": RATE + ["-T", "5", "-S", "50"],
    "-T with -f": RATE + ["-T", "5", "-f", "12500"],
    "-T with -F": RATE + ["-T", "5", "-F", "12500.5"],
    "-T with -a": RATE + ["-T", "5", "-F", "12500.5", "-a", "50"],
    "-T with -A": RATE + ["-T", "5", "-F", "12500.5", "-A", "50"],
    "-T with -w": RATE + ["-T", "5", "-w", "bb.f32"],
    "-T with -j": RATE + ["-T", "5", "-j", "ev.jsonl"],
    "-T with -b": RATE + ["-T", "5", "-b", "64"],
    "-T with -W": ["-W", "1M", "-T", "5"],
    "-T with -W and -r": RATE + ["-W", "1M", "-T", "5"],
    "more than 2^20 frames a slot": ["-r", "4000000000", "-T", "60000"],
}


@pytest.mark.parametrize("case", sorted(USAGE_ERRORS))
def test_usage_error_before_anything_is_opened(tmp_path, case):
    src, out = tmp_path / "in.bin", tmp_path / "dibits.out"
    src.write_bytes(bytes(64))
    r = replay(USAGE_ERRORS[case] + ["u8", str(src), str(out)])
    assert r.returncode == 2 and "usage" in r.stderr and "-T MS" in r.stderr, (case, r.returncode, r.stderr[-500:])
    assert "-S MS" in r.stderr and "-W WINDOW_BYTES" in r.stderr     # the lines the other CLI tests look for are still there
    assert "no usable HIP device" not in r.stderr and r.stdout == ""
    assert os.listdir(tmp_path) == ["in.bin"]


@pytest.mark.gpu
def test_activity_of_a_u8_file(tmp_path):
    """-r 2500000 -T 5 on the keyed scene as u8: 5 ms at 2.5 Msps is 6.1 frames of hop 2048, so slots of 6 frames (4.9152 ms), 51
    of them; one `activity` event on stdout with the five intervals by first slot -- the raster indices, the times of the slots
    within one slot of the truth, offsets within 200 Hz, at least 35 dB over the floor; status 0, no output file"""
    x = WM.keyed_scene()
    src, out = tmp_path / "cap.u8", tmp_path / "dib.out"
    SM.to_u8(x).tofile(src)
    r = replay(RATE + ["-T", "5", "u8", str(src), str(out)])
    assert r.returncode == 0, r.stderr[-1000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    ev = json.loads(lines[0])
    slot_ms = WM.KEY_SLOT * 1000.0 / WM.KEY_FS
    assert ev["event"] == "activity" and ev["slot_frames"] == WM.KEY_B and ev["n_slots"] == 51 and "truncated" not in ev
    assert ev["slot_ms"] == pytest.approx(slot_ms, abs=1e-4)
    truth = WM.keyed_truth()
    assert len(ev["keys"]) == len(truth) == 5
    for k, (r_idx, a, b, off) in zip(ev["keys"], truth):
        assert sorted(k) == ["centre_hz", "db_over_floor", "first_ms", "last_ms", "offset_hz", "raster_index"]
        assert k["raster_index"] == r_idx and k["centre_hz"] == r_idx * 12500.0 and k["db_over_floor"] >= 35.0
        assert abs(k["first_ms"] / slot_ms - a) <= 1.001 and abs(k["last_ms"] / slot_ms - (b + 1)) <= 1.001, (k, a, b)
        assert abs(k["offset_hz"] - off) <= 200.0, (k, off)
    assert not out.exists() and sorted(os.listdir(tmp_path)) == ["cap.u8"]
