"""p25fe_replay -r RATE_HZ -S MS: the survey (docs/SPEC.md 3.0h) from the command line.  The usage errors need no GPU and end as
every other one does (tests/test_replay_cli.py): status 2 and the usage text before anything is opened.  On the GPU the scene of
tests/scan_model.py, written as a u8 file, gives one `scan` event with the four raster channels and status 0; with -F the run goes on
from the start of the input and decodes the tuned channel."""
import json
import os

import numpy as np
import pytest

import scan_model as SM
from test_replay_cli import replay

USAGE_ERRORS = {
    "-S without -r": ["-S", "50"],
    "-S 0": ["-r", "2500000", "-S", "0"],
    "-S 60001": ["-r", "2500000", "-S", "60001"],
    "-S 5x": ["-r", "2500000", "-S", "5x"],
    "-S with -W": ["-W", "1M", "-S", "50"],
    "-S without its value": ["-r", "2500000", "-S"],
}


@pytest.mark.parametrize("case", sorted(USAGE_ERRORS))
def test_usage_error_before_anything_is_opened(tmp_path, case):
    src, out = tmp_path / "in.bin", tmp_path / "dibits.out"
    src.write_bytes(bytes(64))
    r = replay(USAGE_ERRORS[case] + ["u8", str(src), str(out)])
    assert r.returncode == 2 and "usage" in r.stderr and "-S MS" in r.stderr, (case, r.returncode, r.stderr[-500:])
    assert "no usable HIP device" not in r.stderr and r.stdout == ""
    assert os.listdir(tmp_path) == ["in.bin"]


@pytest.mark.gpu
def test_survey_of_a_u8_file(tmp_path):
    """-r 2500000 -S 50 on the scene as u8: one `scan` event on stdout with the raster indices {-33, 0, 11, 12}, each at least 35 dB
    over the floor and within 200 Hz of its true offset, 61 frames of 4096 at hop 2048 in 125000 samples; status 0, no output file.
    With -F at a surveyed frequency the event also goes to the -j file and the run decodes the channel from the start of the input."""
    x, truths = SM.scene()
    src, out, js = tmp_path / "cap.u8", tmp_path / "dib.out", tmp_path / "ev.jsonl"
    SM.to_u8(x).tofile(src)
    r = replay(["-r", str(SM.SCENE_FS), "-S", "50", "u8", str(src), str(out)])
    assert r.returncode == 0, r.stderr[-1000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    ev = json.loads(lines[0])
    assert ev["event"] == "scan" and ev["n_frames"] == 125000 // 2048
    got = {c["raster_index"]: c for c in ev["channels"]}
    assert set(got) == set(SM.SCENE_CHANNELS) and len(ev["channels"]) == 4
    for r_idx, c in got.items():
        assert c["centre_hz"] == r_idx * 12500.0 and c["db_over_floor"] >= 35.0
        assert abs(c["offset_hz"] - SM.SCENE_CHANNELS[r_idx]) <= 200.0, c
    assert not out.exists()
    c = got[11]
    r = replay(["-j", str(js), "-r", str(SM.SCENE_FS), "-S", "50", "-F", "%.1f" % (c["centre_hz"] + c["offset_hz"]), "u8", str(src), str(out)])
    assert r.returncode == 0, r.stderr[-1000:]
    assert json.loads(r.stdout.splitlines()[0]) == ev
    assert [json.loads(ln) for ln in open(js) if '"scan"' in ln] == [ev]
    dib = np.fromfile(out, dtype=np.uint8)
    kk = min(len(dib), len(truths[1]) - 24)
    assert kk > 1100 and np.array_equal(dib[:kk], truths[1][24:24 + kk])
