"""The keys computed on the device (docs/SPEC.md 3.0k: k_keys_pow, k_keys_walk, k_keys_cell) against the host function, which is
the definition.  One yardstick everywhere: the bytes of Keys.read() -- the count and the whole 48-byte records -- equal the bytes of
Scanner.keys (p25fe_waterfall_keys) on the same rows copied back, with the same parameters.  There is no tolerance.

The synthetic rows are written to the device directly, seeded, and made of what the rule has to tell apart: noise words of 2^20 to
2^40, keyed runs at 200 times the noise, runs at 50 times (between the off and the on threshold: they hold an interval and start
none), rows of zero frames inside runs, rows with frames and no power at all (a floor of zero: what is on stays on and peaks at
+inf), rows where all but a few channels are zero, words from 2^63 to 2^64 - 1, runs that reach the last row and runs shorter than
min_slots.  Whether a case really contains them is asked of the host function alone (test_the_cases_contain_what_they_are_for)."""
import ctypes as C
import functools

import numpy as np
import pytest

import scan_model as SM
import waterfall_model as WM
from test_gpu_wide_fmt import dev

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A5A5A5A5A
FRAMES = 6
# shape -> (N, fs, raster): 19 channels (less than a wave), 199 (no multiple of 64), 799 (past 256 and 512 lanes), 3199 (near the limit)
SHAPES = {"c19": (1024, 250000, 12500.0), "c199": (4096, 2500000, 12500.0), "c799": (4096, 10000000, 12500.0),
          "c3199": (4096, 20000000, 6250.0)}
CHANNELS = {"c19": 19, "c199": 199, "c799": 799, "c3199": 3199}
MIN_SLOTS = {1: 1, 2: 1, 7: 2, 65: 5, 300: 2}
# name -> (shape, n_rows, the rule's parameters, slot0, row stride beyond N + 1)
CASES = {"%s_%d" % (s, n): (s, n, dict(min_slots=MIN_SLOTS[n]), 0, 0) for s in SHAPES for n in (1, 2, 7, 65, 300)}
CASES.update({
    "on_equals_off": ("c199", 65, dict(on_db=17.0, off_db=17.0, min_slots=2), 0, 0),
    "half_bw_zero": ("c199", 65, dict(half_bw_hz=0.0, min_slots=1), 0, 0),
    "shared_bins": ("c199", 65, dict(half_bw_hz=20000.0, min_slots=2), 0, 0),
    "slot0_past_2_40": ("c19", 65, dict(min_slots=2), (1 << 40) + 3, 0),
    "padded_rows": ("c199", 7, dict(min_slots=2), 5, 4),
})


def channels_of(N, fs, raster):
    """eligible raster indices and, per channel, the bins of its raster cell (waterfall_model.keys' rule)"""
    fb = SM.bin_hz(N, fs)
    rmax = int(np.floor((fs / 2.0 - raster / 2.0) / raster))
    rs = [r for r in range(-rmax, rmax + 1) if abs(r * raster) + raster / 2.0 <= fs / 2.0]
    return rs, [np.flatnonzero(np.abs(fb - r * raster) <= raster / 2.0) for r in rs]


@functools.lru_cache(maxsize=None)
def synthetic(shape, n, seed):
    """uint64 [n, N + 1], made once per case and never changed: see the module's text.  Six keyed channels (twelve where the
    raster has more than 48), spread over the raster, each with its own pattern of runs"""
    N, fs, raster = SHAPES[shape]
    rng = np.random.default_rng(seed)
    rs, cells = channels_of(N, fs, raster)
    assert len(rs) == CHANNELS[shape]
    level = 1 << int(rng.choice([20, 30, 40]))
    rows = rng.integers(3 * level // 4, level, size=(n, N + 1), dtype=np.uint64)
    rows[:, N] = FRAMES
    keyed = [int(c) for c in rng.choice(len(rs), size=6 if len(rs) <= 48 else 12, replace=False)]

    def run(c, a, b, gain):
        rows[a:b, cells[c]] *= np.uint64(gain)
    for i, c in enumerate(keyed):
        kind = i % 6
        if kind == 0:                                                # from the first row to the last
            run(c, 0, n, 200)
        elif kind == 1:                                              # reaches the last row; held at 50 in its middle third; huge words
            a = n // 4
            run(c, a, n, 200)
            if n >= 7:
                rows[a + (n - a) // 3:a + 2 * (n - a) // 3, cells[c]] //= np.uint64(4)
                big = rng.integers(1 << 63, (1 << 64) - 1, size=len(cells[c]), dtype=np.uint64, endpoint=True)
                big[0] = (1 << 64) - 1
                rows[a + 1, cells[c]] = big
        elif kind == 2:                                              # 50 alone never starts an interval
            run(c, 0, n, 50)
        elif kind == 3:                                              # one row: dropped unless min_slots is 1
            run(c, n // 2 + (1 if n >= 7 else 0), n // 2 + (2 if n >= 7 else 1), 200)
        elif kind == 4:                                              # ends one row short of the end
            run(c, 0, max(1, n - 1), 200)
        else:                                                        # two runs
            run(c, 0, n // 3, 200)
            run(c, n // 2, n, 200)
    if n >= 7:
        rows[1, :N] = 0                                              # all channels zero but two: a floor of zero
        for c in keyed[:2]:
            rows[1, cells[c]] = level
        rows[n // 2, N] = 0                                          # no frame, whatever the words say
        rows[n // 2 + 2, :N] = 0                                     # frames and no power at all
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (N, fs, the rows, the host function's keyword arguments, slot0, padding words per row)"""
    shape, n, kw, slot0, pad = CASES[name]
    N, fs, raster = SHAPES[shape]
    return N, fs, synthetic(shape, n, sorted(CASES).index(name) + 100), dict(kw, raster_hz=raster), slot0, pad


@functools.lru_cache(maxsize=None)
def host_keys(name):
    from p25rx_amd import Scanner
    N, fs, rows, kw, slot0, _pad = case(name)
    got = Scanner.keys(rows, fs, slot0=slot0, **kw)
    got.setflags(write=False)
    return got


class Rig:
    def __init__(self):
        from p25rx_amd import _lib, Scanner
        from p25rx_amd.frontend import FrontEnd
        self.lib, self.Scanner, self.fe = _lib, Scanner, FrontEnd()
        self.scanners = {}

    def scanner(self, N, hop=None):
        key = (N, hop)
        if key not in self.scanners:
            self.scanners[key] = self.Scanner(self.fe, N, hop)
        return self.scanners[key]


@pytest.fixture(scope="module")
def rig():
    return Rig()


def to_device(rows, pad=0):
    """uint64 host rows -> (the whole device buffer, int64 [n, N + 1 + pad] with the padding poisoned; the rows as a view of it)"""
    import torch
    buf = np.full((rows.shape[0], rows.shape[1] + pad), POISON, dtype=np.uint64)
    buf[:, :rows.shape[1]] = rows
    t = torch.from_numpy(buf.view(np.int64)).cuda()
    return t, t[:, :rows.shape[1]]


def same_bytes(got, ref):
    assert len(got) == len(ref), (len(got), len(ref))
    assert got.dtype == ref.dtype and got.dtype.itemsize == 48
    if got.tobytes() != ref.tobytes():
        bad = [i for i in range(len(ref)) if got[i:i + 1].tobytes() != ref[i:i + 1].tobytes()]
        raise AssertionError("records %s differ: device %s, host %s" % (bad[:4], got[bad[:4]], ref[bad[:4]]))


# ---- 1. synthetic rows ------------------------------------------------------------------------------------------------------------
def test_the_cases_contain_what_they_are_for():
    """conditions on the inputs, asked of the host function alone: every case has at least 3 intervals; over the file an interval
    is closed by a row of zero frames, one by the end of the rows, one is dropped for min_slots (min_slots = 1 returns more) and
    one peaks at +inf; and every shape has the channels it is there for"""
    from p25rx_amd import Scanner
    seen = dict(zero_frame=0, end=0, dropped=0, inf=0, huge=0)
    for name in sorted(CASES):
        N, fs, rows, kw, slot0, _pad = case(name)
        keys = host_keys(name)
        assert len(keys) >= 3, (name, len(keys))
        ends = (keys["first_slot"] + keys["n_slots"] - np.uint64(slot0)).astype(np.int64)
        seen["end"] += int((ends == rows.shape[0]).sum())
        seen["zero_frame"] += int(sum(e < rows.shape[0] and rows[e, N] == 0 for e in ends))
        seen["inf"] += int(np.isposinf(keys["peak_db_over_floor"]).sum())
        seen["dropped"] += len(Scanner.keys(rows, fs, slot0=slot0, **dict(kw, min_slots=1))) - len(keys)
        seen["huge"] += int((rows[:, :N] >= 1 << 63).any())
        assert (keys["first_slot"] >= slot0).all() and int(rows[:, :N].min()) >= 0
    print(seen)
    assert all(v >= 1 for v in seen.values()), seen
    for shape, (N, fs, raster) in SHAPES.items():
        assert len(channels_of(N, fs, raster)[0]) == CHANNELS[shape]


@pytest.mark.parametrize("name", sorted(CASES))
def test_synthetic_rows(rig, name):
    """the bytes of the device form equal the host function's, and the rows -- padding included -- are unchanged"""
    import torch
    N, fs, rows, kw, slot0, pad = case(name)
    ref = host_keys(name)
    buf, view = to_device(rows, pad)
    before = buf.clone()
    kp = rig.scanner(N).keys_plan(fs, max_rows=rows.shape[0], max_keys=max(len(ref), 1), **kw)
    kp.run_dev(view, slot0=slot0)
    got = kp.read()
    assert torch.equal(buf, before)
    same_bytes(got, ref)
    short, count = kp.read(cap=2)                                    # p25fe_waterfall_keys' contract for a short array
    assert count == len(ref)
    same_bytes(short, ref[:2])
    kp.close()


def test_thresholds_that_are_not_numbers(rig):
    """on_db = off_db = 4000: 10^400 is +inf, and over a floor of zero the threshold is 0 * inf = NaN.  `>=` fails on the device
    as it does on the host: no key from either, where a comparison turned round would have opened every channel of row 1"""
    N, fs, rows, kw, _slot0, _pad = case("c199_65")
    kw = dict(kw, on_db=4000.0, off_db=4000.0, min_slots=1)
    assert len(rig.Scanner.keys(rows, fs, **kw)) == 0
    kp = rig.scanner(N).keys_plan(fs, max_rows=65, max_keys=8, **kw)
    kp.run_dev(to_device(rows)[1])
    assert len(kp.read()) == 0


# ---- 2. overflow --------------------------------------------------------------------------------------------------------------------
def test_more_intervals_than_max_keys(rig):
    """max_keys below the count: read raises P25FE_ERR_CAPACITY carrying the host's count, and goes on doing so"""
    N, fs, rows, kw, slot0, _pad = case("c199_300")
    ref = host_keys("c199_300")
    assert len(ref) > 4
    kp = rig.scanner(N).keys_plan(fs, max_rows=300, max_keys=len(ref) - 1, **kw)
    kp.run_dev(to_device(rows)[1], slot0=slot0)
    for _ in range(2):
        with pytest.raises(rig.lib.P25feError) as e:
            kp.read()
        assert e.value.status == rig.lib.ERR_CAPACITY and e.value.count == len(ref)
    out = np.zeros(len(ref) + 2, dtype=rig.lib.WATERFALL_KEY_DTYPE)
    out["reserved"] = -99
    n = C.c_size_t(0)
    assert kp.lib.p25fe_keys_read(kp.kp, out.ctypes.data_as(C.c_void_p), len(out), C.byref(n)) == rig.lib.ERR_CAPACITY
    assert n.value == len(ref) and (out["reserved"] == -99).all()    # nothing written


# ---- 3. re-use -------------------------------------------------------------------------------------------------------------------------
def test_one_object_run_twice(rig):
    """300 rows, then 7 different ones, then none: every result is its own rows' alone; before any run there is no key"""
    N, fs, rows, kw, _slot0, _pad = case("c199_300")
    N2, fs2, rows2, kw2, _s, _p = case("c199_7")
    assert (N, fs, kw) == (N2, fs2, kw2) and not np.array_equal(rows[:7], rows2)
    kp = rig.scanner(N).keys_plan(fs, max_rows=300, max_keys=256, **kw)
    assert len(kp.read()) == 0
    kp.run_dev(to_device(rows)[1])
    same_bytes(kp.read(), host_keys("c199_300"))
    short = to_device(rows2)[1]
    kp.run_dev(short)
    same_bytes(kp.read(), host_keys("c199_7"))
    same_bytes(kp.read(), host_keys("c199_7"))                       # reading does not consume
    kp.run_dev(short, n_rows=0)
    assert len(kp.read()) == 0


# ---- 4. the keyed scene -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["cf32", "u8"])
def test_the_keyed_scene(rig, fmt):
    """tests/waterfall_model.py's scene: the survey and the keys enqueued on the same stream with nothing between them; the five
    intervals, bytes equal to the host route's"""
    x = WM.keyed_scene()
    raw = x if fmt == "cf32" else SM.to_u8(x)
    sc = rig.scanner(WM.KEY_N, WM.KEY_HOP)
    kp = sc.keys_plan(WM.KEY_FS, max_rows=64, max_keys=16)
    t = dev(raw)
    rows = sc.waterfall_dev(t, WM.KEY_B)
    kp.run_dev(rows)
    got = kp.read()
    ref = rig.Scanner.keys(rows.cpu().numpy().view(np.uint64), WM.KEY_FS)
    assert rows.shape == (51, WM.KEY_N + 1) and len(ref) == 5
    assert [(int(k["raster_index"])) for k in ref] == [r for r, _a, _b, _o in WM.keyed_truth()]
    same_bytes(got, ref)


# ---- 5. the streaming form ---------------------------------------------------------------------------------------------------------------
def test_the_streaming_form(rig):
    """open_waterfall, the scene in uneven pieces, run_stream: equal to read_waterfall followed by the host function -- after the
    first pieces (a part of the rows) and at the end"""
    x = WM.keyed_scene()
    from p25rx_amd import Scanner
    sc = Scanner(rig.fe, WM.KEY_N, WM.KEY_HOP, shift=WM.KEY_SHIFT)
    kp = sc.keys_plan(WM.KEY_FS, max_rows=64, max_keys=16)
    with pytest.raises(rig.lib.P25feError) as e:                     # no open waterfall yet
        kp.run_stream()
    assert e.value.status == rig.lib.ERR_ARG
    sc.open_waterfall(WM.KEY_B, 51)
    kp.run_stream()
    assert len(kp.read()) == 0                                       # no row touched yet
    edges = [0, 1, 4099, 100000, 100007, 333333, 400001, len(x)]
    for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        sc.waterfall(x[a:b])
        if i == 4:
            kp.run_stream()
            part = sc.read_waterfall()
            assert 20 < part.shape[0] < 51
            ref = Scanner.keys(part, WM.KEY_FS)
            assert len(ref) >= 3
            same_bytes(kp.read(), ref)
    kp.run_stream()
    rows = sc.read_waterfall()
    ref = Scanner.keys(rows, WM.KEY_FS)
    assert rows.shape == (51, WM.KEY_N + 1) and len(ref) == 5
    same_bytes(kp.read(), ref)
    kp.close()
    sc.close()


# ---- 6. refusals that need an object -------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(rig):
    """n_rows > max_rows is P25FE_ERR_CAPACITY; a misaligned pointer, a short stride and run_stream without an open waterfall are
    P25FE_ERR_ARG.  Nothing is enqueued: the result of the run before them is still there afterwards (a refused run that had got
    as far as its memset would have emptied it)"""
    N, fs, rows, kw, _slot0, _pad = case("c19_65")
    ref = host_keys("c19_65")
    sc = rig.Scanner(rig.fe, N)
    kp = sc.keys_plan(fs, max_rows=65, max_keys=64, **kw)
    t = to_device(rows)[1]
    more = to_device(np.concatenate([rows, rows[:1]]))[1]
    kp.run_dev(t)
    same_bytes(kp.read(), ref)
    L, ptr, stream = kp.lib, t.data_ptr(), rig.fe._stream()
    with pytest.raises(rig.lib.P25feError) as e:
        kp.run_dev(more)
    assert e.value.status == rig.lib.ERR_CAPACITY
    assert L.p25fe_keys_dev(kp.kp, C.c_void_p(ptr + 4), 65, N + 1, 0, stream) == rig.lib.ERR_ARG
    assert L.p25fe_keys_dev(kp.kp, None, 65, N + 1, 0, stream) == rig.lib.ERR_ARG
    assert L.p25fe_keys_dev(kp.kp, C.c_void_p(ptr), 65, N, 0, stream) == rig.lib.ERR_ARG
    assert L.p25fe_keys_stream(kp.kp) == rig.lib.ERR_ARG
    same_bytes(kp.read(), ref)
    # create's limits of the device form, which need the object's N: 3999 channels at 6.25 kHz pass, 4799 do not; scratch
    for fs_hz, raster, max_rows, status in ((25000000, 6250.0, 16, None), (30000000, 6250.0, 16, rig.lib.ERR_CAPACITY),
                                            (20000000, 6250.0, 1 << 17, rig.lib.ERR_CAPACITY)):
        big = rig.scanner(4096)
        if status is None:
            big.keys_plan(fs_hz, raster_hz=raster, max_rows=max_rows, max_keys=4).close()
        else:
            with pytest.raises(rig.lib.P25feError) as e:
                big.keys_plan(fs_hz, raster_hz=raster, max_rows=max_rows, max_keys=4)
            assert e.value.status == status, (fs_hz, max_rows)
    kp.close()
    sc.close()
