"""The premises of tests/test_gpu_resample_shapes.py, on the CPU: what tests/resample_shapes.py's table covers of the launch plans the
shape limits of docs/SPEC.md 3.0b admit.  A shape that alone covers a branch cannot leave the table without one of these failing."""
import resample_model as RM
import tune_cuts_model as CM
from resample_shapes import DESIGNED, MAX_L, MAX_M, MAX_T, MAX_TABLE, SHAPES, outputs_for, plan, shape_ok, size_for

PLANS = {s: plan(*s) for s in SHAPES}


def test_the_table():
    assert len(SHAPES) == len(set(SHAPES)) == 34
    assert all(shape_ok(*s) for s in SHAPES)
    for s in SHAPES:
        assert CM.tile(*s) == PLANS[s][3]                             # one restatement


def test_the_plan_at_the_shapes_the_suite_had():
    """the seven shapes and plans of the other GPU files (fit, gl, R, tile)"""
    had = {(1, 10, 80): (197, 64, 3, 192), (12, 125, 84): (188, 60, 3, 180), (15, 128, 69): (231, 60, 3, 180),
           (2, 25, 100): (156, 64, 2, 128), (24, 25, 9): (1950, 48, 4, 192), (3, 250, 667): (17, 63, 1, 17),
           (3, 125, 334): (41, 63, 1, 41)}
    for s, p in had.items():
        assert plan(*s) == p, s
    assert not set(had) & set(SHAPES)


def test_the_designed_rates_are_the_design_rule():
    rates = (960000, 1024000, 1920000, 2000000, 2880000, 3200000, 4000000, 5000000, 6000000, 8000000, 12000000, 16000000, 30720000)
    assert tuple(RM.design(fs)[:3] for fs in rates) == DESIGNED
    assert plan(1, 4, 32) == (503, 64, 4, 256)                        # 960 ksps: the largest sub-tile
    assert plan(1, 128, 1024)[3] == 8                                 # 30.72 Msps
    for s in ((3, 50, 134), (6, 125, 167), (1, 25, 200)):             # 4, 5 and 6 Msps: one full row of lanes
        fit, gl, R, tile = plan(*s)
        assert fit >= gl and R == 1 and tile == gl, s


def test_every_R_with_a_full_row():
    assert {R for fit, gl, R, tile in PLANS.values() if fit >= gl} == {1, 2, 3, 4}
    assert any(gl == 64 and R == 4 and tile == 256 for fit, gl, R, tile in PLANS.values())
    assert all(tile <= 256 for fit, gl, R, tile in PLANS.values())


def test_every_lane_count():
    assert {gl for fit, gl, R, tile in PLANS.values()} >= {51, 52, 55, 60, 62, 63, 64}
    assert {gl for fit, gl, R, tile in PLANS.values() if fit >= gl and R > 1} >= {51, 55, 62}      # xstep and the idle lanes at work


def test_the_small_tiles():
    small = {tile for fit, gl, R, tile in PLANS.values() if tile < gl}
    assert small >= {1, 2, 4, 8} and all(fit == tile and R == 1 for fit, gl, R, tile in PLANS.values() if tile < gl)


def test_the_tap_loop_paths():
    Ts = [s[2] for s in SHAPES]
    assert {T % 8 for T in Ts} == set(range(8))
    assert {1, 2, 3} <= set(Ts)                                       # T < 4: neither block
    assert {T for T in Ts if 4 <= T < 8} >= {5, 6, 7}                 # the 4-block alone, with 1, 2 and 3 taps behind it
    assert any(T >= 8 and T % 8 == 0 for T in Ts) and 8 in Ts and 15 in Ts
    assert MAX_T in Ts


def test_both_ends_of_the_limits():
    assert any(L == MAX_L for L, M, T in SHAPES) and any(M == MAX_M for L, M, T in SHAPES)
    assert any(L * T == MAX_TABLE for L, M, T in SHAPES) and any(M == L + 1 for L, M, T in SHAPES)
    assert (1, MAX_M, MAX_T) in SHAPES and (MAX_L, MAX_L + 1, MAX_TABLE // MAX_L) in SHAPES


def test_the_sizes():
    """size_for's n owns 9 tile + 3 outputs from position 0 and no sample more than it needs; every phase occurs"""
    total = 0
    for L, M, T in SHAPES:
        n, want = size_for(L, M, T), outputs_for(L, M, T)
        tile = PLANS[(L, M, T)][3]
        assert want == 9 * tile + 3 == RM.n_resample(L, M, 0, n) and RM.n_resample(L, M, 0, n - 1) == want - 1
        assert -(-want // (tile * CM.RS_SUBS)) == 3                  # three workgroups, the last one partial
        assert set(RM.phases(L, M, want).tolist()) == set(range(L)), (L, M, T)
        assert 12 <= want <= 2307 and 2164 <= n <= 21504, (L, M, T, want, n)
        total += n
    assert total == 314609                                            # input samples over the whole table: the file stays small
