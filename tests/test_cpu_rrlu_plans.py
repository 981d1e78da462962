"""The shapes the rrLU planners select are the shapes the launchers instantiate (tensor4all-rs_amd/csrc/rrlu_shapes.hpp).

tests/rrlu_plan_sweep.hip calls rrlu_reg_make_plan for every 1 <= M <= 4224, 1 <= N <= 2176 at 256, 64 and 16 compute units and
rrlu_wg_make_plan for every 1 <= M <= 160, 1 <= N <= 640.  A table entry nobody selects is a kernel compiled for nothing; a
selected shape outside the table would be refused by the launcher (T4A_GPU_INTERNAL_ERROR)."""
from rrlu_plan_sweep import sweep


def test_register_kernel_table_is_what_the_planner_selects_at_256_compute_units():
    s = sweep()
    assert len(s["reg_table"]) > 0
    assert set(s["reg"][256]) == s["reg_table"]


def test_register_kernel_shapes_at_fewer_compute_units_are_in_the_table():
    s = sweep()
    for cus in (64, 16):
        assert len(s["reg"][cus]) > 0
        assert set(s["reg"][cus]) <= s["reg_table"], cus


def test_multi_workgroup_shapes_are_wave_uniform_from_three_columns_up():
    multi = [k for k in sweep()["reg_table"] if not k[2]]
    assert multi and all(uni and cpt >= 3 for (_, cpt, _, uni) in multi)


def test_one_workgroup_kernel_table_is_what_the_planner_selects():
    s = sweep()
    assert set(s["wg"]) == s["wg_table"] == {(1, 8), (1, 16), (2, 8)}
