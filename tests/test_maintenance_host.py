"""The plans that tests/test_maintenance_gpu.py walks (maintenance_cases.py), without a device: every step of a plan replaces
its buffer with a larger one under the restatement of grown() -- which is itself held against csrc/grown.h -- and the small
batches of the child hold every status an all-zero answer would get wrong."""
import os
import re
import subprocess

import maintenance_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jubjub_schnorr_amd", "csrc")


def test_grown_is_the_engines(tmp_path):
    """The Python grown() against csrc/grown.h compiled as it stands (plain C++), around every step from 4 KiB to 1 GiB."""
    wants = sorted({max(1, s + d) for k in range(12, 31) for s in (1 << k, 3 << (k - 1)) for d in (-1, 0, 1)} | {0, 1, 4095})
    src = tmp_path / "grown_check.cpp"
    src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "grown.h"\n'
                   'int main(int c, char** v) { for (int i = 1; i < c; ++i) printf("%zu\\n", jjs::grown(strtoull(v[i], 0, 10))); }\n')
    exe = tmp_path / "grown_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + CSRC, "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)] + [str(w) for w in wants], text=True).split()
    assert [int(x) for x in out] == [cases.grown(w) for w in wants]


def test_the_restated_constants_are_the_engines():
    text = open(os.path.join(CSRC, "engine_state.h")).read()
    assert int(re.search(r"#define JJS_LANE_MAX_ITEMS (\d+)", text).group(1)) == cases.LANE_MAX_ITEMS
    assert int(re.search(r"#define JJS_COMBINE_MAX_CALL_ITEMS (\d+)", text).group(1)) == cases.COMBINE_MAX_CALL_ITEMS
    assert int(re.search(r"constexpr int N_HOST_LANES = (\d+);", text).group(1)) == cases.N_HOST_LANES
    assert "grow_only<uint8_t, true> pinned{{size_t(1) << 20}};" in text and cases.LANE_MIN_BYTES == 1 << 20


def test_lane_plan_grows_the_lanes_at_every_step():
    plan = cases.lane_plan()
    sizes = [cases.lane_bytes_after_reserve(*step) for step in plan]
    assert sizes == [3 * cases.MIB // 2, 2 * cases.MIB, 3 * cases.MIB, 4 * cases.MIB, 6 * cases.MIB, 8 * cases.MIB], (plan, sizes)
    assert all(a < b for a, b in zip([cases.LANE_MIN_BYTES] + sizes, sizes))
    assert all(cases.COMBINE_MAX_CALL_ITEMS < n <= cases.LANE_MAX_ITEMS for _, _, n in plan)
    # each step is the next capacity grown() knows: no step is skipped, and one more item than a step's would not fit it
    for (scheme, fmt, n), size in zip(plan, sizes):
        assert cases.grown(cases.lane_layout_total(scheme, fmt, n)) == size
        assert n == cases.LANE_MAX_ITEMS or cases.lane_layout_total(scheme, fmt, n + 1) > size


def test_large_and_resident_plans_grow_at_every_step():
    plan = cases.large_plan()
    sizes = [cases.stage_bytes_after_reserve("single", "affine", n) for n in plan]
    assert plan[-1] == 1 << 20 and len(plan) >= 4
    assert sizes[0] > cases.stage_bytes_after_reserve("single", "affine", cases.LARGE_CALL_ITEMS)      # above what the calls themselves leave
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and all(a < b for a, b in zip(plan, plan[1:]))
    assert cases.LARGE_CALL_ITEMS > cases.LANE_MAX_ITEMS
    resident = cases.resident_plan()
    assert all(a < b for a, b in zip(resident, resident[1:])) and resident[-1] == 1 << 20


def test_small_batches_hold_every_status():
    import maintenance_child as child
    work = child.small_work()
    assert set(work) == set(cases.SMALL_CALL_ITEMS)
    for n in (64, 1024):
        for scheme, arrays, want in work[n]:
            assert len(want) == n and all(len(a) == n for a in arrays) and set(want.tolist()) >= {0, 1, 2}, (scheme, n)
    assert sorted(int(w[0]) for _, _, w in work[1]) == [0, 0, 1, 1, 2, 2]
