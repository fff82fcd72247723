"""Cases of tests/test_maintenance_gpu.py and tests/test_maintenance_host.py: the plans of jjs_reserve calls that the
maintenance thread of maintenance_child.py walks beside live calls, derived from a restatement of the engine's own sizing --
grown() of csrc/grown.h, lane_layout_for and lane_cap_for of csrc/host_lanes.h, the device arena of a large host-buffer call
(csrc/host_calls.h reserve_host_block) -- so that every step of a plan is known to replace a buffer with a larger one.
Plain Python: nothing here touches the device or the library."""
from __future__ import annotations

MIB = 1 << 20
LANE_MIN_BYTES = MIB                 # growth_rule of host_lane::dev and ::pinned (csrc/engine_state.h)
COMBINE_MAX_CALL_ITEMS = 4096        # a larger call has a lane to itself, laid out for exactly its items (lane_cap_for)
LANE_MAX_ITEMS = 16384               # a larger host-buffer call takes the piece-by-piece pipeline (csrc/host_calls.h)
N_HOST_LANES = 8

# bytes per item of every column of a call shape, in ABI order (csrc/jjs_gpu.hip SHAPES)
COLUMN_WIDTHS = {
    ("single", "affine"): (32, 64, 64, 32),
    ("double", "affine"): (32, 64, 64, 64, 64, 32),
    ("single", "ext"): (32, 96, 96, 32),
    ("double", "ext"): (32, 96, 96, 96, 96, 32),
}


def grown(want: int) -> int:
    """csrc/grown.h: the smallest of 2^k, 1.5 * 2^k (from 4 096 up) that holds `want`."""
    cap = 4096
    while cap < want:
        cap <<= 1
    mid = cap // 4 * 3
    return mid if mid >= want else cap


def pad256(x: int) -> int:
    return (x + 255) & ~255


def lane_layout_total(scheme: str, fmt: str, cap: int) -> int:
    """lane_layout_for(...).total: one array per column for `cap` items, then their statuses."""
    return sum(pad256(cap * w) for w in COLUMN_WIDTHS[(scheme, fmt)]) + pad256(cap)


def lane_bytes_after_reserve(scheme: str, fmt: str, n: int) -> int:
    """Bytes of each of a lane's two areas after jjs_reserve(scheme, fmt, n, host_buffers=1), n in (4 096, 16 384]."""
    assert COMBINE_MAX_CALL_ITEMS < n <= LANE_MAX_ITEMS
    return grown(max(LANE_MIN_BYTES, lane_layout_total(scheme, fmt, n)))


def stage_bytes_after_reserve(scheme: str, fmt: str, n: int) -> int:
    """Bytes of the device arena of the large host-buffer calls after jjs_reserve(scheme, fmt, n, host_buffers=1), one device."""
    assert n > LANE_MAX_ITEMS
    return grown(sum(pad256(n * w) for w in COLUMN_WIDTHS[(scheme, fmt)]) + pad256(n))


def lane_plan():
    """(scheme, fmt, n) per step: the lane areas go from 1 MiB through 1.5, 2, 3, 4, 6 and 8 MiB.  Per step the first of the two
    shapes that can reach the size, at the most items that still fit it."""
    plan = []
    size = LANE_MIN_BYTES
    while True:
        size = grown(size + 1)
        step = None
        for shape in (("single", "affine"), ("double", "ext")):
            fits = [n for n in range(COMBINE_MAX_CALL_ITEMS + 1, LANE_MAX_ITEMS + 1) if lane_bytes_after_reserve(*shape, n) == size]
            if fits:
                step = (*shape, fits[-1])
                break
        if step is None:
            return plan
        plan.append(step)


def large_plan():
    """n per step of jjs_reserve("single", "affine", n, host_buffers=1): every grown() step of the device arena from the one a
    call of LARGE_CALL_ITEMS items leaves up to 2^20 items."""
    return [n for k in range(16, 20) for n in (3 << (k - 1), 1 << (k + 1))]


def resident_plan():
    """n per step of jjs_reserve("single", "affine", n, host_buffers=0): small, medium and big slots in turn."""
    return [20000, 40000, 65536, 131072, 262144, 524288, 1 << 20]


LARGE_CALL_ITEMS = 65536             # above the lane limit; its pieces are smaller than the pipeline's chunk (2^18)
SMALL_CALL_ITEMS = (1, 64, 1024)
