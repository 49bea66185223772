"""The launch plans the setup times on a box-grid level (box_plan_candidates, through sparsh_debug_box_plan_candidates): host only.

A plan is (threads per workgroup, points per thread Q, lines per tile TY, planes per chunk CZ).  The refusal rules and the planners are
restated here: every candidate must pass the rules, the first one is the planner's plan on 1024 threads, the list is the same on every
call and short, and a thread count whose Q * threads points cannot hold the smallest region yields nothing.
"""
import pytest

import sparsh_amg_amd as sa

THREADS = (256, 512, 1024)
BOXES = [(216, 216, 216), (108, 216, 216), (108, 108, 54), (54, 108, 54), (27, 54, 54), (40, 36, 45), (27, 50, 33), (4, 80, 60)]
LIMIT = 12  # kBoxCandidates


def _halo(kernel):
    return 4 if kernel == 2 else 2


def _lds_bytes(kernel, nx, ty):
    return (2 if kernel == 2 else 1) * ((ty + _halo(kernel)) * (nx + 1) + 1) * 8


def _refused(kernel, box, plan):
    """box_plan_refusal restated: thread values, Q, TY and CZ ranges, region <= Q * threads points, LDS <= 64 KiB."""
    nx, ny, nz = box
    threads, q, ty, cz = plan
    if threads not in THREADS:
        return "threads"
    if not 2 <= q <= 4:
        return "q"
    if not 1 <= ty <= ny:
        return "ty"
    if not 1 <= cz <= nz:
        return "cz"
    if (ty + _halo(kernel)) * nx > q * threads:
        return "region"
    if _lds_bytes(kernel, nx, ty) > 65536:
        return "lds"
    return None


def _planner(kernel, nx, ny, nz):
    """box_planner restated (1024 threads): the plan with the lowest modelled cost, the first one on ties."""
    best, plan = None, None
    for q in (2, 3, 4):
        ty = min(ny, q * 1024 // nx - _halo(kernel))
        while ty >= 1 and _lds_bytes(kernel, nx, ty) > 65536:
            ty -= 1
        if ty < 1:
            continue
        ytiles = -(-ny // ty)
        for zch in range(1, nz + 1):
            cz = -(-nz // zch)
            w = ytiles * -(-nz // cz)
            steps = cz + (2 if kernel == 2 else 1)
            cost = ((w + 511) // 512) * steps * q * 16 if kernel == 2 and q == 2 and w > 256 else ((w + 255) // 256) * steps * q * 10
            if best is None or cost < best:
                best, plan = cost, (q, ty, cz)
    return plan


@pytest.mark.parametrize("kernel", [2, 1])
@pytest.mark.parametrize("box", BOXES, ids=lambda b: "x".join(map(str, b)))
def test_candidates_pass_the_rules(kernel, box):
    cands = sa.box_plan_candidates(kernel, *box)
    print(kernel, box, cands)
    assert 1 <= len(cands) <= LIMIT
    assert len(set(cands)) == len(cands)
    for plan in cands:
        assert _refused(kernel, box, plan) is None, (kernel, box, plan, _refused(kernel, box, plan))
    assert cands[0] == (1024,) + _planner(kernel, *box)
    assert cands == sa.box_plan_candidates(kernel, *box) == sa.box_plan_candidates({2: "double", 1: "marching"}[kernel], *box)


def test_smaller_workgroups_are_offered_where_they_fit():
    """Lines of 108 and fewer points: both smaller workgroups appear among the double sweep's candidates; lines of 216 points: none
    of them holds the 18-line region of TY = 14 (216 * 18 = 3888 > 4 * 512)."""
    for box in ((108, 108, 54), (54, 108, 54), (27, 54, 54), (40, 36, 45), (27, 50, 33)):
        for kernel in (2, 1):
            assert {p[0] for p in sa.box_plan_candidates(kernel, *box)} >= {256, 512}, (kernel, box)
    c216 = sa.box_plan_candidates(2, 216, 216, 216)
    assert c216[0] == (1024, 4, 14, 14)
    assert not [p for p in c216 if p[0] < 1024 and p[2] == 14]
    assert all((p[2] + 4) * 216 <= p[1] * p[0] for p in c216)


@pytest.mark.parametrize("kernel", [2, 1])
def test_line_too_long_for_a_thread_count(kernel):
    """The smallest region is five lines (double sweep, TY = 1): a line of more than 4 * threads / 5 points leaves a thread count
    without any candidate (the marching kernel's smallest region is three lines: 4 * threads / 3)."""
    lines = _halo(kernel) + 1
    for threads in (256, 512):
        nx = 4 * threads // lines + 1
        cands = sa.box_plan_candidates(kernel, nx, 20, 20)
        assert cands and all(p[0] > threads for p in cands), (threads, nx, cands)
        assert any(p[0] == threads for p in sa.box_plan_candidates(kernel, 4 * threads // lines, 20, 20)), (threads, nx - 1)
    assert sa.box_plan_candidates(kernel, 4 * 1024 // lines + 1, 20, 20) == []  # too long for the planner too


def test_marching_candidates_fit_the_partial_buffers():
    """One partial per marching workgroup: with room for fewer than the largest candidate launches, none launches more; the double
    sweep ignores the bound."""
    box = (27, 54, 54)

    def wgs(p):
        return -(-box[1] // p[2]) * -(-box[2] // p[3])

    free = sa.box_plan_candidates(1, *box)
    cap = max(wgs(p) for p in free) - 1
    assert cap >= 1
    capped = sa.box_plan_candidates(1, *box, part_cap=cap)
    assert capped and capped != free and all(wgs(p) <= cap for p in capped)
    assert sa.box_plan_candidates(2, *box, part_cap=cap) == sa.box_plan_candidates(2, *box)
    with pytest.raises(ValueError):
        sa.box_plan_candidates(3, *box)
