#!/usr/bin/env python3
"""Records tests/golden/box_plan_candidates.json: the launch plans (threads, q, ty, cz) that sparsh_amg_amd.box_plan_candidates lists
for the double sweep (kernel 2), the plane-marching kernel (kernel 1) and the plane-marching kernel with room for 64 partial sums:
    python tests/golden/make_box_plan_fixture.py [commit]

The fixture is DATA: lists of integers, recorded with the library built from the commit named in the file, before the planning code
moved into csrc/box_plan.cpp.  A list's first entry is the planner's plan and, for the marching kernel, its second entry the shared-CU
plan where that is another one, so the lists pin down the planner for both kernels and both of its shared-CU settings, the refusal rules
and the pruning.  Run it again only to record a deliberate change of the plans; tests/test_box_plan_host.py compares against it.

Boxes: the eight of tests/test_box_plan_candidates_host.py, and every line length at which a thread count stops holding the smallest
region (5 lines for the double sweep, 3 for the marching kernel) or the 64 KiB of LDS start to bind, with its neighbours, against five
(ny, nz) that clip TY and CZ or do not.
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "box_plan_candidates.json")

BOXES = [(216, 216, 216), (108, 216, 216), (108, 108, 54), (54, 108, 54), (27, 54, 54), (40, 36, 45), (27, 50, 33), (4, 80, 60)]
NX = [2, 3, 5, 27, 54, 108, 204, 205, 216, 341, 342, 409, 410, 682, 683, 818, 819, 820, 1365, 1366]
NYNZ = [(1, 1), (20, 20), (54, 108), (216, 216), (7, 300)]
PART_CAP = 64


def main():
    import sparsh_amg_amd as sa

    commit = sys.argv[1] if len(sys.argv) > 1 else subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    boxes = BOXES + [(nx, ny, nz) for nx in NX for ny, nz in NYNZ]
    cases = []
    for box in boxes:
        cases.append({
            "box": list(box),
            "double": [list(p) for p in sa.box_plan_candidates(2, *box)],
            "marching": [list(p) for p in sa.box_plan_candidates(1, *box)],
            "marching_capped": [list(p) for p in sa.box_plan_candidates(1, *box, part_cap=PART_CAP)],
        })
    doc = {"recorded_from_commit": commit, "plan": ["threads", "q", "ty", "cz"], "part_cap": PART_CAP, "cases": cases}
    with open(OUT, "w") as f:
        f.write("{\n")
        for k in ("recorded_from_commit", "plan", "part_cap"):
            f.write(f' "{k}": {json.dumps(doc[k])},\n')
        f.write(' "cases": [\n')
        f.write(",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in cases))
        f.write("\n ]\n}\n")
    with open(OUT) as f:
        assert json.load(f) == doc
    print(f"wrote {OUT}: {len(cases)} boxes, {sum(len(c[k]) for c in cases for k in ('double', 'marching', 'marching_capped'))} plans, "
          f"{os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
