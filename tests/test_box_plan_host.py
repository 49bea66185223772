"""csrc/box_plan.cpp against the plans recorded before the planning code moved there (tests/golden/box_plan_candidates.json, made by
tests/golden/make_box_plan_fixture.py): host only.

For every box of the fixture the candidate lists of the double sweep, the plane-marching kernel and the plane-marching kernel with
room for 64 partial sums must equal the recorded ones entry for entry, in order -- the first entry is the planner's plan, the marching
kernel's second its shared-CU plan, so the planner is pinned for both kernels and both shared-CU settings.  Checked twice: through
tests/cpp/box_plan_check.cpp, built from box_plan.cpp alone with plain g++ under the address and undefined-behaviour sanitizers (it
also fails if box_plan_refusal rejects a plan it lists), and through the library's C ABI.
"""
import json
import os
import subprocess

import pytest

import sparsh_amg_amd as sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LISTS = (("double", 2, 0), ("marching", 1, 0), ("marching_capped", 1, None))  # (fixture key, kernel, part_cap; None: the fixture's)


@pytest.fixture(scope="session")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "box_plan_candidates.json")) as f:
        doc = json.load(f)
    assert doc["plan"] == ["threads", "q", "ty", "cz"] and len(doc["cases"]) >= 100
    return doc


def _queries(doc):
    """(kernel, box, part_cap, recorded list) for every list of the fixture."""
    return [(kernel, tuple(case["box"]), doc["part_cap"] if cap is None else cap, [tuple(p) for p in case[key]])
            for case in doc["cases"] for key, kernel, cap in LISTS]


@pytest.fixture(scope="session")
def box_plan_check(tmp_path_factory):
    d = tmp_path_factory.getbasetemp() / "boxplan"
    d.mkdir(exist_ok=True)
    exe = d / "box_plan_check"
    if not exe.exists():
        csrc = os.path.join(ROOT, "sparsh_amg_amd", "csrc")
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-I{csrc}",
               os.path.join(ROOT, "tests", "cpp", "box_plan_check.cpp"), os.path.join(csrc, "box_plan.cpp"), "-o", str(exe)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    return str(exe)


def test_host_program_lists_the_recorded_plans(recorded, box_plan_check):
    queries = _queries(recorded)
    text = "".join(f"{kernel} {box[0]} {box[1]} {box[2]} {cap}\n" for kernel, box, cap, _ in queries)
    r = subprocess.run([box_plan_check], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.split("\n")
    assert lines[-1] == "" and len(lines) == len(queries) + 1
    for (kernel, box, cap, want), line in zip(queries, lines):
        got = [tuple(int(t) for t in p.split()) for p in line.split(";")] if line else []
        assert got == want, (kernel, box, cap)


def test_library_lists_the_recorded_plans(recorded):
    for kernel, box, cap, want in _queries(recorded):
        assert sa.box_plan_candidates(kernel, *box, part_cap=cap) == want, (kernel, box, cap)
