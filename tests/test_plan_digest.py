"""The WHOLE plan, tile tables included, pinned on the CPU: tests/sanitize/plan_digest.cpp builds Plan and every rank's LocalPlan
for a fixed corpus and prints one 64-bit digest per case over every field; the digests must equal tests/golden/plan_digests.json,
whatever the number of planner threads.

The golden file is never written from the code under test. A pull request that MEANS to change the plan regenerates it from
its own planner and says so; one that means to leave plans alone (a refactor) generates it from the PARENT commit's planner:

    mkdir /tmp/parent && git show HEAD~1:softbodyunity_amd/csrc/plan.cpp > /tmp/parent/plan.cpp \\
                      && git show HEAD~1:softbodyunity_amd/csrc/plan.hpp > /tmp/parent/plan.hpp
    python tests/test_plan_digest.py --regenerate /tmp/parent

(without a directory: the planner of the working tree). The file in the tree was generated from be3c950, the parent of the commit
that split build_plan into stages.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "softbodyunity_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_digests.json")


def _build(out_dir, planner_dir=CSRC):
    exe = os.path.join(str(out_dir), "plan_digest")
    # the Makefile's flags for plan.cpp
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", "-I", planner_dir, "-I", os.path.join(ROOT, "tests", "sanitize"),
                           os.path.join(ROOT, "tests", "sanitize", "plan_digest.cpp"), os.path.join(planner_dir, "plan.cpp"), "-o", exe])
    return exe


def _digests(exe, threads):
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, SB_PLAN_THREADS=str(threads)), timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    pairs = [line.split() for line in out.stdout.splitlines()]
    assert len({name for name, _ in pairs}) == len(pairs), "duplicate case names"
    return dict(pairs)


def test_every_field_of_every_plan_matches_the_golden_digests(tmp_path):
    exe = _build(tmp_path)
    with open(GOLDEN) as f:
        want = json.load(f)
    assert len(want) >= 50
    for threads in (1, 4):      # (the planner reads SB_PLAN_THREADS once per process)
        got = _digests(exe, threads)
        missing, extra = sorted(set(want) - set(got)), sorted(set(got) - set(want))
        different = sorted(name for name in want if name in got and got[name] != want[name])
        assert not (missing or extra or different), f"SB_PLAN_THREADS={threads}: missing {missing}, extra {extra}, different {different}"


if __name__ == "__main__":
    import tempfile
    assert len(sys.argv) >= 2 and sys.argv[1] == "--regenerate", __doc__
    with tempfile.TemporaryDirectory() as tmp:
        exe = _build(tmp, os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else CSRC)
        digests = _digests(exe, 1)
        assert digests == _digests(exe, 4), "the digests depend on the thread count"
    with open(GOLDEN, "w") as f:
        json.dump(digests, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(digests)} digests to {GOLDEN}")
