"""Frame sequences on the GPU (tests/frame_sequence_cases.py): what csharp/Softbody.cs does every FixedUpdate -- several between-tick calls
back to back, a step, a readback, queries -- on a SoftbodyGroup, every observation compared with the reference driver's under the rule of
its kind: positions, velocities, snapshot arrays, boxes and hits bitwise, body-state and reaction sums within their derived bounds with
exact counts, refusals by their status, and sb_stats' ticks_fused / ticks_fused_kinematic / readback_peeks after every step against the
counter model. tests/test_frame_sequences.py asserts on the CPU that the fixed slice covers what it claims to.

a. one rank: the fixed slice, in chunks -- 25 of the first block, 10 of the second (the signed-distance calls, SPEC.md 2i)        b. 2 and 4 ranks, both host models, whole meshes and windows (tests/frame_group_case.py)
c. twins: reactions fetched at once and after the next tick -- the same bits throughout, ticks_fused as the model predicts for each"""
import functools
import os
import subprocess
import sys
import time

import pytest

import frame_sequence_cases as fc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _reference(seed, twin=False):
    """the reference's observations of a scenario of the slice: computed once, shared by the tests below, never written to"""
    from oracle import oracle
    oracle.build()
    sc = fc.make_scenario(seed)
    if twin:
        sc = fc.defer_fetches(sc)
    return sc, fc.run_reference(oracle, sc)


def _run(sc):
    g = fc.open_group(sc)
    try:
        if sc["body"] == "cube16":
            assert fc.coded_format_in_force(g), ("the coded format is not in force", g.rank(0).stats()["launch_bytes"])
        assert g.rank(0).stats()["n_tilings"] == 2, "the counter model takes the body for tiled"
        return fc.run_group(g, sc)
    finally:
        g.OnDestroy()


def _check(seed, twin=False):
    sc, want = _reference(seed, twin)
    got = _run(sc)
    bad = fc.first_mismatch(want, got)
    assert bad is None, fc.report(sc, want, got, *bad, command=f"python tests/fuzz/fuzz_frames.py --only {seed}")
    return want, got


# ---- a. one rank ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", range(len(fc.chunks())))
def test_one_rank_walks_the_fixed_slice_like_the_reference(chunk):
    t0 = time.perf_counter()
    for seed in fc.chunks()[chunk]:
        _check(seed)
    print(f"chunk {chunk}: seeds {fc.chunks()[chunk][0]} .. {fc.chunks()[chunk][-1]} in {time.perf_counter() - t0:.1f} s")


# ---- c. the fetch rule: twins --------------------------------------------------------------------------------------------------------------------

def _twin_seeds():
    """scenarios of the slice that fetch reactions right behind the call, a tick following: their twins fetch behind that tick"""
    out = []
    for seed in fc.FIRST_BLOCK:
        names = [n for n, _ in fc.make_scenario(seed)["script"]]
        at = [k for k, n in enumerate(names) if n == "collider_reactions" and names[k - 1] == "collide_with_reactions"]
        if at and "step" in names[at[0]:]:
            out.append(seed)
    return out[::max(1, len(out) // 8)][:8]


def test_reactions_fetched_at_once_or_after_the_next_tick_leave_the_same_bits_and_the_predicted_fusion():
    seeds = _twin_seeds()
    assert len(seeds) >= 6
    for seed in seeds:
        want_now, got_now = _check(seed)
        want_late, got_late = _check(seed, twin=True)
        state = lambda obs: [o for o in obs if o[0] in ("bits", "ray", "closest")]       # noqa: E731
        a, b = state(got_now), state(got_late)
        assert len(a) == len(b) > 0
        for p, q in zip(a, b):
            assert p[1].split()[2:] == q[1].split()[2:] and fc.mismatch(p, (p[0], p[1], q[2])) is None, f"seed {seed}: the twins differ at '{p[1]}' / '{q[1]}'"
        # ticks_fused of each twin is what the model predicts for its script; the fetch waits for the call's own event and completes
        # nothing, so the prediction is the same number for both
        predicted = want_late[-1][2][0] - want_now[-1][2][0]
        assert got_late[-1][2][0] - got_now[-1][2][0] == predicted == 0, (seed, got_now[-1][2], got_late[-1][2])
        records = lambda obs: [o[2][0].tobytes() for o in obs if o[0] == "react"]       # noqa: E731
        assert records(got_now) == records(got_late), f"seed {seed}: the records fetched late are not the records fetched at once"


# ---- b. several ranks ----------------------------------------------------------------------------------------------------------------------------

_GROUP_CASE_ENDED_ABNORMALLY = []


@pytest.mark.parametrize("ranks", [2, 4])
@pytest.mark.parametrize("host", ["threads", "walk"])
def test_a_group_of_several_ranks_walks_the_scripts_like_the_reference(host, ranks):
    # ranks of one process on one device, as tests/test_gpu_group.py runs them: a hardware queue per rank for the peer transport.
    # One subprocess under a timeout. 0 and 1 are the case's own exits (OK / MISMATCH); after any other exit or a timeout the cases
    # behind it are not started here.
    assert not _GROUP_CASE_ENDED_ABNORMALLY, f"not started: the case before ended abnormally ({_GROUP_CASE_ENDED_ABNORMALLY[0]})"
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16")
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "frame_group_case.py"), host, str(ranks)], env=env, capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired:
        _GROUP_CASE_ENDED_ABNORMALLY.append(f"{host} x {ranks}: timeout")
        raise
    if out.returncode not in (0, 1):
        _GROUP_CASE_ENDED_ABNORMALLY.append(f"{host} x {ranks}: exit {out.returncode}")
    print(out.stdout[-1500:])
    assert out.returncode == 0 and "FRAME GROUP OK" in out.stdout, out.stdout[-4000:] + out.stderr[-3000:]
