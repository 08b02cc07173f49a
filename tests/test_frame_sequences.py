"""The fixed slice of tests/frame_sequence_cases.py, walked by the reference driver alone: the conditions that keep
tests/test_gpu_frame_sequences.py honest are asserted here, without a GPU -- the pair matrix, the planted (call x left state) and
(call x tick shape) combinations, how often every step occurs, that contacts and forces actually do something, that every state stays
finite and moving, that planted refusals are refusals, that a printed script replays, and the counter model on hand-written scripts.

Measured here (one x86 core): the reference driver takes 4.1 s for the 200 scenarios of the slice, 0.02 s per scenario on average and
0.16 s for the slowest (seed 194: a 16^3 cube with surface forces, whose reference is a Python loop over 2 700 triangles); building the
four bodies once costs about 1 s. A chunk of frame_sequence_cases.CHUNK = 8 scenarios therefore costs the GPU module about 0.2 s of
reference, 1.3 s at the very worst, and less than that on the GPU side."""
import collections
import time

import numpy as np
import pytest

import frame_sequence_cases as fc
from frame_sequence_cases import LEFT_STATES, STATE_CHANGING, TICK_SHAPES, TickModel


@pytest.fixture(scope="module")
def slice_(oracle_mod):
    """every scenario of the fixed slice with the reference's observations and what the driver noted about it; computed once"""
    assert fc.constants_match()
    out, seconds = [], []
    for seed in fc.FIXED_SLICE:
        sc = fc.make_scenario(seed)
        info = {}
        t0 = time.perf_counter()
        obs = fc.run_reference(oracle_mod, sc, info=info)
        seconds.append(time.perf_counter() - t0)
        out.append((sc, obs, info))
    print(f"reference: {sum(seconds):.1f} s for {len(out)} scenarios, mean {np.mean(seconds):.3f} s, slowest {max(seconds):.2f} s (seed {int(np.argmax(seconds))})")
    return out


def _features(sc):
    """what a script holds beyond its step names: the variants the issue lists"""
    f = collections.Counter()
    script = sc["script"]
    pending, fetched_since_call, ticks_since_call = [], True, 0
    for k, (name, a) in enumerate(script):
        f[name] += 1
        f[fc.coverage_name(name, a)] += 1 if fc.coverage_name(name, a) != name else 0
        prev = script[k - 1][0] if k else None
        if name == "set_kinematic_positions" and prev == "set_kinematic_positions":
            f["kinematic move twice"] += 1
        if name == "set_heightfield" and fc.coverage_name(prev, script[k - 1][1]) in STATE_CHANGING:
            f["heightfield set right behind a call"] += 1
        if name == "apply_impulses":
            for it in a["items"]:
                f["impulse item " + it[0]] += 1
        if name == "place":
            f["place " + ("mirror" if a["mirror"] is not None else "from_reference" if a["from_reference"] else "keep_pinned" if a["keep_pinned"] else "rigid")] += 1
        if name == "step":
            pending = [t + 1 for t in pending]
            ticks_since_call += 1
        if name == "readback_begin":
            pending.append(0)
            if len(pending) == 2:
                f["two snapshots pending"] += 1
        if name == "readback_end":
            f[f"snapshot ended {min(pending.pop(0), 2)} ticks later"] += 1
        if name == "collide_with_reactions":
            fetched_since_call, ticks_since_call = False, 0
        if name == "collider_reactions":
            f["reactions fetched " + ("again" if fetched_since_call else "at once" if ticks_since_call == 0 else "after the next tick")] += 1
            if a["twice"]:
                f["reactions fetched twice"] += 1
            fetched_since_call = True
    return f


def test_the_slice_is_what_the_gpu_module_runs():
    assert len(fc.FIXED_SLICE) == fc.N_PAIRS + fc.N_PLANTED + fc.N_RANDOM == 200
    assert [s for c in fc.chunks() for s in c] == list(fc.FIXED_SLICE) and all(len(c) <= fc.CHUNK for c in fc.chunks())


def test_a_scenario_is_a_pure_function_of_its_seed_and_prints_as_text():
    for seed in (0, 57, 123, 150, 199, 12345):
        a, b = fc.make_scenario(seed), fc.make_scenario(seed)
        assert a == b and fc.loads(fc.dumps(a)) == a
        assert all(isinstance(step, list) and isinstance(step[0], str) and isinstance(step[1], dict) for step in a["script"])


def test_every_ordered_pair_of_state_changing_calls_stands_back_to_back(slice_):
    seen = set()
    for sc, _, _ in slice_:
        names = [fc.coverage_name(n, a) for n, a in sc["script"]]
        seen |= {(p, q) for p, q in zip(names, names[1:]) if p in STATE_CHANGING and q in STATE_CHANGING}
    missing = [(p, q) for p in STATE_CHANGING for q in STATE_CHANGING if (p, q) not in seen]
    print(f"pair matrix: {len(STATE_CHANGING) ** 2 - len(missing)} of {len(STATE_CHANGING) ** 2} ordered pairs")
    assert not missing, missing
    # ... and scenario k of the slice is the one that plants pair k
    for k in range(fc.N_PAIRS):
        sc = slice_[k][0]
        A, B = STATE_CHANGING[k // len(STATE_CHANGING)], STATE_CHANGING[k % len(STATE_CHANGING)]
        names = [fc.coverage_name(n, a) for n, a in sc["script"]]
        assert (A, B) in set(zip(names, names[1:])), (k, A, B)


def test_every_call_meets_every_left_state_and_every_tick_shape(slice_):
    left, shape = set(), set()
    for _, _, info in slice_:
        left |= set(info["call_left"]); shape |= set(info["call_shape"])
    missing = [(c, s) for c in STATE_CHANGING for s in LEFT_STATES if (c, s) not in left] + [(c, s) for c in STATE_CHANGING for s in TICK_SHAPES if (c, s) not in shape]
    assert not missing, missing


def test_every_step_occurs_often_enough(slice_):
    total = collections.Counter()
    for sc, _, _ in slice_:
        total += _features(sc)
    print("steps of the slice: " + ", ".join(f"{k} {v}" for k, v in sorted(total.items())))
    names = ["step", "apply_impulses", "impulse_surface", "impulses", "place", "apply_surface_forces", "collide", "collide_with_reactions", "collide_heightfield",
             "set_state", "get_velocities", "body_motion", "body_pose", "set_kinematic_positions", "kinematic move twice", "set_heightfield",
             "heightfield set right behind a call", "clear_heightfield", "get_positions", "get_bounds", "readback_begin", "readback_end", "raycast", "closest_points",
             "collider_reactions", "reactions fetched at once", "reactions fetched after the next tick", "reactions fetched twice", "two snapshots pending",
             "snapshot ended 0 ticks later", "snapshot ended 1 ticks later", "snapshot ended 2 ticks later", "impulse item P", "impulse item R", "impulse item S",
             "place rigid", "place mirror", "place from_reference", "place keep_pinned", "refuse"]
    few = {k: total[k] for k in names if total[k] < 10}
    assert not few, few
    assert total["refuse"] == len(slice_), "one refusal per scenario"
    axes = collections.Counter()
    for sc, _, _ in slice_:
        axes[sc["body"]] += 1; axes[sc["mode"]] += 1
        for k in ("peek0", "graph", "uvs", "every_tick"):
            axes[f"{k}={sc[k]}"] += 1
    print("axes: " + ", ".join(f"{k} {v}" for k, v in sorted(axes.items())))
    assert all(axes[k] >= 20 for k in list(fc.BODIES) + ["full", "render_set", "embedding"] + [f"{k}={v}" for k in ("peek0", "graph", "uvs", "every_tick") for v in (True, False)]), axes
    lattice = axes["cube16"] + axes["cube10"]
    assert 0.2 * lattice <= axes["embedding"] <= 0.5 * lattice, "about one lattice configuration in three has an embedding in force"


def test_contacts_hit_and_forces_move_something(slice_):
    with_contacts = [info for sc, _, info in slice_ if any(n in ("collide", "collide_with_reactions", "collide_heightfield") for n, _ in sc["script"])]
    hit = sum(1 for info in with_contacts if any(h > 0 for h in info["contact_hits"]))
    with_forces = [info for sc, _, info in slice_ if any(n in ("apply_surface_forces", "apply_impulses") for n, _ in sc["script"])]
    moved = sum(1 for info in with_forces if any(info["velocity_changed"]))
    print(f"contacts: a non-empty hit mask in {hit} of {len(with_contacts)} scenarios; forces: velocities changed in {moved} of {len(with_forces)}")
    assert len(with_contacts) >= 60 and 2 * hit >= len(with_contacts)
    assert len(with_forces) >= 60 and 2 * moved >= len(with_forces)


def test_every_final_state_is_finite_and_moving(slice_):
    for sc, obs, info in slice_:
        x, v = info["final"]
        assert np.isfinite(x).all() and np.isfinite(v).all(), sc["seed"]
        assert np.abs(v).max() > 0.05, sc["seed"]
        for kind, lab, payload in obs:      # nothing is excluded from a comparison
            if kind == "bits":
                assert np.isfinite(payload).all(), (sc["seed"], lab)


def test_every_planted_refusal_is_one_the_reference_refuses(slice_):
    kinds = collections.Counter()
    for sc, obs, info in slice_:
        assert len(info["refusals"]) == 1, sc["seed"]
        what, status = info["refusals"][0]
        assert status is not None and status < 0, (sc["seed"], what)
        kinds[what] += 1
        # ... and it changes no counter: the observation behind it repeats the one before it
        k = [i for i, o in enumerate(obs) if o[0] == "status"][0]
        before = [o for o in obs[:k] if o[0] == "counters"]
        assert obs[k + 1][0] == "counters" and (not before or obs[k + 1][2] == before[-1][2]), sc["seed"]
    print("refusals: " + ", ".join(f"{k} {v}" for k, v in sorted(kinds.items())))
    assert len(kinds) >= 5 and min(kinds.values()) >= 5


def test_replaying_a_printed_script_gives_the_same_observations(slice_, oracle_mod):
    for k in (3, 36, 64, 117, 150, 199):
        sc, obs, _ = slice_[k]
        again = fc.run_reference(oracle_mod, fc.loads(fc.dumps(sc)))
        assert fc.first_mismatch(_as_group(obs), _as_group(again)) is None, sc["seed"]


def _as_group(obs):
    """reference observations in the shape run_group returns them, so that the rules can compare two reference runs: body and react carry the
    reference's own records, which the rules cannot take as `got` -- those two kinds are compared by their numbers instead"""
    out = []
    for kind, lab, p in obs:
        if kind == "body":
            out.append(("bits", lab, np.asarray(p[1]["sums"], np.float64).astype(np.float32)))
        elif kind == "react":
            out.append(("bits", lab, np.concatenate([np.asarray(r["sums"], np.float64) for r in p]).astype(np.float32)))
        else:
            out.append((kind, lab, p))
    return out


def test_replay_helper_compares_like_with_like(slice_):
    sc, obs, _ = slice_[150]
    a = _as_group(obs)
    assert fc.first_mismatch(a, a) is None
    b = list(a)
    k = [i for i, o in enumerate(b) if o[0] == "bits"][-1]
    bad = np.array(b[k][2], copy=True); bad.view(np.uint32).reshape(-1)[0] ^= 1
    b[k] = (b[k][0], b[k][1], bad)
    assert fc.first_mismatch(a, b)[0] == k, "one flipped bit in one observation is found, at its index"


# ---- the counter model on hand-written scripts (include/softbody.h: sb_step, sb_set_kinematic_positions, sb_apply_impulses, sb_get_bounds) ------

def _walk(model, script):
    for name, *a in script:
        getattr(model, name)(*a)
    return model.counters()


def test_counter_model_plain_ticks_fuse_from_the_second_on():
    assert _walk(TickModel(peeking=False), [("step", 0.02, 6)] * 5) == (4, 0, 0)


def test_counter_model_a_state_changing_call_costs_the_next_tick_its_fusion_once():
    s = ("step", 0.02, 6)
    assert _walk(TickModel(peeking=False), [s, s, ("complete",), s, s, s]) == (3, 0, 0)       # 1 + 0 + 1 + 1


def test_counter_model_tick_shapes():
    s = ("step", 0.02, 6)
    assert _walk(TickModel(peeking=False), [s, s, ("step", 0.02, 4), ("step", 0.02, 4)]) == (2, 0, 0), "another even S starts unfused, then fuses"
    assert _walk(TickModel(peeking=False), [s, s, ("step", 0.01, 6), ("step", 0.01, 6)]) == (2, 0, 0), "another dt likewise"
    assert _walk(TickModel(peeking=False), [s, s, ("step", 0.02, 3), ("step", 0.02, 3), s, s]) == (2, 0, 0), "an odd S under a tiling holds nothing back"
    assert _walk(TickModel(peeking=False, tiled=False), [("step", 0.02, 3)] * 3) == (2, 0, 0), "... without a tiling it does"


def test_counter_model_reads_peek_where_peeking_is_on_and_complete_elsewhere():
    s = ("step", 0.02, 6)
    read = ("read_positions",)
    assert _walk(TickModel(peeking=True), [s, read, s, read, read, s]) == (2, 0, 3)
    assert _walk(TickModel(peeking=False), [s, read, s, read, read, s]) == (0, 0, 0)
    assert _walk(TickModel(peeking=True), [("step", 0.02, 3), read, ("step", 0.02, 3)]) == (0, 0, 0), "nothing held back: nothing to peek"
    assert _walk(TickModel(peeking=True), [s, ("complete",), read, s]) == (0, 0, 0)


def test_counter_model_kinematic_moves():
    s = ("step", 0.02, 6)
    k = ("kinematic",)
    assert _walk(TickModel(peeking=False), [s, k, s, k, s]) == (2, 2, 0), "a move every tick rides the fused kernel"
    assert _walk(TickModel(peeking=False), [s, k, k, s, s]) == (1, 0, 0), "a second move completes the tick: the earlier one takes effect first"
    assert _walk(TickModel(peeking=True), [s, k, ("read_positions",), s]) == (1, 1, 1), "a peek shows the move and leaves it pending"
    assert _walk(TickModel(peeking=False), [s, k, ("read_positions",), s, s]) == (1, 0, 0), "a read that completes the tick lands it"
    assert _walk(TickModel(peeking=False), [s, k, ("complete",), s, s]) == (1, 0, 0)
    assert _walk(TickModel(peeking=False), [s, k, ("step", 0.01, 6), ("step", 0.01, 6)]) == (1, 0, 0), "an unfused tick lands it at its start"


def test_counter_model_calls_that_touch_nothing(oracle_mod):
    s = ("step", 0.02, 6)
    assert _walk(TickModel(peeking=False), [s, ("nothing",), s]) == (1, 0, 0), "set_heightfield, queries, a reactions fetch, a refusal"
    # in the driver: a heightfield call with no table set completes nothing (softbody_group.h)
    sc = dict(fc.make_scenario(0))
    step = ["step", {"dt": 0.02, "S": 6}]
    sc["script"] = [step, ["collide_heightfield", {"friction": 0.1, "restitution": 0.0}], step,
                    ["set_heightfield", {"lo": [0, 0, 0], "hi": [15, 15, 15], "scale": 1.0, "lift": 0.0}], step, ["collide_heightfield", {"friction": 0.1, "restitution": 0.0}], step,
                    ["clear_heightfield", {}], ["collide_heightfield", {"friction": 0.1, "restitution": 0.0}], step]
    obs = fc.run_reference(oracle_mod, sc)
    assert obs[-1][2] == (3, 0, 0), obs[-1]
