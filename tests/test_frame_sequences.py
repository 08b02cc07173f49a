"""The fixed slice of tests/frame_sequence_cases.py, walked by the reference driver alone: the conditions that keep
tests/test_gpu_frame_sequences.py honest are asserted here, without a GPU -- the pair matrix, the planted (call x left state) and
(call x tick shape) combinations, how often every step occurs, that contacts and forces actually do something, that every state stays
finite and moving, that planted refusals are refusals, that a printed script replays, and the counter model on hand-written scripts.

Measured here (one x86 core): the reference driver takes 4.1 s for the 200 scenarios of the slice, 0.02 s per scenario on average and
0.16 s for the slowest (seed 194: a 16^3 cube with surface forces, whose reference is a Python loop over 2 700 triangles); building the
four bodies once costs about 1 s. A chunk of frame_sequence_cases.CHUNK = 8 scenarios therefore costs the GPU module about 0.2 s of
reference, 1.3 s at the very worst, and less than that on the GPU side.
The second block (seeds 200 .. 279, the signed-distance calls; tables of 9^3 and 17^3 samples): 3.2 s for its 80 scenarios, 0.04 s on
average and 0.27 s for the slowest (seed 268: the 16^3 cube again, with two surface-force calls -- the Python loop, not its table), 1.7 times the
first block's slowest."""
import collections
import hashlib
import os
import time

import numpy as np
import pytest

import frame_sequence_cases as fc
from frame_sequence_cases import ALL, LEFT_STATES, STATE_CHANGING, TICK_SHAPES, D, TickModel


def _walk_block(oracle_mod, seeds):
    assert fc.constants_match()
    out, seconds = [], []
    for seed in seeds:
        sc = fc.make_scenario(seed)
        info = {}
        t0 = time.perf_counter()
        obs = fc.run_reference(oracle_mod, sc, info=info)
        seconds.append(time.perf_counter() - t0)
        out.append((sc, obs, info))
    print(f"reference: {sum(seconds):.1f} s for {len(out)} scenarios, mean {np.mean(seconds):.3f} s, slowest {max(seconds):.2f} s (seed {seeds[int(np.argmax(seconds))]})")
    return out


@pytest.fixture(scope="module")
def slice_(oracle_mod):
    """every scenario of the first block with the reference's observations and what the driver noted about it; computed once"""
    return _walk_block(oracle_mod, fc.FIRST_BLOCK)


@pytest.fixture(scope="module")
def slice2(oracle_mod):
    """the same of the second block (the signed-distance calls)"""
    return _walk_block(oracle_mod, fc.SECOND_BLOCK)


def _features(sc):
    """what a script holds beyond its step names: the variants the issue lists"""
    f = collections.Counter()
    script = sc["script"]
    pending, fetched_since_call, ticks_since_call = [], True, 0
    full, behind_a_call = {}, False          # signed-distance slot -> samples of its table; whether the step before was a call that completes the tick
    for k, (name, a) in enumerate(script):
        f[name] += 1
        f[fc.coverage_name(name, a)] += 1 if fc.coverage_name(name, a) != name else 0
        prev = script[k - 1][0] if k else None
        if name == "set_kinematic_positions" and prev == "set_kinematic_positions":
            f["kinematic move twice"] += 1
        if name == "set_heightfield" and fc.coverage_name(prev, script[k - 1][1]) in STATE_CHANGING:
            f["heightfield set right behind a call"] += 1
        if name == "set_distance_field":
            count = 27 if a["prop"] == "floor" else a["n"] ** 3
            f[f"slot {a['slot']}"] += 1; f["prop " + a["prop"]] += 1
            if a["slot"] in full:
                f["table replaced, " + ("the same size" if full[a["slot"]] == count else "another size")] += 1
                f["table replaced right behind a call"] += behind_a_call
            full[a["slot"]] = count
        if name == "clear_distance_field":
            f[f"slot {a['slot']}"] += 1
            f["slot cleared right behind a call"] += behind_a_call and a["slot"] in full
            full.pop(a["slot"], None)
        if name == D:
            f[f"slot {a['slot']}"] += 1
            f["collide on a full slot" if a["slot"] in full else "collide on an empty slot"] += 1
            f["a moving pose"] += any(a["lin"]) and any(a["ang"])
        behind_a_call = fc.coverage_name(name, a) in STATE_CHANGING or (name == D and a["slot"] in full)
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
    assert len(fc.FIXED_SLICE) == fc.N_PAIRS + fc.N_PLANTED + fc.N_RANDOM + len(fc.SECOND_BLOCK) == 200 + len(fc.SECOND_BLOCK)
    assert fc.FIXED_SLICE == fc.FIRST_BLOCK + fc.SECOND_BLOCK and len(fc.FIRST_BLOCK) == 200
    assert len(fc.SECOND_BLOCK) == fc.N2_PAIRS + fc.N2_PLANTED + fc.N2_LIFETIMES + fc.N2_RANDOM == 21 + 4 + 7 + 48 and len(fc.chunks()) == 25 + 10
    assert [s for c in fc.chunks() for s in c] == list(fc.FIXED_SLICE) and all(len(c) <= fc.CHUNK for c in fc.chunks())


def test_a_scenario_is_a_pure_function_of_its_seed_and_prints_as_text():
    for seed in (0, 57, 123, 150, 199, 12345, 200, 220, 224, 228, 231, 250):
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
    _finite_and_moving(slice_)


def test_second_block_every_final_state_is_finite_and_moving(slice2):
    _finite_and_moving(slice2)


def _finite_and_moving(block):
    for sc, obs, info in block:
        x, v = info["final"]
        assert np.isfinite(x).all() and np.isfinite(v).all(), sc["seed"]
        assert np.abs(v).max() > 0.05, sc["seed"]
        for kind, lab, payload in obs:      # nothing is excluded from a comparison
            if kind == "bits":
                assert np.isfinite(payload).all(), (sc["seed"], lab)


def _refusals_of(block):
    kinds = collections.Counter()
    for sc, obs, info in block:
        assert len(info["refusals"]) == 1, sc["seed"]
        what, status = info["refusals"][0]
        assert status is not None and status < 0, (sc["seed"], what)
        kinds[what] += 1
        # ... and it changes no counter: the observation behind it repeats the one before it
        k = [i for i, o in enumerate(obs) if o[0] == "status"][0]
        before = [o for o in obs[:k] if o[0] == "counters"]
        assert obs[k + 1][0] == "counters" and (not before or obs[k + 1][2] == before[-1][2]), sc["seed"]
    print("refusals: " + ", ".join(f"{k} {v}" for k, v in sorted(kinds.items())))
    return kinds


def test_every_planted_refusal_is_one_the_reference_refuses(slice_):
    kinds = _refusals_of(slice_)
    assert len(kinds) >= 5 and min(kinds.values()) >= 5


def test_second_block_every_planted_refusal_is_one_the_reference_refuses(slice2):
    kinds = _refusals_of(slice2)      # (one per scenario, a refusal, changing no counter: asserted in there)
    assert kinds["distance_field_slot_4"] >= 5 and kinds["distance_field_restitution"] >= 5, kinds
    for sc, _, _ in slice2:
        for name, a in sc["script"]:
            if name == "refuse" and a["what"] == "distance_field_restitution":
                full = {}
                for n2, a2 in sc["script"][:sc["script"].index([name, a])]:
                    if n2 == "set_distance_field":
                        full[a2["slot"]] = True
                    elif n2 == "clear_distance_field":
                        full.pop(a2["slot"], None)
                assert a["slot"] in full and a["pose"]["restitution"] == 1.5, (sc["seed"], "restitution 1.5 on a FULL slot")


def test_replaying_a_printed_script_gives_the_same_observations(slice_, oracle_mod):
    _replay(slice_, (3, 36, 64, 117, 150, 199), oracle_mod)


def test_second_block_replaying_a_printed_script_gives_the_same_observations(slice2, oracle_mod):
    _replay(slice2, (0, 20, 24, 28, 31, 60), oracle_mod)      # a pair, (D, D), a planted one, two table lifetimes, a random one


def _replay(block, picks, oracle_mod):
    for k in picks:
        sc, obs, _ = block[k]
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


# ---- the second block: the signed-distance calls (SPEC.md 2i) against everything above ------------------------------------------------------------

def test_the_first_block_is_byte_for_byte_what_it_was():
    """tests/golden/frame_slice_v1.sha256.txt: one SHA-256 of dumps(make_scenario(seed)) per line for seeds 0 .. 199, written by the commit
    before the generator learnt the signed-distance steps"""
    with open(os.path.join(fc.ROOT, "tests", "golden", "frame_slice_v1.sha256.txt")) as fh:
        want = fh.read().split()
    assert len(want) == len(fc.FIRST_BLOCK) == 200
    got = [hashlib.sha256(fc.dumps(fc.make_scenario(seed)).encode()).hexdigest() for seed in fc.FIRST_BLOCK]
    assert got == want, [seed for seed in fc.FIRST_BLOCK if got[seed] != want[seed]]
    assert not any(name.endswith("distance_field") for seed in fc.FIRST_BLOCK for name, _ in fc.make_scenario(seed)["script"])


def _names_with_slots(sc):
    """coverage names of a script, D only where its slot holds a table (elsewhere "D on an empty slot": not the call that completes the tick)"""
    full, out = set(), []
    for name, a in sc["script"]:
        if name == "set_distance_field":
            full.add(a["slot"])
        elif name == "clear_distance_field":
            full.discard(a["slot"])
        out.append((D if a["slot"] in full else "D on an empty slot") if name == D else fc.coverage_name(name, a))
    return out


def test_second_block_every_ordered_pair_with_the_distance_field_call_stands_back_to_back(slice2):
    seen = set()
    for sc, _, _ in slice2:
        names = _names_with_slots(sc)
        seen |= set(zip(names, names[1:]))
    pairs = [(p, q) for p in ALL for q in ALL if D in (p, q)]
    missing = [pq for pq in pairs if pq not in seen]
    print(f"second block, pair matrix: {len(pairs) - len(missing)} of {len(pairs)} ordered pairs with {D}")
    assert len(pairs) == 21 and not missing, missing
    for j, (A, B) in enumerate(fc.DF_PAIRS):       # scenario j of the block is the one that plants pair j, the table set before the first tick
        sc = slice2[j][0]
        names = _names_with_slots(sc)
        assert (A, B) in set(zip(names, names[1:])), (j, A, B)
        assert names.index("set_distance_field") < names.index("step"), j
        if (A, B) == (D, D):
            k = list(zip(names, names[1:])).index((D, D))
            assert sc["script"][k][1]["slot"] != sc["script"][k + 1][1]["slot"], "two different slots"


def test_second_block_the_distance_field_call_meets_every_left_state_and_every_tick_shape(slice2):
    left, shape = set(), set()
    for _, _, info in slice2:
        left |= set(info["call_left"]); shape |= set(info["call_shape"])
    missing = [(D, s) for s in LEFT_STATES if (D, s) not in left] + [(D, s) for s in TICK_SHAPES if (D, s) not in shape]
    assert not missing, missing
    for k in range(fc.N2_PLANTED):                 # ... and the planted scenarios are the ones that say so
        info = slice2[fc.N2_PAIRS + k][2]
        assert (D, LEFT_STATES[k]) in info["call_left"] and (D, TICK_SHAPES[(k + 1) % 4]) in info["call_shape"], k


def test_second_block_every_step_occurs_often_enough(slice2):
    total = collections.Counter()
    for sc, _, _ in slice2:
        total += _features(sc)
    print("steps of the second block: " + ", ".join(f"{k} {v}" for k, v in sorted(total.items())))
    names = ["set_distance_field", "clear_distance_field", "collide_distance_field", "table replaced right behind a call", "collide on an empty slot",
             "slot cleared right behind a call", "slot 0", "slot 1", "slot 2", "slot 3", "prop sphere", "prop floor", "a moving pose"]
    few = {k: total[k] for k in names if total[k] < 10}
    assert not few, few
    assert total["table replaced, the same size"] >= 5 and total["table replaced, another size"] >= 5, "the memory written over, and released"
    assert total["refuse"] == len(slice2), "one refusal per scenario"
    sizes = {a["n"] for sc, _, _ in slice2 for name, a in sc["script"] if name == "set_distance_field" and a["prop"] == "sphere"}
    assert sizes == {9, 17}
    axes = collections.Counter()
    for sc, _, _ in slice2:
        axes[sc["body"]] += 1; axes[sc["mode"]] += 1
        for k in ("peek0", "graph", "uvs", "every_tick"):
            axes[f"{k}={sc[k]}"] += 1
    print("axes of the second block: " + ", ".join(f"{k} {v}" for k, v in sorted(axes.items())))
    assert all(axes[k] >= 8 for k in list(fc.BODIES) + ["full", "render_set", "embedding"] + [f"{k}={v}" for k in ("peek0", "graph", "uvs", "every_tick") for v in (True, False)]), axes


def test_second_block_distance_field_contacts_hit(slice2):
    with_calls = [info for sc, _, info in slice2 if D in _names_with_slots(sc)]
    hit = sum(1 for info in with_calls if any(h > 0 for h in info["distance_field_hits"]))
    calls = [h for info in with_calls for h in info["distance_field_hits"]]
    print(f"signed-distance contacts: a non-empty hit mask in {hit} of {len(with_calls)} scenarios, in {sum(h > 0 for h in calls)} of {len(calls)} calls on a full slot")
    assert len(with_calls) >= fc.N2_PAIRS + fc.N2_PLANTED + fc.N2_LIFETIMES and 2 * hit >= len(with_calls)      # (every written scenario has such a call)
    for sc, _, info in slice2:                      # the list is the signed-distance calls' alone, one entry per call on a full slot
        assert len(info["distance_field_hits"]) == _names_with_slots(sc).count(D), sc["seed"]


def test_second_block_the_steps_listed_as_leaving_the_tick_held_back_do(slice2):
    """the table-lifetime scenarios name the steps that must not complete the tick: behind each, with nothing but such steps and table
    sets between, the next tick fuses -- which is what the GPU's ticks_fused is compared with"""
    listed = 0
    for k in range(fc.N2_LIFETIMES):
        sc, obs, _ = slice2[fc.N2_PAIRS + fc.N2_PLANTED + k]
        assert sc["plan"] == "table lifetime: " + fc.DF_LIFETIMES[k]
        counters = [o[2] for o in obs if o[0] == "counters"]
        assert len(counters) == len(sc["script"])
        for at in sc["leaves_held_back"]:
            assert sc["script"][at][0] in ("set_distance_field", "clear_distance_field", D), (sc["seed"], at)
            nxt = at + 1
            while sc["script"][nxt][0] != "step":
                assert nxt in sc["leaves_held_back"], (sc["seed"], at, "something else stands between the step and the next tick")
                nxt += 1
            assert sc["script"][at - 1][0] == "step" or at - 1 in sc["leaves_held_back"], (sc["seed"], at, "the tick is not held back in front of the step")
            assert counters[at] == counters[at - 1] and counters[nxt][0] == counters[at][0] + 1, (sc["seed"], at, "the next tick does not fuse")
            listed += 1
    names = lambda k: _names_with_slots(slice2[fc.N2_PAIRS + fc.N2_PLANTED + k][0])      # noqa: E731
    assert listed >= 8
    assert "D on an empty slot" in names(3) and "D on an empty slot" in names(4)
    f = names(5)                                   # colliders, terrain, then props: one slot at two poses, then a second slot
    k = f.index("collide_with_reactions")
    assert f[k:k + 5] == ["collide_with_reactions", "collide_heightfield", D, D, D]
    a = [s[1] for s in slice2[fc.N2_PAIRS + fc.N2_PLANTED + 5][0]["script"][k + 2:k + 5]]
    assert a[0]["slot"] == a[1]["slot"] != a[2]["slot"] and a[0]["centre"] != a[1]["centre"]
    g = [n for n, _ in slice2[fc.N2_PAIRS + fc.N2_PLANTED + 6][0]["script"]]
    k = g.index("readback_begin")
    assert g[k:k + 5] == ["readback_begin", D, "readback_end", "raycast", "closest_points"]


def test_counter_model_distance_field_slots(oracle_mod):
    s = ("step", 0.02, 6)
    assert _walk(TickModel(peeking=False), [s, ("set_distance_field", 1), s]) == (1, 0, 0), "a set completes nothing"
    assert _walk(TickModel(peeking=False), [s, ("set_distance_field", 1), s, ("collide_distance_field", 1), s, s]) == (2, 0, 0), "a call on a full slot completes the tick"
    assert _walk(TickModel(peeking=False), [s, ("set_distance_field", 1), s, ("collide_distance_field", 2), s, s]) == (3, 0, 0), "a call on an empty slot does nothing"
    assert _walk(TickModel(peeking=False), [s, ("set_distance_field", 1), ("set_distance_field", 1), ("clear_distance_field", 1), ("collide_distance_field", 1), s]) == (1, 0, 0)
    assert _walk(TickModel(peeking=False), [s, ("kinematic",), ("collide_distance_field", 0), s]) == (1, 1, 0), "... and leaves a pending move pending"
    assert _walk(TickModel(peeking=False), [s, ("set_distance_field", 0), ("kinematic",), ("collide_distance_field", 0), s, s]) == (1, 0, 0), "a call on a full slot lands it"
    # in the driver: the twin of the heightfield script above
    sc = dict(fc.make_scenario(0))
    step = ["step", {"dt": 0.02, "S": 6}]
    call = [D, {"slot": 2, "centre": [7.5, -3.0, 7.5], "quat": [0, 0, 0, 1], "lin": [0, 0, 0], "ang": [0, 0, 0], "friction": 0.1, "restitution": 0.0}]
    table = ["set_distance_field", {"slot": 2, "prop": "sphere", "radius": 4.5, "n": 9, "thickness": 2.7}]
    sc["script"] = [step, call, step, table, step, call, step, ["clear_distance_field", {"slot": 2}], call, step]
    info = {}
    obs = fc.run_reference(oracle_mod, sc, info=info)
    assert obs[-1][2] == (3, 0, 0), obs[-1]
    assert len(info["distance_field_hits"]) == 1 and info["distance_field_hits"][0] > 0 and info["call_left"] == [(D, LEFT_STATES[1])]
