"""What the body gives back to each collider, on the GPU (SPEC.md 2g; sb_group_collide_reactions / sb_group_get_collider_reactions). The
state is compared bitwise -- with tests/collider_ref.py and with a second group that takes the same list through sb_group_collide --, the
sums against tests/collider_reaction_ref.py within SPEC.md 2g's binding bound (n_contacts + 16) 2^-52 A; counts are exact and a sum that
is not finite in the reference is NaN, +inf or -inf as the reference's is."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import collider_reaction_ref as rref
import collider_ref
from collider_ref import bits, to_native
from helpers import build_plan, make_oracle
from softbodyunity_amd import SoftbodyGroup, jelly_cube, native, sphere_collider
from test_colliders import bad_colliders
from test_gpu_colliders import BATCH, DT, _free_body, hostile_state, shape_cases, ticking_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKGROUP = 1024                 # particles per workgroup of the pass = per row (collide_kernels.hip.hpp: kCollideLanes * kCollidePerLane)
FINAL_RUNS = 8                   # kReactFinalRuns: a final workgroup adds its rows in 8 runs
ROWS_PER_GROUP = 64              # kReactRowsPerGroup: more rows than this are added in two levels
# 20 483 particles = 21 rows: one final workgroup whose runs hold 3 rows each. 68 613 particles = 68 rows > ROWS_PER_GROUP: two levels, the
# first with two workgroups (64 rows and 4: a cut run), the last over their 2 rows. The grid is not capped: no workgroup takes a second chunk.
SIZES = (1, 4, 5, 1023, 1024, 1025, 4099, 20 * WORKGROUP + 3, (ROWS_PER_GROUP + 3) * WORKGROUP + 5)
assert -(-SIZES[-2] // WORKGROUP) > 2 * FINAL_RUNS and ROWS_PER_GROUP < -(-SIZES[-1] // WORKGROUP) < 2 * ROWS_PER_GROUP


def _check_records(got, refs, what):
    assert len(got) == len(refs), what
    worst = 0.0
    for k, (rec, ref) in enumerate(zip(got, refs)):
        why = rref.check(rec, ref)
        assert not why, (what, f"collider {k}", why)
        worst = max(worst, rref.worst_ratio(rec, ref))
    return worst


def finite_state(n, seed):
    """hostile_state with its special rows redrawn: the same inverse masses (pinned rows too), every value ordinary"""
    x, v, w, special = hostile_state(n, seed)
    redo = special | (np.arange(n) % 8 == 0)
    rng = np.random.default_rng(seed + 1000)
    x[redo] = rng.uniform(-4, 4, size=(int(redo.sum()), 3)).astype(np.float32)
    v[redo] = rng.uniform(-2, 2, size=(int(redo.sum()), 3)).astype(np.float32)
    x[0] = hostile_state(n, seed)[0][0]
    v[0] = np.float32([1.0, 1.5, -1.0])                       # particle 0 runs into the single sphere (its centre is 0.1, 0.2, -0.1 away)
    assert np.isfinite(x).all() and np.isfinite(v).all()
    return x, v, w


@pytest.mark.parametrize("n", SIZES)
def test_every_shape_and_list_length_over_the_float_range(n):
    hx, hv, w, _ = hostile_state(n, n)
    fx, fv, _ = finite_state(n, n)
    assert w[0] > 0 and np.array_equal(hx[0], fx[0])
    g = SoftbodyGroup(_free_body(n, w), [0], substeps=4).Start()
    plain = SoftbodyGroup(_free_body(n, w), [0], substeps=4).Start()
    try:
        worst, odd_sums = 0.0, 0
        for state, (x, v) in (("hostile", (hx, hv)), ("finite", (fx, fv))):
            moved = dict(impulse=False, torque=False)
            for name, cols in shape_cases(x[0]).items():
                assert len(cols) in (1, BATCH, BATCH + 1, 2 * BATCH + 1)
                what = (n, state, name)
                g.set_state(x, v); plain.set_state(x, v)
                wx, wv = x.copy(), v.copy()
                hits, refs = rref.apply(wx, wv, w, cols)
                items = [to_native(c) for c in cols]
                g.collide_with_reactions(items)
                plain.collide(items)
                gx, gv = g.get_positions(), g.get_velocities()
                assert np.array_equal(bits(gx), bits(wx)) and np.array_equal(bits(gv), bits(wv)), (what, "the state is not the reference's")
                assert np.array_equal(bits(gx), bits(plain.get_positions())) and np.array_equal(bits(gv), bits(plain.get_velocities())), (what, "not sb_group_collide's bits")
                got = g.collider_reactions()
                worst = max(worst, _check_records(got, refs, what))
                assert [int(r["n_contacts"]) for r in got] == hits.sum(axis=1).tolist(), what
                odd_sums += sum(int((~np.isfinite(r["sums"])).sum()) for r in refs)
                if state == "finite":
                    assert all(np.isfinite(rref.record_sums(r)).all() for r in got), what
                    if len(cols) == 1 and not name.startswith("mixed"):
                        assert got[0]["n_contacts"] > 0, (what, "the collider hit nothing")
                        moved["impulse"] |= bool(np.any(got["impulse"] != 0)); moved["torque"] |= bool(np.any(got["angular_impulse"] != 0))
            if state == "finite":
                assert moved["impulse"] and moved["torque"], (n, "no single shape took an impulse and a torque", moved)
        print(f"n = {n}: worst error / bound = {worst:.3f}, non-finite reference sums met = {odd_sums}")
        assert n < 1023 or odd_sums > 0, "the hostile state made no sum NaN or infinite"
    finally:
        plain.OnDestroy()
        g.OnDestroy()


def test_the_known_answer_is_exact():
    """tests/test_collider_reactions.py's one particle of mass 2 in the unit box: every term is exact in binary64, so the record is too"""
    w = np.float32([0.5])
    g = SoftbodyGroup(_free_body(1, w), [0], substeps=4).Start()
    try:
        g.set_state(np.float32([[0.25, 0.75, 0.0]]), np.float32([[0.0, -3.0, 0.0]]))
        g.collide_with_reactions([to_native(collider_ref.box((0, 0, 0), np.eye(3), (1, 1, 1), friction=0.0, restitution=0.5))])
        (rec,) = g.collider_reactions()
        assert g.get_positions().tolist() == [[0.25, 1.0, 0.0]] and g.get_velocities().tolist() == [[0.0, 1.5, 0.0]]
        assert rec["impulse"].tolist() == [0.0, -9.0, 0.0] and rec["angular_impulse"].tolist() == [0.0, 0.0, -2.25]
        assert rec["contact_mass"] == 2.0 and rec["n_contacts"] == 1
    finally:
        g.OnDestroy()


# ---- the fetch ---------------------------------------------------------------------------------------------------------------------------------

def _raw_fetch(g, capacity):
    out = (native.SbColliderReaction * max(1, capacity))()
    n = C.c_int32(-1)
    assert native.lib().sb_group_get_collider_reactions(g._g, out, capacity, C.byref(n)) == native.SB_OK
    return bytes(out)[:64 * capacity], n.value


def _cube_lists(mesh):
    mid = mesh.pos.mean(axis=0)
    ball = sphere_collider(mid + np.float32([0.3, -2.0, 0.1]), 3.5, lin=(0.5, 2.0, 0), ang=(0, 1, 0.5), friction=0.4, restitution=0.2)
    rng = np.random.default_rng(3)
    many = [sphere_collider(rng.uniform(1, 10, size=3), float(rng.uniform(1.0, 2.5)), lin=rng.uniform(-1, 1, size=3), friction=0.3, restitution=0.5) for _ in range(BATCH + 3)]
    return [ball], many


def test_the_fetch_repeats_truncates_waits_for_its_call_alone_and_the_buffers_are_allocated_once():
    L = native.lib()
    mesh = jelly_cube(12)
    one, many = _cube_lists(mesh)
    d = native.SbDesc(); L.sb_desc_default(C.byref(d))
    early = C.c_void_p()
    assert L.sb_group_create(C.byref(d), None, 1, 0, C.byref(early)) == native.SB_OK
    try:
        n = C.c_int32(-1)
        out = (native.SbColliderReaction * 1)()
        items = (native.SbCollider * 1)(one[0])
        assert L.sb_group_collide_reactions(early, items, 1) == native.SB_ERR_STATE and b"sb_group_finalize" in L.sb_last_error()
        assert L.sb_group_collide_reactions(early, items, 0) == native.SB_ERR_STATE
        assert L.sb_group_collide_reactions(early, (native.SbCollider * 1)(bad_colliders()[0][0]), 1) == native.SB_ERR_INVALID_ARG, "the list is checked first"
        assert L.sb_group_get_collider_reactions(early, out, 1, C.byref(n)) == native.SB_ERR_STATE and n.value == -1
    finally:
        L.sb_group_destroy(early)
    g = SoftbodyGroup(mesh, [0], substeps=6).Start()
    twin = SoftbodyGroup(mesh, [0], substeps=6).Start()
    try:
        stats = lambda: g.rank(0).stats()       # noqa: E731
        for h in (g, twin):
            h.step(); h.step()
        d0 = stats()["device_bytes"]
        assert _raw_fetch(g, 4) == (bytes(256), 0), "before any reactions call: count 0, nothing written"
        g.collide(one)
        assert stats()["device_bytes"] == d0 and _raw_fetch(g, 4)[1] == 0, "sb_group_collide allocates nothing and reports nothing"
        g.collide_with_reactions(many); twin.collide(one); twin.collide_with_reactions(many)
        d1 = stats()["device_bytes"]
        assert d1 > d0, "the first reactions call allocates the rows"
        first, count = _raw_fetch(g, len(many))
        assert count == len(many) and _raw_fetch(g, len(many)) == (first, count), "a second fetch returns the same bits"
        assert _raw_fetch(twin, len(many)) == (first, count), "two identical groups give identical bits"
        recs = g.collider_reactions()
        assert recs.tobytes() == first and (recs["n_contacts"] > 0).sum() > 3 and np.any(recs["impulse"] != 0)
        assert _raw_fetch(g, 5) == (first[:64 * 5], count) and _raw_fetch(g, 0) == (b"", count), "capacity < count truncates and still reports count"
        assert len(g.collider_reactions(capacity=2)) == 2
        # a refused call, a plain collide, ticks and a placement in between leave the stored records alone
        assert L.sb_group_collide_reactions(g._g, (native.SbCollider * 1)(bad_colliders()[0][0]), 1) == native.SB_ERR_INVALID_ARG
        g.collide(one); g.step(); g.step()
        f0 = stats()["ticks_fused"]
        assert _raw_fetch(g, len(many)) == (first, count)
        g.step()
        assert stats()["ticks_fused"] == f0 + 1, "a fetch completes nothing: the held-back kernel still fuses with the next tick"
        g.place(to=(0.5, 0.25, 0))
        assert _raw_fetch(g, len(many)) == (first, count)
        # later calls replace the records and allocate nothing
        g.collide_with_reactions(one)
        again, count = _raw_fetch(g, len(many))
        assert count == 1 and again[:64] != first[:64] and again[64:] == bytes(64 * (len(many) - 1)), "min(count, capacity) records are written"
        g.collide_with_reactions(many * 3)
        assert _raw_fetch(g, 1)[1] == 3 * len(many)
        g.collide(many)
        assert stats()["device_bytes"] == d1, "device_bytes is constant from the second call on"
        f1 = stats()["ticks_fused"]
        g.collide_with_reactions([])
        assert _raw_fetch(g, 4) == (bytes(256), 0), "count == 0: no records"
        g.step(); g.step(); g.collide_with_reactions([]); g.step()
        assert stats()["ticks_fused"] == f1 + 2, "count == 0 does nothing to the state: only the step behind the real call started unfused"
        assert L.sb_group_collide_reactions(g._g, (native.SbCollider * (native.SB_COLLIDE_REACTIONS_MAX + 1))(*[one[0]] * (native.SB_COLLIDE_REACTIONS_MAX + 1)),
                                            native.SB_COLLIDE_REACTIONS_MAX + 1) == native.SB_ERR_INVALID_ARG
        g.collide_with_reactions([sphere_collider((100, 100, 100), 1.0)] * native.SB_COLLIDE_REACTIONS_MAX)
        full = g.collider_reactions()
        assert len(full) == native.SB_COLLIDE_REACTIONS_MAX and full.tobytes() == bytes(64 * len(full)) and stats()["device_bytes"] == d1
    finally:
        twin.OnDestroy()
        g.OnDestroy()


# ---- ticking bodies ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["cube", "bunny"])
def test_reactions_between_the_ticks_match_the_oracle_and_a_late_fetch_is_the_same(case, oracle_mod):
    mesh, pins, kw, okw, colliders_of_tick = ticking_case(case)
    S = kw["substeps"]
    g = SoftbodyGroup(mesh, [0], **kw).Start()
    late = SoftbodyGroup(mesh, [0], **kw).Start()
    try:
        o = make_oracle(oracle_mod, mesh, build_plan(mesh), **okw)
        worst = 0.0
        for t in range(5):
            nudge = np.float32([0.02 * t, -0.01 * t, 0.015 * t])
            if t == 2:                    # a move of the pins before the call: the call lands it first
                target = o.x[pins] + nudge
                for h in (g, late, o):
                    h.set_kinematic_positions(pins, target)
            cols = colliders_of_tick(t)
            items = [to_native(c) for c in cols]
            g.collide_with_reactions(items); late.collide_with_reactions(items)
            hits, refs = rref.apply(o.x, o.v, o.w, cols)
            assert hits[0].any() and not hits[:, pins].any(), (t, hits.sum(axis=1))
            if t == 3:                    # ... and after it: pending until the tick starts
                target = o.x[pins] + nudge
                for h in (g, late, o):
                    h.set_kinematic_positions(pins, target)
            got = g.collider_reactions()                       # at once
            worst = max(worst, _check_records(got, refs, (case, t)))
            assert np.any(got["impulse"][0] != 0) and np.any(got["angular_impulse"][0] != 0), (case, t, "the rising ball took nothing")
            g.step(); late.step(); o.step(DT, S)
            assert late.collider_reactions().tobytes() == got.tobytes(), (case, t, "a fetch behind the next step's launch differs")
            if t & 1:
                assert np.array_equal(bits(g.get_positions()), bits(o.x)) and np.array_equal(bits(g.get_velocities()), bits(o.v)), (case, t)
        for h in (g, late):
            assert np.array_equal(bits(h.get_positions()), bits(o.x)) and np.array_equal(bits(h.get_velocities()), bits(o.v)), (case, "at the end")
        print(f"{case}: worst error / bound = {worst:.3f}")
        assert np.isfinite(o.x).all() and np.abs(o.v).max() > 0.05
        assert late.rank(0).stats()["ticks_fused"] >= g.rank(0).stats()["ticks_fused"], "the late fetch cost no fused boundary"
    finally:
        late.OnDestroy()
        g.OnDestroy()


# ---- groups of several ranks -------------------------------------------------------------------------------------------------------------------

_GROUP_CASE_ENDED_ABNORMALLY = []


@pytest.mark.parametrize("host", ["threads", "walk"])
def test_a_group_of_several_ranks_counts_every_contact_once(host):
    # ranks of one process on one device, as tests/test_gpu_colliders.py runs them. One subprocess under a timeout. 0 and 1 are the case's
    # own exits (OK / MISMATCH); after any other exit or a timeout the other host model's case is not started here.
    assert not _GROUP_CASE_ENDED_ABNORMALLY, f"not started: the case before ended abnormally ({_GROUP_CASE_ENDED_ABNORMALLY[0]})"
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16")
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "collider_reaction_group_case.py"), host], env=env, capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired:
        _GROUP_CASE_ENDED_ABNORMALLY.append(f"{host}: timeout")
        raise
    if out.returncode not in (0, 1):
        _GROUP_CASE_ENDED_ABNORMALLY.append(f"{host}: exit {out.returncode}")
    assert out.returncode == 0 and "COLLIDER REACTION GROUP OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
