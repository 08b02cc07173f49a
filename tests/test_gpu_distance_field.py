"""Contacts with signed-distance volumes between two ticks on the GPU (SPEC.md 2i; sb_group_set_distance_field,
sb_group_collide_distance_field). A tick is bit-identical to the CPU oracle and a contact is a closed-form float32 rule per particle, so every
comparison is bitwise on x and v, nothing left out: the oracle's state receives the same table and pose from tests/distance_field_ref.py
between its ticks. The inputs are tests/distance_field_cases.py's; tests/test_distance_field.py checks on the CPU that they reach every
branch of the reference."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import distance_field_cases
import distance_field_ref
from distance_field_cases import DT, SIZES
from distance_field_ref import bits, pose_to_native, to_native
from helpers import build_plan, make_oracle
from softbodyunity_amd import SoftbodyGroup, jelly_cube, native
from test_distance_field import bad_distance_fields, bad_poses
from test_gpu_colliders import _free_body

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(g, o, what):
    x, v = g.get_positions(), g.get_velocities()
    assert np.array_equal(bits(x), bits(o.x)), f"{what}: positions"
    assert np.array_equal(bits(v), bits(o.v)), f"{what}: velocities"


def _set(g, slot, df):
    g.set_distance_field(slot, *to_native(df))


def _collide(g, slot, ps):
    g.collide_distance_field(slot, pose_to_native(ps))


def _table(df):
    return 4 * df["nx"] * df["ny"] * df["nz"]


# ---- 1. kernel shapes x grids x frames x motions x cells x float range, no ticks ---------------------------------------------------------------

@pytest.fixture(scope="module")
def cases():
    return distance_field_cases.field_cases()


@pytest.mark.parametrize("n", SIZES)
def test_every_grid_frame_motion_and_cell_over_the_float_range(n, cases):
    w = distance_field_cases.state(n, cases[0][3])[2]
    pinned = w == 0
    nans_made = hits_made = 0
    g = SoftbodyGroup(_free_body(n, w), [0], substeps=4).Start()
    try:
        for k, (name, df, ps, P) in enumerate(cases):
            slot = k % native.SB_DISTANCE_FIELD_SLOTS
            x, v, w1, rows = distance_field_cases.state(n, P)
            assert np.array_equal(w1, w)
            g.set_state(x, v)
            assert np.array_equal(bits(g.get_positions()), bits(x)) and np.array_equal(bits(g.get_velocities()), bits(v)), "set_state changed a value"
            wx, wv = x.copy(), v.copy()
            hit = distance_field_ref.apply(wx, wv, w, df, ps)
            d0 = g.rank(0).stats()["device_bytes"]               # (around the set and the call alone: a state read may allocate its staging)
            _set(g, slot, df)
            _collide(g, slot, ps)
            assert g.rank(0).stats()["device_bytes"] == d0 + _table(df), "the table is counted; the call allocates nothing"
            g.clear_distance_field(slot)                         # right behind the call: it waits for the pass
            assert g.rank(0).stats()["device_bytes"] == d0
            gx, gv = g.get_positions(), g.get_velocities()
            for got, want, what in ((gx, wx, "positions"), (gv, wv, "velocities")):
                bad = bits(got) != bits(want)
                assert not bad.any(), (n, name, what, [(int(p), int(c), hex(bits(got)[p, c]), hex(bits(want)[p, c])) for p, c in np.argwhere(bad)[:8]])
            assert hit[rows[0]] and not hit[pinned].any() and not hit[~np.isfinite(x).all(axis=1)].any()
            assert np.array_equal(bits(gx[~hit]), bits(x[~hit])) and np.array_equal(bits(gv[~hit]), bits(v[~hit])), "untouched and pinned rows keep their bits"
            for got, was in ((gx, x), (gv, v)):
                made = np.isnan(got) & (bits(got) != bits(was))
                assert (bits(got)[made] == 0x7fc00000).all()
                nans_made += int(made.sum())
            hits_made += int(hit.sum())
            if n >= 1023 and "cell" not in name:
                assert (~hit[~pinned]).any() and hit.sum() > 12, name      # (the planted hit and a dozen of the random cloud)
        assert n < 1023 or nans_made > 0, "no case made a NaN"
        assert hits_made >= len(cases)
    finally:
        g.OnDestroy()


# ---- 2. ticking bodies over a sphere that rises and turns through them: one slot, a new pose every tick -------------------------------------------

@pytest.mark.parametrize("compare", ["every_tick", "at_the_end"])
@pytest.mark.parametrize("case", ["cube", "bunny"])
def test_contacts_between_the_ticks_match_the_oracle(case, compare, oracle_mod, monkeypatch):
    # compare = at_the_end: nothing between two ticks reads the state, so the call itself meets the held-back last kernel of the tick
    monkeypatch.setenv("SB_PEEK_MIN_TILES", "0")
    mesh, pins, kw, okw, df, poses = distance_field_cases.ticking_case(case)
    S = kw["substeps"]
    g = SoftbodyGroup(mesh, [0], **kw).Start()
    try:
        o = make_oracle(oracle_mod, mesh, build_plan(mesh), **okw)
        _set(g, 0, df)
        ticks_with_contacts = 0
        for t, ps in enumerate(poses):
            nudge = np.float32([0.02 * t, -0.01 * t, 0.015 * t])
            if t == 2:                    # a move of the pins before the call: the call lands it first
                target = o.x[pins] + nudge
                g.set_kinematic_positions(pins, target); o.set_kinematic_positions(pins, target)
            before = (o.x.copy(), o.v.copy())
            _collide(g, 0, ps)
            hit = distance_field_ref.apply(o.x, o.v, o.w, df, ps)
            ticks_with_contacts += bool(hit.any())
            assert np.array_equal(bits(before[0][pins]), bits(o.x[pins])) and np.array_equal(bits(before[1][pins]), bits(o.v[pins]))
            if t == 4:                    # ... and after it: pending until the tick starts
                target = o.x[pins] + nudge
                g.set_kinematic_positions(pins, target); o.set_kinematic_positions(pins, target)
            if compare == "every_tick" and t & 1:
                assert np.array_equal(bits(g.get_positions()), bits(o.x)), f"positions between the call and the step of tick {t}"
            g.step()
            o.step(DT, S)
            if compare == "every_tick":
                _same(g, o, f"{case}, after tick {t}")
        _same(g, o, f"{case}, at the end")
        at_end = distance_field_ref.apply(o.x.copy(), o.v.copy(), o.w, df, poses[-1])
        print(f"{case}: contacts in {ticks_with_contacts} of {len(poses)} ticks, {at_end.sum()} of {mesh.n} particles hit at the end")
        assert ticks_with_contacts >= 4 and at_end.sum() >= 0.01 * mesh.n
        assert np.isfinite(o.x).all() and np.abs(o.v).max() > 0.05
    finally:
        g.OnDestroy()


# ---- 3. several slots, several poses of one slot, in one frame -------------------------------------------------------------------------------------

def test_two_slots_used_alternately_and_one_slot_at_two_poses_in_one_frame():
    n = 20_000
    rng = np.random.default_rng(37)
    x = rng.uniform(-4, 4, size=(n, 3)).astype(np.float32)
    v = rng.uniform(-2, 2, size=(n, 3)).astype(np.float32)
    w = np.ones(n, np.float32); w[::5] = 0
    ball, side = distance_field_cases.sampled_sphere(1.5, n=21, thickness=0.75)
    nx, ny, nz = distance_field_cases.GRIDS["9x5x17"]
    floor = distance_field_ref.make(distance_field_cases.samples_of(nx, ny, nz), (6.0 / (nx - 1), 6.0 / (ny - 1), 6.0 / (nz - 1)), 0.25, 0.75)
    here = distance_field_cases.pose_about((-1.5, 0.5, 0.0), side, (0, 0, 0, 1), friction=0.3, restitution=0.5)
    there = distance_field_cases.pose_about((1.75, -0.5, 0.5), side, (0.3, -0.5, 0.2, 0.7), friction=0.0, restitution=0.25, **distance_field_cases.MOVING)
    under = distance_field_ref.pose((-3.0, -3.0, -3.0), friction=0.4, restitution=0.0)
    tilted = distance_field_cases._centred(distance_field_ref.pose((0, 0, 0), rot=distance_field_cases.TILT, friction=0.2, restitution=1.0, **distance_field_cases.MOVING), floor)
    g = SoftbodyGroup(_free_body(n, w), [0], substeps=4).Start()
    try:
        g.set_state(x, v)
        d0 = g.rank(0).stats()["device_bytes"]
        _set(g, 1, ball); _set(g, 3, floor)
        assert g.rank(0).stats()["device_bytes"] == d0 + _table(ball) + _table(floor), "every slot's table is counted"
        wx, wv = x.copy(), v.copy()
        hits = []
        for slot, df, ps in ((1, ball, here), (3, floor, under), (1, ball, there), (3, floor, tilted), (0, ball, here), (2, floor, under)):      # (slots 0 and 2 are empty: nothing)
            _collide(g, slot, ps)
            if slot in (1, 3):
                hits.append(int(distance_field_ref.apply(wx, wv, w, df, ps).sum()))
        assert g.rank(0).stats()["device_bytes"] == d0 + _table(ball) + _table(floor)
        assert min(hits) > 100, hits
        assert np.array_equal(bits(g.get_positions()), bits(wx)) and np.array_equal(bits(g.get_velocities()), bits(wv)), hits
        d1 = g.rank(0).stats()["device_bytes"]                # (d0, the tables and what the read allocated)
        g.clear_distance_field(1)
        assert g.rank(0).stats()["device_bytes"] == d1 - _table(ball), "a clear gives back its own slot's table alone"
        _collide(g, 1, here); _collide(g, 3, under)           # slot 1 is empty now, slot 3 still holds the floor
        distance_field_ref.apply(wx, wv, w, floor, under)
        assert np.array_equal(bits(g.get_positions()), bits(wx)) and np.array_equal(bits(g.get_velocities()), bits(wv))
    finally:
        g.OnDestroy()


# ---- 4. previous-position codes --------------------------------------------------------------------------------------------------------------

def test_previous_position_codes_are_dead_between_two_ticks(oracle_mod, monkeypatch):
    """A spring cube on the narrow launch hands previous positions from kernel to kernel as 8-byte codes against x. A plane field through
    the cube's middle with a thick band shoves its lower half up by several units between two ticks: were a code of the tick before read
    by the tick after, its previous position would be decoded against the new x. The first kernel of a tick only writes them."""
    monkeypatch.setenv("SB_NARROW_MIN_TILES", "1")
    monkeypatch.setenv("SB_PEEK_MIN_TILES", "0")
    for k in ("SB_NO_LANE_PACK", "SB_TILE_LANES", "SB_NO_WIDE_SLOTS"):
        monkeypatch.delenv(k, raising=False)
    S = 6
    mesh = jelly_cube(16)
    y = -40.0 + 50.0 * np.arange(3)
    df = distance_field_ref.make(np.broadcast_to((y - 7.5)[None, :, None], (3, 3, 3)), 50.0, 0.0, 100.0)       # phi = y - 7.5 on a 100^3 volume
    ps = distance_field_ref.pose((-40.0, -40.0, -40.0), friction=0.2, restitution=0.3)
    g = SoftbodyGroup(mesh, [0], substeps=S).Start()
    try:
        st = g.rank(0).stats()
        lb, n = st["launch_bytes"], st["n_particles_local"]
        assert lb[2] - lb[0] == 4 * n and lb[3] - lb[0] == 4 * n, ("the coded format is not in force", lb)
        o = make_oracle(oracle_mod, mesh, build_plan(mesh))
        _set(g, 2, df)
        g.step(); o.step(DT, S)
        before = o.x.copy()
        _collide(g, 2, ps)
        hit = distance_field_ref.apply(o.x, o.v, o.w, df, ps)
        assert 0.3 * mesh.n < hit.sum() < 0.6 * mesh.n and np.abs(o.x - before).max() > 5.0
        g.step(); o.step(DT, S)
        assert np.array_equal(bits(g.get_positions()), bits(o.x)), "positions after the first tick behind the call"
        g.step(); o.step(DT, S)
        _same(g, o, "the second tick behind the call")
        assert g.rank(0).stats()["ticks_fused"] >= 1 and np.isfinite(o.x).all()
    finally:
        g.OnDestroy()


# ---- 5. tick fusion, device memory, the tables' lifetime -------------------------------------------------------------------------------------------

def test_a_set_keeps_the_fusion_a_call_breaks_it_once_and_the_tables_are_counted():
    mesh = jelly_cube(12)
    away = distance_field_ref.make(np.ones((5, 5, 5)), 1.0, 0.0, 1.0)                                                # stands far from the body
    y = -10.0 + 10.0 * np.arange(4)
    under = distance_field_ref.make(np.broadcast_to((y - 1.5)[None, :, None], (4, 4, 4)), 10.0, 0.0, 100.0)        # phi = y - 1.5: above its two lowest layers
    far, at = distance_field_ref.pose((-100.0, -100.0, -100.0)), distance_field_ref.pose((-10.0, -10.0, -10.0), friction=0.5)
    g = SoftbodyGroup(mesh, [0], substeps=6).Start()
    try:
        stats = lambda: g.rank(0).stats()       # noqa: E731
        d0 = stats()["device_bytes"]
        for _ in range(3):
            g.step()
        f0 = stats()["ticks_fused"]
        assert stats()["device_bytes"] == d0 and f0 >= 1
        _collide(g, 0, far)
        g.step()
        assert stats()["ticks_fused"] == f0 + 1, "with nothing set in the slot the call does nothing at all: the tick stayed held back and the next one fused"
        _set(g, 0, away)
        assert stats()["device_bytes"] == d0 + _table(away)
        g.step()
        assert stats()["ticks_fused"] == f0 + 2, "a set between two ticks leaves their fusion alone"
        _collide(g, 1, far)
        g.step()
        assert stats()["ticks_fused"] == f0 + 3, "a call on an empty slot beside a full one does nothing either"
        _set(g, 0, away); g.clear_distance_field(0); _set(g, 0, away)
        g.step()
        assert stats()["ticks_fused"] == f0 + 4 and stats()["device_bytes"] == d0 + _table(away), "... and so do a replacement and a clear"
        _collide(g, 0, far)
        assert stats()["device_bytes"] == d0 + _table(away), "the call allocates nothing"
        g.step()
        assert stats()["ticks_fused"] == f0 + 4, "the step after a call starts unfused (a call that touches nothing too)"
        g.step(); g.step()
        assert stats()["ticks_fused"] == f0 + 6, "the steps after it fuse again"
        for _ in range(3):
            _set(g, 0, away); _collide(g, 0, far)
            assert stats()["device_bytes"] == d0 + _table(away), "replacements of equal size and calls keep device_bytes"
        _set(g, 0, under)
        assert stats()["device_bytes"] == d0 + _table(under), "a table of another size releases the one before"
        _collide(g, 0, at)
        assert stats()["device_bytes"] == d0 + _table(under)
        x = g.get_positions()                                 # (a state read may allocate its staging: checked before it)
        assert np.isfinite(x).all() and x[:, 1].min() > 1.5 - 1e-5, "nothing is left under the contact surface"
        d1 = stats()["device_bytes"] - _table(under)          # (d0 and what the read allocated)
        g.clear_distance_field(0)
        g.clear_distance_field(0)
        assert stats()["device_bytes"] == d1 >= d0, "cleared: the table's bytes are back"
        x1 = g.get_positions().copy()
        g.step(); g.step()
        f1 = stats()["ticks_fused"]
        _collide(g, 0, at); g.step()
        assert stats()["ticks_fused"] == f1 + 1, "cleared: the call does nothing again"
        assert not np.array_equal(x1, g.get_positions())
    finally:
        g.OnDestroy()


# ---- 6. a replacement right behind a call ----------------------------------------------------------------------------------------------------------

def test_replacing_the_table_right_behind_a_call_gives_the_first_tables_bits():
    """The pass is asynchronous; the set that follows it writes the same device memory (a table of the same size). It waits for the pass."""
    n = 50_000
    rng = np.random.default_rng(31)
    x = rng.uniform(-4, 4, size=(n, 3)).astype(np.float32)
    v = rng.uniform(-2, 2, size=(n, 3)).astype(np.float32)
    w = np.ones(n, np.float32); w[::5] = 0
    first, side = distance_field_cases.sampled_sphere(2.0, n=97, thickness=1.0)
    second, _ = distance_field_cases.sampled_sphere(2.5, n=97, pad=0.2, thickness=0.5)        # as many samples: the memory is written over
    third, side3 = distance_field_cases.sampled_sphere(1.0, n=33, thickness=0.25)             # another size: the old memory is released
    p1 = distance_field_cases.pose_about((0.5, 0.0, -0.5), side, (0, 0, 0, 1), friction=0.4, restitution=0.5)
    p2 = distance_field_cases.pose_about((0.0, 0.5, 0.0), side, (0.3, -0.5, 0.2, 0.7))
    p3 = distance_field_cases.pose_about((-1.0, -1.0, 1.0), side3, (0, 0, 0, 1), friction=0.3, restitution=1.0)
    g = SoftbodyGroup(_free_body(n, w), [0], substeps=4).Start()
    try:
        g.set_state(x, v)
        wx, wv = x.copy(), v.copy()
        _set(g, 0, first)
        _collide(g, 0, p1)
        _set(g, 0, second)                                    # right behind the call
        h1 = distance_field_ref.apply(wx, wv, w, first, p1)
        assert h1.sum() > 1500
        assert np.array_equal(bits(g.get_positions()), bits(wx)) and np.array_equal(bits(g.get_velocities()), bits(wv)), "the call read the table it was given"
        _collide(g, 0, p2)
        _set(g, 0, third)
        _collide(g, 0, p3)
        g.clear_distance_field(0)                             # right behind the call, too
        h2 = distance_field_ref.apply(wx, wv, w, second, p2)
        h3 = distance_field_ref.apply(wx, wv, w, third, p3)
        assert h2.sum() > 500 and h3.sum() > 100, (h2.sum(), h3.sum())
        assert np.array_equal(bits(g.get_positions()), bits(wx)) and np.array_equal(bits(g.get_velocities()), bits(wv))
    finally:
        g.OnDestroy()


# ---- 7. errors on a live group -------------------------------------------------------------------------------------------------------------------

def test_every_refusal_on_a_live_group_leaves_the_state_and_the_tables_alone():
    L = native.lib()
    fp = lambda s: s.ctypes.data_as(C.POINTER(C.c_float))       # noqa: E731
    y = -10.0 + 10.0 * np.arange(4)
    df = distance_field_ref.make(np.broadcast_to((y - 1.5)[None, :, None], (4, 4, 4)), 10.0, 0.0, 2.0)
    ps = distance_field_ref.pose((-10.0, -10.0, -10.0), friction=0.5, restitution=0.5)
    good, samples = to_native(df)
    pose = pose_to_native(ps)
    d = native.SbDesc(); L.sb_desc_default(C.byref(d))
    early = C.c_void_p()
    assert L.sb_group_create(C.byref(d), None, 1, 0, C.byref(early)) == native.SB_OK
    try:
        assert L.sb_group_set_distance_field(early, 0, C.byref(good), fp(samples)) == native.SB_ERR_STATE and b"sb_group_finalize" in L.sb_last_error()
        assert L.sb_group_set_distance_field(early, 0, None, None) == native.SB_ERR_STATE
        assert L.sb_group_collide_distance_field(early, 0, C.byref(pose)) == native.SB_ERR_STATE and b"sb_group_finalize" in L.sb_last_error()
        bad, bs, _ = bad_distance_fields()[0]
        assert L.sb_group_set_distance_field(early, 0, C.byref(bad), fp(bs)) == native.SB_ERR_INVALID_ARG, "the table is checked first"
        assert L.sb_group_set_distance_field(early, 4, None, None) == native.SB_ERR_INVALID_ARG, "... and so is the slot"
        assert L.sb_group_collide_distance_field(early, 0, C.byref(bad_poses()[0][0])) == native.SB_ERR_INVALID_ARG
    finally:
        L.sb_group_destroy(early)
    g = SoftbodyGroup(jelly_cube(8), [0], substeps=4).Start()
    try:
        g.set_distance_field(1, good, samples)
        g.step()
        x, v = g.get_positions().copy(), g.get_velocities().copy()
        g.step()                                              # a refused call does not complete the held-back tick either ...
        before = g.rank(0).stats()
        for bad, bs, word in bad_distance_fields():
            assert L.sb_group_set_distance_field(g._g, 1, C.byref(bad), fp(bs)) == native.SB_ERR_INVALID_ARG and word in L.sb_last_error().decode(), word
        assert L.sb_group_set_distance_field(g._g, 1, C.byref(good), None) == native.SB_ERR_INVALID_ARG
        for slot in (-1, 4):
            assert L.sb_group_set_distance_field(g._g, slot, C.byref(good), fp(samples)) == native.SB_ERR_INVALID_ARG
            assert L.sb_group_set_distance_field(g._g, slot, None, None) == native.SB_ERR_INVALID_ARG
            assert L.sb_group_collide_distance_field(g._g, slot, C.byref(pose)) == native.SB_ERR_INVALID_ARG
        for bad, word in bad_poses():
            assert L.sb_group_collide_distance_field(g._g, 1, C.byref(bad)) == native.SB_ERR_INVALID_ARG and word in L.sb_last_error().decode(), word
        assert L.sb_group_collide_distance_field(g._g, 1, None) == native.SB_ERR_INVALID_ARG
        assert L.sb_group_collide_distance_field(None, 1, C.byref(pose)) == native.SB_ERR_INVALID_ARG
        assert g.rank(0).stats()["device_bytes"] == before["device_bytes"]
        g.step()
        assert g.rank(0).stats()["ticks_fused"] == before["ticks_fused"] + 1, "... so the next tick still fuses"
        x2, v2 = g.get_positions().copy(), g.get_velocities().copy()
        assert not np.array_equal(bits(x), bits(x2))
        # the table set before the refusals is still in force
        g.collide_distance_field(1, pose)
        want_x, want_v = x2.copy(), v2.copy()
        hit = distance_field_ref.apply(want_x, want_v, np.asarray(g.mesh.inv_mass, np.float32), df, ps)
        assert hit.sum() > 100
        assert np.array_equal(bits(g.get_positions()), bits(want_x)) and np.array_equal(bits(g.get_velocities()), bits(want_v))
    finally:
        g.OnDestroy()


# ---- 8. groups of several ranks ------------------------------------------------------------------------------------------------------------------

_GROUP_CASE_ENDED_ABNORMALLY = []


@pytest.mark.parametrize("host", ["threads", "walk"])
def test_a_group_of_several_ranks_collides_the_whole_body(host):
    # ranks of one process on one device, as tests/test_gpu_group.py runs them: a hardware queue per rank for the peer transport.
    # One subprocess under a timeout. 0 and 1 are the case's own exits (OK / MISMATCH); after any other exit or a timeout the other
    # host model's case is not started here.
    assert not _GROUP_CASE_ENDED_ABNORMALLY, f"not started: the case before ended abnormally ({_GROUP_CASE_ENDED_ABNORMALLY[0]})"
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16")
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "distance_field_group_case.py"), host], env=env, capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired:
        _GROUP_CASE_ENDED_ABNORMALLY.append(f"{host}: timeout")
        raise
    if out.returncode not in (0, 1):
        _GROUP_CASE_ENDED_ABNORMALLY.append(f"{host}: exit {out.returncode}")
    assert out.returncode == 0 and "DISTANCE FIELD GROUP OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
