"""Heightfield contacts between two ticks on the GPU (SPEC.md 2h; sb_group_set_heightfield, sb_group_collide_heightfield). A tick is
bit-identical to the CPU oracle and a contact is a closed-form float32 rule per particle, so every comparison is bitwise on x and v, nothing
left out: the oracle's state receives the same table from tests/heightfield_ref.py between its ticks. The inputs are
tests/heightfield_cases.py's; tests/test_heightfield.py checks on the CPU that they reach every branch of the reference."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import heightfield_cases
import heightfield_ref
from heightfield_cases import DT, SIZES
from heightfield_ref import bits, to_native
from helpers import build_plan, make_oracle
from softbodyunity_amd import SoftbodyGroup, jelly_cube, native
from test_gpu_colliders import _free_body
from test_heightfield import bad_heightfields

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(g, o, what):
    x, v = g.get_positions(), g.get_velocities()
    assert np.array_equal(bits(x), bits(o.x)), f"{what}: positions"
    assert np.array_equal(bits(v), bits(o.v)), f"{what}: velocities"


def _set(g, hf):
    g.set_heightfield(*to_native(hf))


# ---- a. kernel shapes x grids x frames x cells x float range, no ticks -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cases():
    return heightfield_cases.field_cases()


@pytest.mark.parametrize("n", SIZES)
def test_every_grid_frame_and_cell_over_the_float_range(n, cases):
    w = heightfield_cases.state(n, cases[0][4])[2]
    pinned = w == 0
    nans_made = hits_made = 0
    g = SoftbodyGroup(_free_body(n, w), [0], substeps=4).Start()
    try:
        for name, hf, friction, restitution, P in cases:
            x, v, w1, rows = heightfield_cases.state(n, P)
            assert np.array_equal(w1, w)
            g.set_state(x, v)
            assert np.array_equal(bits(g.get_positions()), bits(x)) and np.array_equal(bits(g.get_velocities()), bits(v)), "set_state changed a value"
            wx, wv = x.copy(), v.copy()
            hit = heightfield_ref.apply(wx, wv, w, hf, friction, restitution)
            d0 = g.rank(0).stats()["device_bytes"]               # (around the set and the call alone: a state read may allocate its staging)
            _set(g, hf)
            g.collide_heightfield(friction, restitution)
            assert g.rank(0).stats()["device_bytes"] == d0 + 4 * hf["nx"] * hf["nz"], "the table is counted; the call allocates nothing"
            g.clear_heightfield()                                # right behind the call: it waits for the pass
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
                assert (~hit[~pinned]).any() and hit.sum() > 20, name
        assert n < 1023 or nans_made > 0, "no case made a NaN"
        assert hits_made >= len(cases)
    finally:
        g.OnDestroy()


# ---- b. ticking bodies -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("compare", ["every_tick", "at_the_end"])
@pytest.mark.parametrize("peek_small", [False, True])
@pytest.mark.parametrize("case", ["cube", "bunny"])
def test_contacts_between_the_ticks_match_the_oracle(case, peek_small, compare, oracle_mod, monkeypatch):
    # compare = at_the_end: nothing between two ticks reads the state, so the call itself meets the held-back last kernel of the tick
    if peek_small:
        monkeypatch.setenv("SB_PEEK_MIN_TILES", "0")
    else:
        monkeypatch.delenv("SB_PEEK_MIN_TILES", raising=False)
    mesh, pins, kw, okw, hf = heightfield_cases.ticking_case(case)
    S = kw["substeps"]
    friction, restitution = 0.5, 0.1
    g = SoftbodyGroup(mesh, [0], **kw).Start()
    try:
        o = make_oracle(oracle_mod, mesh, build_plan(mesh), **okw)
        _set(g, hf)
        ticks_with_contacts = 0
        for t in range(6):
            nudge = np.float32([0.02 * t, -0.01 * t, 0.015 * t])
            if t == 2:                    # a move of the pins before the call: the call lands it first
                target = o.x[pins] + nudge
                g.set_kinematic_positions(pins, target); o.set_kinematic_positions(pins, target)
            before = (o.x.copy(), o.v.copy())
            g.collide_heightfield(friction, restitution)
            hit = heightfield_ref.apply(o.x, o.v, o.w, hf, friction, restitution)
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
        at_end = heightfield_ref.apply(o.x.copy(), o.v.copy(), o.w, hf, friction, restitution)
        print(f"{case}: contacts in {ticks_with_contacts} of 6 ticks, {at_end.sum()} of {mesh.n} particles hit at the end")
        assert ticks_with_contacts >= 3 and 0.02 * mesh.n <= at_end.sum() <= 0.6 * mesh.n
        assert np.isfinite(o.x).all() and np.abs(o.v).max() > 0.05
    finally:
        g.OnDestroy()


# ---- c. previous-position codes --------------------------------------------------------------------------------------------------------------

def test_previous_position_codes_are_dead_between_two_ticks(oracle_mod, monkeypatch):
    """A spring cube on the narrow launch hands previous positions from kernel to kernel as 8-byte codes against x. A thick, slightly tilted
    field through the cube's middle lifts its lower half by up to 7.5 units between two ticks: were a code of the tick before read by the
    tick after, its previous position would be decoded against the new x. The first kernel of a tick only writes them."""
    monkeypatch.setenv("SB_NARROW_MIN_TILES", "1")
    monkeypatch.setenv("SB_PEEK_MIN_TILES", "0")
    for k in ("SB_NO_LANE_PACK", "SB_TILE_LANES", "SB_NO_WIDE_SLOTS"):
        monkeypatch.delenv(k, raising=False)
    S = 6
    mesh = jelly_cube(16)
    hf = heightfield_ref.make((-40.0, 0.0, -40.0), 100.0, np.float32([[7.25, 7.5], [7.5, 7.75]]), thickness=100.0)
    g = SoftbodyGroup(mesh, [0], substeps=S).Start()
    try:
        st = g.rank(0).stats()
        lb, n = st["launch_bytes"], st["n_particles_local"]
        assert lb[2] - lb[0] == 4 * n and lb[3] - lb[0] == 4 * n, ("the coded format is not in force", lb)
        o = make_oracle(oracle_mod, mesh, build_plan(mesh))
        _set(g, hf)
        g.step(); o.step(DT, S)
        before = o.x.copy()
        g.collide_heightfield(0.2, 0.3)
        hit = heightfield_ref.apply(o.x, o.v, o.w, hf, 0.2, 0.3)
        assert 0.3 * mesh.n < hit.sum() < 0.6 * mesh.n and np.abs(o.x - before).max() > 5.0
        g.step(); o.step(DT, S)
        assert np.array_equal(bits(g.get_positions()), bits(o.x)), "positions after the first tick behind the call"
        g.step(); o.step(DT, S)
        _same(g, o, "the second tick behind the call")
        assert g.rank(0).stats()["ticks_fused"] >= 1 and np.isfinite(o.x).all()
    finally:
        g.OnDestroy()


# ---- d. tick fusion, device memory, the table's lifetime ---------------------------------------------------------------------------------------

def test_a_set_keeps_the_fusion_a_call_breaks_it_once_and_the_table_is_counted():
    mesh = jelly_cube(12)
    below = heightfield_ref.make((-10.0, -50.0, -10.0), 4.0, np.zeros((9, 9)), thickness=1.0)          # wholly below the body
    under = heightfield_ref.make((-10.0, 0.0, -10.0), 2.0, np.full((17, 17), 1.5), thickness=100.0)    # above its two lowest layers
    table = lambda hf: 4 * hf["nx"] * hf["nz"]       # noqa: E731
    g = SoftbodyGroup(mesh, [0], substeps=6).Start()
    try:
        stats = lambda: g.rank(0).stats()       # noqa: E731
        d0 = stats()["device_bytes"]
        for _ in range(3):
            g.step()
        f0 = stats()["ticks_fused"]
        assert stats()["device_bytes"] == d0 and f0 >= 1
        g.collide_heightfield(0.5, 0.0)
        g.step()
        assert stats()["ticks_fused"] == f0 + 1, "with no heightfield set the call does nothing at all: the tick stayed held back and the next one fused"
        _set(g, below)
        assert stats()["device_bytes"] == d0 + table(below)
        g.step()
        assert stats()["ticks_fused"] == f0 + 2, "a set between two ticks leaves their fusion alone"
        _set(g, below); g.clear_heightfield(); _set(g, below)
        g.step()
        assert stats()["ticks_fused"] == f0 + 3 and stats()["device_bytes"] == d0 + table(below), "... and so do a replacement and a clear"
        g.collide_heightfield(0.5, 0.0)
        assert stats()["device_bytes"] == d0 + table(below), "the call allocates nothing"
        g.step()
        assert stats()["ticks_fused"] == f0 + 3, "the step after a call starts unfused (a call that touches nothing too)"
        g.step(); g.step()
        assert stats()["ticks_fused"] == f0 + 5, "the steps after it fuse again"
        for _ in range(3):
            _set(g, below); g.collide_heightfield(0.5, 0.0)
            assert stats()["device_bytes"] == d0 + table(below), "replacements of equal size and calls keep device_bytes"
        _set(g, under)
        assert stats()["device_bytes"] == d0 + table(under), "a table of another size releases the one before"
        g.collide_heightfield(0.5, 0.0)
        assert stats()["device_bytes"] == d0 + table(under)
        x = g.get_positions()                                 # (a state read may allocate its staging: checked before it)
        assert np.isfinite(x).all() and x[:, 1].min() > 1.5 - 1e-5, "nothing is left under the field"
        d1 = stats()["device_bytes"] - table(under)           # (d0 and what the read allocated)
        g.clear_heightfield()
        g.clear_heightfield()
        assert stats()["device_bytes"] == d1 >= d0, "cleared: the table's bytes are back"
        x1 = g.get_positions().copy()
        g.step(); g.step()
        f1 = stats()["ticks_fused"]
        g.collide_heightfield(0.5, 0.0); g.step()
        assert stats()["ticks_fused"] == f1 + 1, "cleared: the call does nothing again"
        assert not np.array_equal(x1, g.get_positions())
    finally:
        g.OnDestroy()


def test_replacing_the_table_right_behind_a_call_gives_the_first_tables_bits():
    """The pass is asynchronous; the set that follows it writes the same device memory (a table of the same size). It waits for the pass."""
    n = 50_000
    rng = np.random.default_rng(31)
    x = rng.uniform(-4, 4, size=(n, 3)).astype(np.float32)
    v = rng.uniform(-2, 2, size=(n, 3)).astype(np.float32)
    w = np.ones(n, np.float32); w[::5] = 0
    nx = nz = 513
    ix, iz = np.meshgrid(np.arange(nx), np.arange(nz))
    first = heightfield_ref.make((-3.0, 0.0, -3.0), 6.0 / (nx - 1), 0.5 * np.sin(0.05 * ix) * np.cos(0.07 * iz), thickness=1.0)
    second = heightfield_ref.make((-3.0, 0.0, -3.0), 6.0 / (nx - 1), 2.0 + 0.0 * ix, thickness=0.5)
    third = heightfield_ref.make((-3.0, 0.0, -3.0), 12.0 / (nx // 2 - 1), np.full((nz // 2, nx // 2), -1.0), thickness=0.25)      # another size: the old memory is released
    g = SoftbodyGroup(_free_body(n, w), [0], substeps=4).Start()
    try:
        g.set_state(x, v)
        wx, wv = x.copy(), v.copy()
        _set(g, first)
        g.collide_heightfield(0.4, 0.5)
        _set(g, second)                                       # right behind the call
        h1 = heightfield_ref.apply(wx, wv, w, first, 0.4, 0.5)
        assert h1.sum() > 1500
        assert np.array_equal(bits(g.get_positions()), bits(wx)) and np.array_equal(bits(g.get_velocities()), bits(wv)), "the call read the table it was given"
        g.collide_heightfield(0.0, 0.0)
        _set(g, third)
        g.collide_heightfield(0.3, 1.0)
        g.clear_heightfield()                                 # right behind the call, too
        h2 = heightfield_ref.apply(wx, wv, w, second, 0.0, 0.0)
        h3 = heightfield_ref.apply(wx, wv, w, third, 0.3, 1.0)
        assert h2.sum() > 500 and h3.sum() > 250
        assert np.array_equal(bits(g.get_positions()), bits(wx)) and np.array_equal(bits(g.get_velocities()), bits(wv))
    finally:
        g.OnDestroy()


# ---- e. errors on a live group ---------------------------------------------------------------------------------------------------------------

def test_every_refusal_on_a_live_group_leaves_the_state_and_the_table_alone():
    L = native.lib()
    fp = lambda h: h.ctypes.data_as(C.POINTER(C.c_float))       # noqa: E731
    hf = heightfield_ref.make((-10.0, 0.0, -10.0), 2.0, np.full((17, 17), 1.5), thickness=2.0)
    good, heights = to_native(hf)
    d = native.SbDesc(); L.sb_desc_default(C.byref(d))
    early = C.c_void_p()
    assert L.sb_group_create(C.byref(d), None, 1, 0, C.byref(early)) == native.SB_OK
    try:
        assert L.sb_group_set_heightfield(early, C.byref(good), fp(heights)) == native.SB_ERR_STATE and b"sb_group_finalize" in L.sb_last_error()
        assert L.sb_group_set_heightfield(early, None, None) == native.SB_ERR_STATE
        assert L.sb_group_collide_heightfield(early, 0.0, 0.0) == native.SB_ERR_STATE and b"sb_group_finalize" in L.sb_last_error()
        bad, bh, _ = bad_heightfields()[0]
        assert L.sb_group_set_heightfield(early, C.byref(bad), fp(bh)) == native.SB_ERR_INVALID_ARG, "the table is checked first"
        assert L.sb_group_collide_heightfield(early, -1.0, 0.0) == native.SB_ERR_INVALID_ARG
    finally:
        L.sb_group_destroy(early)
    g = SoftbodyGroup(jelly_cube(8), [0], substeps=4).Start()
    try:
        g.set_heightfield(good, heights)
        g.step()
        x, v = g.get_positions().copy(), g.get_velocities().copy()
        g.step()                                              # a refused call does not complete the held-back tick either ...
        before = g.rank(0).stats()
        for bad, bh, word in bad_heightfields():
            assert L.sb_group_set_heightfield(g._g, C.byref(bad), fp(bh)) == native.SB_ERR_INVALID_ARG and word in L.sb_last_error().decode(), word
        assert L.sb_group_set_heightfield(g._g, C.byref(good), None) == native.SB_ERR_INVALID_ARG
        for friction, restitution in ((-0.125, 0.0), (np.nan, 0.0), (0.0, np.inf), (0.0, -0.125), (0.0, 1.0 + 2.0 ** -23)):
            assert L.sb_group_collide_heightfield(g._g, friction, restitution) == native.SB_ERR_INVALID_ARG
        assert L.sb_group_collide_heightfield(None, 0.0, 0.0) == native.SB_ERR_INVALID_ARG
        assert g.rank(0).stats()["device_bytes"] == before["device_bytes"]
        g.step()
        assert g.rank(0).stats()["ticks_fused"] == before["ticks_fused"] + 1, "... so the next tick still fuses"
        x2, v2 = g.get_positions().copy(), g.get_velocities().copy()
        assert not np.array_equal(bits(x), bits(x2))
        # the table set before the refusals is still in force
        g.collide_heightfield(0.5, 0.5)
        want_x, want_v = x2.copy(), v2.copy()
        hit = heightfield_ref.apply(want_x, want_v, np.asarray(g.mesh.inv_mass, np.float32), hf, 0.5, 0.5)
        assert hit.sum() > 100
        assert np.array_equal(bits(g.get_positions()), bits(want_x)) and np.array_equal(bits(g.get_velocities()), bits(want_v))
    finally:
        g.OnDestroy()


# ---- f. groups of several ranks ------------------------------------------------------------------------------------------------------------------

_GROUP_CASE_ENDED_ABNORMALLY = []


@pytest.mark.parametrize("host", ["threads", "walk"])
def test_a_group_of_several_ranks_collides_the_whole_body(host):
    # ranks of one process on one device, as tests/test_gpu_group.py runs them: a hardware queue per rank for the peer transport.
    # One subprocess under a timeout. 0 and 1 are the case's own exits (OK / MISMATCH); after any other exit or a timeout the other
    # host model's case is not started here.
    assert not _GROUP_CASE_ENDED_ABNORMALLY, f"not started: the case before ended abnormally ({_GROUP_CASE_ENDED_ABNORMALLY[0]})"
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16")
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "heightfield_group_case.py"), host], env=env, capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired:
        _GROUP_CASE_ENDED_ABNORMALLY.append(f"{host}: timeout")
        raise
    if out.returncode not in (0, 1):
        _GROUP_CASE_ENDED_ABNORMALLY.append(f"{host}: exit {out.returncode}")
    assert out.returncode == 0 and "HEIGHTFIELD GROUP OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
