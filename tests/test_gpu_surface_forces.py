"""Surface forces between two ticks on the GPU (SPEC.md 2e; sb_group_apply_surface_forces). A tick is bit-identical to the CPU oracle and a
call is a closed-form float32 update of the velocities, so every comparison is bitwise: the oracle's `v` receives the same update from
tests/surface_force_ref.py between its ticks. The entry point is the group's (a group of one device), as for a placement."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import surface_force_ref
from helpers import build_plan, make_oracle
from softbodyunity_amd import SoftbodyGroup, from_triangle_mesh, jelly_cube, make_surface_force, native
from softbodyunity_amd.mesh import SoftbodyMesh
from surface_force_ref import bits
from test_surface_forces import bad_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

N = 512
ALL = dict(wind=(1.5, -0.75, 2.25), normal=3.0, tangential=0.75, pressure=-1.25, dt=0.02)
POOL = np.array([0x00000000, 0x80000000, 0x000116c2, 0x80000001, 0x7f800000, 0xff800000, 0x7f61b1e6, 0xff61b1e6, 0x7fc12345, 0xffc00001,
                 0x3fc00000, 0xc0100000, 0x3a83126f, 0x40e00000], np.uint32)      # +-0, subnormals, +-inf, +-3e38, NaNs with payload and sign, ordinary


def _free_body(n, inv_mass):
    """n particles without constraints (the planner never sees the test's state: it arrives through set_state)"""
    i = np.arange(n)
    rest = (np.stack([i % 8, (i // 8) % 8, i // 64], axis=1) * 0.5).astype(np.float32)
    return SoftbodyMesh(rest_pos=rest, pos=rest.copy(), vel=np.zeros((n, 3), np.float32), inv_mass=np.asarray(inv_mass, np.float32),
                        dist_ij=np.zeros((0, 2), np.int32), dist_rest=np.zeros(0, np.float32))


def _still_state(seed=3):
    rng = np.random.default_rng(seed)
    w = rng.choice(np.float32([0, 0.5, 1, 2, 3]), size=N).astype(np.float32)
    x = rng.uniform(-2, 2, size=(N, 3)).astype(np.float32)
    v = rng.uniform(-1, 1, size=(N, 3)).astype(np.float32)
    return w, x, v, rng


def _check(g, x, v, w, tri, what, **force):
    """set the state, apply on the device and in the reference, compare every bit -> the reference's velocities"""
    g.set_state(x, v)
    assert np.array_equal(bits(g.get_positions()), bits(x)) and np.array_equal(bits(g.get_velocities()), bits(v)), "set_state changed a value"
    want = v.copy()
    surface_force_ref.apply(x, want, w, tri, **force)
    g.apply_surface_forces(**force)
    got = g.get_velocities()
    assert np.array_equal(bits(g.get_positions()), bits(x)), f"{what}: positions never change"
    bad = bits(got) != bits(want)
    assert not bad.any(), (what, int(bad.any(axis=1).sum()), [(int(p), int(c), hex(bits(got)[p, c]), hex(bits(want)[p, c])) for p, c in np.argwhere(bad)[:8]])
    return want


# ---- 1. kernel shapes on a still free body ----------------------------------------------------------------------------------------------------

def _shape(case, rng):
    """-> (m, 3) triangles over the N particles of the still body"""
    if case.startswith("count_"):
        return rng.integers(0, N, size=(int(case[6:]), 3))
    if case == "fan_300":                         # one lane's list is longer than a wavefront and longer than a workgroup
        ring = 1 + np.arange(301)
        return np.stack([np.zeros(300, np.int64), ring[:-1], ring[1:]], axis=1)
    if case.startswith("strip_"):                 # P render particles: P - 2 triangles, every particle's list 1 .. 3 long
        i = 7 + np.arange(int(case[6:]) - 2)
        return np.stack([i, i + 1, i + 2], axis=1)
    if case == "repeated_vertex":
        return np.array([[3, 3, 9], [3, 9, 3], [9, 3, 3], [11, 11, 11], [3, 9, 20], [20, 9, 40], [40, 40, 3], [3, 20, 40]])
    assert case == "first_and_last"
    tri = rng.integers(10, 200, size=(100, 3))
    tri[0] = (5, 17, 80); tri[-1] = (90, 5, 33)
    return tri


SHAPES = ["count_1", "count_2", "count_255", "count_256", "count_257", "fan_300", "strip_255", "strip_256", "strip_257", "repeated_vertex", "first_and_last"]


@pytest.mark.parametrize("case", SHAPES)
def test_kernel_shapes_on_a_still_free_body(case):
    w, x, v, rng = _still_state()
    tri = _shape(case, rng)
    used = np.unique(tri)
    if case.startswith("strip_"):
        assert used.size == int(case[6:])
    if case == "fan_300":
        w[0] = 2.0
        assert (tri == 0).sum() == 300
    if case == "first_and_last":
        w[5] = 1.0
        assert np.nonzero((tri == 5).any(axis=1))[0].tolist() == [0, 99]
    g = SoftbodyGroup(_free_body(N, w), [0], substeps=4).Start()
    try:
        g.set_render_triangles(tri)
        want = _check(g, x, v, w, tri, case, **ALL)
        changed = (bits(want) != bits(v)).any(axis=1)
        assert changed.any() and not changed[np.setdiff1d(np.arange(N), used)].any() and not changed[w == 0].any()
        if case == "repeated_vertex":
            assert not changed[11] and changed[[3, 9, 20, 40]].all() == bool((w[[3, 9, 20, 40]] > 0).all())
        # a second call runs on the velocities the first one left
        again = want.copy()
        surface_force_ref.apply(x, again, w, tri, wind=(0, 0, 0), normal=1.0, tangential=1.0, dt=0.25)
        g.apply_surface_forces(normal=1.0, tangential=1.0, dt=0.25)
        assert np.array_equal(bits(g.get_velocities()), bits(again)), f"{case}: still-air drag on top"
    finally:
        g.OnDestroy()


# ---- 2. the float range -------------------------------------------------------------------------------------------------------------------------

FORCES = {"normal": dict(wind=(1.5, -0.75, 2.25), normal=3.0, dt=0.02), "tangential": dict(wind=(1.5, -0.75, 2.25), tangential=0.75, dt=0.02),
          "pressure": dict(pressure=-1.25, dt=0.02), "all": ALL}


def _mesh_triangles(rng):
    """a strip through every particle plus random triangles: every particle is a corner, lists of many lengths"""
    i = np.arange(N - 2)
    return np.concatenate([np.stack([i, i + 1, i + 2], axis=1), rng.integers(0, N, size=(300, 3))])


def test_positions_and_velocities_scaled_across_the_float_range():
    # |f|^2 of a triangle of size s goes with s^4: the threshold 2^-96 is met around s = 2^-24, +inf around s = 2^32; far outside both
    # every triangle is skipped and every velocity keeps its bits
    w, x, v, rng = _still_state(5)
    tri = _mesh_triangles(rng)
    seen = set()
    g = SoftbodyGroup(_free_body(N, w), [0], substeps=4).Start()
    try:
        g.set_render_triangles(tri)
        for e in (-60, -30, -25, -24, -23, -10, 0, 10, 20, 30, 31, 32, 40):
            s = np.float32(2.0 ** e)
            xs, vs = x * s, v * s
            one = np.float32(1)
            skipped = np.array([surface_force_ref.triangle_impulse(xs, vs, t, np.zeros(3, np.float32), one, one, one) is None for t in tri[:N - 2:7]])      # of the strip
            for name, force in FORCES.items():
                want = _check(g, xs, vs, w, tri, f"scale 2^{e}, {name}", **force)
                changed = (bits(want) != bits(vs)).any(axis=1)
                seen.add("none" if not changed.any() else "some" if skipped.any() else "all")
                if e in (-60, 40):
                    assert not changed.any()
        assert seen == {"none", "some", "all"}, seen
    finally:
        g.OnDestroy()


def test_hostile_values_beside_healthy_triangles():
    """Subnormal, zero-area and overflowing triangles beside healthy ones; infinite and NaN velocities, -0, payloads; masses from 0 and
    subnormal to 2^100. Everything bit for bit: a component that comes out NaN is 0x7fc00000, and whoever is not written keeps its bits."""
    w, x, v, rng = _still_state(7)
    w[40:48] = [0, np.float32(1e-40), np.float32(2.0 ** 100), np.float32(2.0 ** -100), np.float32(1e-45), 0.5, 3, 0]
    i = np.arange(N)
    special = (i % 16 == 1) | (i % 16 == 4)
    for c in range(3):
        v.view(np.uint32)[special, c] = POOL[(3 * i + 5 * c + i // 5 + 1)[special] % POOL.size]
    x[64:72] *= np.float32(1e-20)                  # subnormal doubled areas among themselves, sliver triangles with the others
    x[72:76] = x[72]                               # coincident: zero areas
    x[80:84] *= np.float32(1e25)                   # overflowing areas
    x[90] = (np.nan, 1, 1); x[91] = (1, np.inf, 1); x[92] = (-np.inf, 0, 0)
    tri = np.concatenate([_mesh_triangles(rng), [[64, 65, 66], [66, 67, 68], [72, 73, 74], [72, 73, 200], [80, 81, 82], [81, 82, 300], [90, 10, 11], [91, 92, 12]]])
    g = SoftbodyGroup(_free_body(N, w), [0], substeps=4).Start()
    try:
        g.set_render_triangles(tri)
        for name, force in FORCES.items():
            want = _check(g, x, v, w, tri, f"hostile, {name}", **force)
            made = np.isnan(want) & (bits(want) != bits(v))
            assert (bits(want)[made] == 0x7fc00000).all()
            assert np.array_equal(bits(want[w == 0]), bits(v[w == 0]))
            if name == "all":
                assert made.any() and np.isinf(want).any() and (bits(want) != bits(v)).any(axis=1).sum() > N // 2
                assert (np.isnan(v) & (bits(want) == bits(v)) & (bits(v) != 0x7fc00000)).any(), "an unwritten NaN payload survives"
    finally:
        g.OnDestroy()


# ---- 3. ticking bodies ------------------------------------------------------------------------------------------------------------------------

def _cloth(nx=12):
    rng = np.random.default_rng(21)
    u = np.arange(nx) * 0.25
    V = np.stack(np.meshgrid(u, [0.0], u, indexing="ij"), axis=-1).reshape(-1, 3)
    V[:, 1] = 2.0 + 0.02 * rng.standard_normal(V.shape[0])
    idx = lambda a, b: a * nx + b       # noqa: E731
    T = np.array([t for a in range(nx - 1) for b in range(nx - 1)
                  for t in ((idx(a, b), idx(a + 1, b), idx(a + 1, b + 1)), (idx(a, b), idx(a + 1, b + 1), idx(a, b + 1)))])
    mesh, particle_of_vertex = from_triangle_mesh(V, T)
    pins = particle_of_vertex[[idx(0, 0), idx(0, nx - 1)]].astype(np.int32)
    return mesh, particle_of_vertex[T].astype(np.int32), pins


def _jelly(n=8):
    from readback_bench import surface_triangles
    mesh = jelly_cube(n)
    pins = np.nonzero(mesh.pos[:, 1] > mesh.pos[:, 1].max() - 0.5)[0].astype(np.int32)
    return mesh, np.asarray(surface_triangles(n), np.int32), pins


@pytest.mark.parametrize("compare", ["every_tick", "at_the_end"])
@pytest.mark.parametrize("case", ["cloth", "jelly"])
def test_a_call_before_every_tick_matches_the_oracle(case, compare, oracle_mod, monkeypatch):
    # compare = at_the_end: nothing between two ticks reads the state, so the call itself meets the held-back last kernel of the tick
    monkeypatch.setenv("SB_PEEK_MIN_TILES", "0")
    S = 6
    if case == "cloth":
        mesh, tri, pins = _cloth()
        kw = dict(substeps=S, damping=0.05, distance_compliance=1e-7, bending_compliance=1e-3)
        okw = dict(damping=0.05, compliance=(1e-7, 0.0, 1e-3))
        assert len(mesh.bend_rest) and 130 <= mesh.n <= 150 and tri.shape[0] == 2 * 11 * 11
    else:
        mesh, tri, pins = _jelly()
        kw = dict(substeps=S, damping=0.05)
        okw = dict(damping=0.05)
    mesh.inv_mass[pins] = 0.0
    rest = np.asarray(mesh.pos, np.float32).reshape(-1, 3)[pins].copy()
    g = SoftbodyGroup(mesh, [0], **kw).Start()
    try:
        g.set_render_triangles(tri)
        o = make_oracle(oracle_mod, mesh, build_plan(mesh), **okw)
        for t in range(6):
            force = dict(wind=(3.0 * np.cos(0.7 * t), 0.5 * t - 1.0, 2.0 * np.sin(0.7 * t)), normal=2.0, tangential=0.5, pressure=0.3 if case == "jelly" else 0.0, dt=0.02)
            target = rest + np.float32([0.02 * t, -0.01 * t, 0.015 * t])
            if t == 2:                    # a move of the pins before the call: the call lands it
                g.set_kinematic_positions(pins, target); o.set_kinematic_positions(pins, target)
            before = o.v.copy()
            g.apply_surface_forces(**force)
            surface_force_ref.apply(o.x, o.v, o.w, tri, **force)
            assert not np.array_equal(bits(before), bits(o.v)) and np.array_equal(bits(before[pins]), bits(o.v[pins]))
            if t == 4:                    # ... and after it: pending until the tick starts
                g.set_kinematic_positions(pins, target); o.set_kinematic_positions(pins, target)
            if compare == "every_tick" and t & 1:
                assert np.array_equal(bits(g.get_velocities()), bits(o.v)), f"velocities between the call and the step of tick {t}"
            g.step()
            o.step(0.02, S)
            if compare == "every_tick":
                assert np.array_equal(bits(g.get_positions()), bits(o.x)) and np.array_equal(bits(g.get_velocities()), bits(o.v)), f"{case}, after tick {t}"
        assert np.array_equal(bits(g.get_positions()), bits(o.x)) and np.array_equal(bits(g.get_velocities()), bits(o.v)), f"{case}, at the end"
        assert np.isfinite(o.x).all() and np.abs(o.v).max() > 0.05
    finally:
        g.OnDestroy()


# ---- 4. the tick boundary, device memory, a changed triangle list ---------------------------------------------------------------------------------

def _table_bytes(tri):
    m, parts = tri.shape[0], np.unique(tri).size
    return 4 * (3 * m + parts + (parts + 1) + 3 * m) + 16 * m


def test_the_step_after_a_call_starts_unfused_and_the_tables_follow_the_triangles(oracle_mod):
    from readback_bench import surface_triangles
    n, S = 12, 6
    mesh = jelly_cube(n)
    tri = np.asarray(surface_triangles(n), np.int32)
    g = SoftbodyGroup(mesh, [0], substeps=S).Start()
    try:
        stats = lambda: g.rank(0).stats()       # noqa: E731
        g.set_render_triangles(tri)
        d0 = stats()["device_bytes"]
        o = make_oracle(oracle_mod, mesh, build_plan(mesh))
        for _ in range(3):
            g.step(); o.step(0.02, S)
        st = stats()
        f0 = st["ticks_fused"]
        assert st["device_bytes"] == d0 and f0 >= 1, "nothing is allocated before the first call"
        g.apply_surface_forces(**ALL); surface_force_ref.apply(o.x, o.v, o.w, tri, **ALL)
        assert stats()["device_bytes"] == d0 + _table_bytes(tri)
        g.step(); o.step(0.02, S)
        assert stats()["ticks_fused"] == f0, "the step after a call starts unfused"
        g.step(); g.step(); o.step(0.02, S); o.step(0.02, S)
        assert stats()["ticks_fused"] == f0 + 2, "the steps after it fuse again"
        g.apply_surface_forces(**ALL); surface_force_ref.apply(o.x, o.v, o.w, tri, **ALL)
        assert stats()["device_bytes"] == d0 + _table_bytes(tri), "the tables are built once"
        # another list between two calls: the old tables go, the next call builds the new ones and uses them
        half = tri[::2][:, [0, 2, 1]].copy()
        g.set_render_triangles(half)
        assert stats()["device_bytes"] == d0
        g.apply_surface_forces(**ALL); surface_force_ref.apply(o.x, o.v, o.w, half, **ALL)
        assert stats()["device_bytes"] == d0 + _table_bytes(half)
        g.step(); o.step(0.02, S)
        assert np.array_equal(bits(g.get_positions()), bits(o.x)) and np.array_equal(bits(g.get_velocities()), bits(o.v))
    finally:
        g.OnDestroy()


def test_a_readback_with_normals_pending_across_the_call_is_delivered_unchanged():
    from readback_bench import surface_triangles
    n = 8
    tri = np.asarray(surface_triangles(n), np.int32)
    g = SoftbodyGroup(jelly_cube(n), [0], substeps=4).Start()
    try:
        g.set_render_triangles(tri)
        g.step(); g.step()
        g.readback_begin()
        p0, n0 = (a.copy() for a in g.readback_end(normals=True))
        g.readback_begin()
        g.apply_surface_forces(**ALL)
        p1, n1 = (a.copy() for a in g.readback_end(normals=True))
        assert np.array_equal(bits(p0), bits(p1)) and np.array_equal(bits(n0), bits(n1)) and np.abs(n0).max() > 0.5
        g.readback_begin()
        g.apply_surface_forces(**ALL)
        g.step()
        p2, n2 = (a.copy() for a in g.readback_end(normals=True))
        assert np.array_equal(bits(p0), bits(p2)) and np.array_equal(bits(n0), bits(n2)), "the snapshot was taken before the call and the step"
    finally:
        g.OnDestroy()


# ---- 5. errors and limits -----------------------------------------------------------------------------------------------------------------------

def test_every_refusal_on_a_live_group_leaves_the_state_alone():
    from embedding_ref import lattice_cell_cages
    from readback_bench import surface_triangles
    L = native.lib()
    fn = L.sb_group_apply_surface_forces
    good = make_surface_force(**ALL)
    d = native.SbDesc(); L.sb_desc_default(C.byref(d))
    early = C.c_void_p()
    assert L.sb_group_create(C.byref(d), None, 1, 0, C.byref(early)) == native.SB_OK
    try:
        assert fn(early, C.byref(good)) == native.SB_ERR_STATE and b"sb_group_finalize" in L.sb_last_error()
        assert fn(early, C.byref(bad_records()[0][0])) == native.SB_ERR_INVALID_ARG, "the record is checked first"
    finally:
        L.sb_group_destroy(early)
    n = 8
    mesh = jelly_cube(n)
    tri = np.asarray(surface_triangles(n), np.int32)
    w = np.asarray(mesh.inv_mass, np.float32)
    g = SoftbodyGroup(mesh, [0], substeps=4).Start()
    try:
        stats = lambda: g.rank(0).stats()       # noqa: E731
        g.step()
        assert fn(g._g, C.byref(good)) == native.SB_ERR_STATE and b"no render triangles" in L.sb_last_error()
        g.set_render_triangles(tri)
        g.step()
        x, v = g.get_positions().copy(), g.get_velocities().copy()
        g.step()                                              # a refused call does not complete the held-back tick either ...
        before = stats()
        for f, word in bad_records():
            assert fn(g._g, C.byref(f)) == native.SB_ERR_INVALID_ARG and word in L.sb_last_error().decode(), word
        assert fn(g._g, None) == native.SB_ERR_INVALID_ARG and fn(None, C.byref(good)) == native.SB_ERR_INVALID_ARG
        assert stats()["device_bytes"] == before["device_bytes"]
        g.step()
        assert stats()["ticks_fused"] == before["ticks_fused"] + 1, "... so the next tick still fuses"
        x2, v2 = g.get_positions().copy(), g.get_velocities().copy()
        assert not np.array_equal(bits(x), bits(x2))
        # an embedding in force: unsupported (render triangles and an embedding exclude each other), and no triangles at all: state
        g.set_render_triangles(np.zeros((0, 3), np.int32))
        assert fn(g._g, C.byref(good)) == native.SB_ERR_STATE
        rng = np.random.default_rng(5)
        cage = lattice_cell_cages(n, rng.integers(0, n - 1, size=(50, 3)), rng)
        g.set_render_embedding(cage, np.full((50, 4), 0.25, np.float32), np.array([[0, 1, 2]], np.int32))
        assert fn(g._g, C.byref(good)) == native.SB_ERR_UNSUPPORTED and b"embedding" in L.sb_last_error()
        g.set_render_embedding(None, None)
        for f, _ in bad_records()[:4]:
            assert fn(g._g, C.byref(f)) == native.SB_ERR_INVALID_ARG
        assert np.array_equal(bits(g.get_positions()), bits(x2)) and np.array_equal(bits(g.get_velocities()), bits(v2)), "a refused call changed the state"
        assert stats()["device_bytes"] == before["device_bytes"]
        g.set_render_triangles(tri)
        assert fn(g._g, C.byref(good)) == native.SB_OK
        want = v2.copy()
        surface_force_ref.apply(x2, want, w, tri, **ALL)
        assert np.array_equal(bits(g.get_positions()), bits(x2)) and np.array_equal(bits(g.get_velocities()), bits(want)) and not np.array_equal(bits(want), bits(v2))
    finally:
        g.OnDestroy()


@pytest.mark.parametrize("walk", [False, True])
def test_a_group_of_one_rank_gives_the_reference_in_both_host_models(walk, oracle_mod):
    mesh, tri, pins = _jelly()
    mesh.inv_mass[pins] = 0.0
    S = 4
    g = SoftbodyGroup(mesh, [0], substeps=S, walk=walk).Start()
    try:
        g.set_render_triangles(tri)
        o = make_oracle(oracle_mod, mesh, build_plan(mesh))
        for t in range(3):
            g.step(); o.step(0.02, S)
            g.apply_surface_forces(**ALL); surface_force_ref.apply(o.x, o.v, o.w, tri, **ALL)
        assert np.array_equal(bits(g.get_positions()), bits(o.x)) and np.array_equal(bits(g.get_velocities()), bits(o.v))
    finally:
        g.OnDestroy()


_GROUP_CASE_ENDED_ABNORMALLY = []


@pytest.mark.parametrize("host", ["threads", "walk"])
def test_a_group_of_two_ranks_is_unsupported_and_keeps_its_state(host):
    # two ranks of one process on one device, as tests/test_gpu_group.py runs them: a hardware queue per rank for the peer transport.
    # One subprocess under a timeout. 0 and 1 are the case's own exits (OK / MISMATCH); after any other exit or a timeout the other
    # host model's case is not started here.
    assert not _GROUP_CASE_ENDED_ABNORMALLY, f"not started: the case before ended abnormally ({_GROUP_CASE_ENDED_ABNORMALLY[0]})"
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16")
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "surface_force_group_case.py"), host], env=env, capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired:
        _GROUP_CASE_ENDED_ABNORMALLY.append(f"{host}: timeout")
        raise
    if out.returncode not in (0, 1):
        _GROUP_CASE_ENDED_ABNORMALLY.append(f"{host}: exit {out.returncode}")
    assert out.returncode == 0 and "SURFACE FORCE GROUP OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
