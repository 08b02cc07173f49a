"""Impulses between two ticks on the GPU (SPEC.md 2c; sb_apply_impulses and sb_group_apply_impulses). A tick is bit-identical to the CPU oracle
and an impulse is a closed-form float32 update of the velocities, so every comparison is bitwise: the oracle's `v` receives the same update
from tests/impulse_ref.py between its ticks."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import impulse_ref
from embedding_ref import lattice_cell_cages
from helpers import make_oracle
from impulse_ref import bits
from softbodyunity_amd import IMPULSE, Softbody, bunny_surrogate, impulse_explosion, impulse_hits, impulse_particles, jelly_cube, native
from softbodyunity_amd.mesh import SoftbodyMesh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

IP = C.POINTER(native.SbImpulse)


def _cat(*parts):
    return np.concatenate([np.atleast_1d(p) for p in parts])


def _raw(handle, items, count=None, fn=None):
    items = np.ascontiguousarray(items, IMPULSE)
    fn = fn or native.lib().sb_apply_impulses
    return fn(handle, items.ctypes.data_as(IP) if items.size else None, items.shape[0] if count is None else count)


def _same(sb, o, what):
    x, v = sb.get_positions(), sb.get_velocities()
    assert np.array_equal(bits(x), bits(o.x)), f"{what}: positions"
    assert np.array_equal(bits(v), bits(o.v)), f"{what}: velocities"


def _free_body(n, inv_mass=None):
    """n particles without constraints (the planner never sees the test's state: it arrives through sb_set_state)"""
    i = np.arange(n)
    rest = (np.stack([i % 8, (i // 8) % 8, i // 64], axis=1) * 0.5).astype(np.float32)
    w = np.ones(n, np.float32) if inv_mass is None else np.asarray(inv_mass, np.float32)
    return SoftbodyMesh(rest_pos=rest, pos=rest.copy(), vel=np.zeros((n, 3), np.float32), inv_mass=w,
                        dist_ij=np.zeros((0, 2), np.int32), dist_rest=np.zeros(0, np.float32))


# ---- 1. mixed batches against the oracle ----------------------------------------------------------------------------------------------------

def _mixed_batch(mesh, pins, t, rng):
    """PARTICLE items (one id three times, a pinned id, both modes) interleaved with RADIAL items (both falloffs, a negative strength, two in
    a row, one that covers the whole body, one that misses it)"""
    free = np.setdiff1d(np.arange(mesh.n), pins)
    a, b = int(free[(37 * t + 5) % free.size]), int(free[(91 * t + 11) % free.size])
    lo, hi = mesh.pos.min(axis=0), mesh.pos.max(axis=0)
    ext = float((hi - lo).max())
    mid = (lo + hi) / 2
    j = lambda: rng.uniform(-0.4, 0.4, size=3).astype(np.float32)      # noqa: E731
    c = lambda: (mid + rng.uniform(-0.4, 0.4, size=3) * ext).astype(np.float32)      # noqa: E731
    return _cat(impulse_particles([a], j()),
                impulse_explosion(c(), 0.45 * ext, 0.3, linear_falloff=True),
                impulse_particles([a, int(pins[t % pins.size])], [j(), j()], velocity_change=True),
                impulse_explosion(c(), 0.35 * ext, -0.25),
                impulse_explosion(c(), 0.5 * ext, 0.2, linear_falloff=True, velocity_change=True),      # (two RADIAL items in a row)
                impulse_particles([b, a, int(pins[(t + 3) % pins.size])], [j(), j(), j()]),
                impulse_explosion(mid.astype(np.float32), 4.0 * ext, 0.05, linear_falloff=True),        # covers the whole body
                impulse_explosion((mid + 10.0 * ext).astype(np.float32), 0.5 * ext, 5.0))               # misses the body


@pytest.mark.parametrize("compare", ["every_tick", "at_the_end"])
@pytest.mark.parametrize("peek_small", [False, True])
@pytest.mark.parametrize("case", ["cube", "cube_global_colours_only", "bunny"])
def test_mixed_batches_match_the_oracle(case, peek_small, compare, oracle_mod, monkeypatch):
    # compare = at_the_end: nothing between two ticks reads velocities, so the apply itself meets the held-back last kernel of the tick
    if peek_small:
        monkeypatch.setenv("SB_PEEK_MIN_TILES", "0")
    else:
        monkeypatch.delenv("SB_PEEK_MIN_TILES", raising=False)
    S = 6
    if case.startswith("cube"):
        mesh = jelly_cube(12)
        pins = np.nonzero(mesh.pos[:, 1] > mesh.pos[:, 1].max() - 0.5)[0].astype(np.int32)       # the top layer
        kw = dict(substeps=S, damping=0.05)
        if case.endswith("global_colours_only"):
            kw["tile_particles"] = -1
        okw = dict(damping=0.05)
    else:
        mesh = bunny_surrogate(target_verts=5000, seed=11)
        pins = np.argsort(mesh.pos[:, 0])[-40:].astype(np.int32)
        kw = dict(substeps=S, distance_compliance=1e-7, volume_compliance=1e-7, bending_compliance=1e-4,
                  ground_plane=(0, 1, 0, float(mesh.pos[:, 1].min()) - 0.05))
        okw = dict(compliance=(1e-7, 1e-7, 1e-4), ground_plane=kw["ground_plane"])
        assert len(mesh.dist_rest) and len(mesh.vol_rest) and len(mesh.bend_rest)
    mesh.inv_mass[pins] = 0.0
    rest = mesh.pos[pins].copy()
    rng = np.random.default_rng(7)
    sb = Softbody(mesh, **kw).Start()
    try:
        o = make_oracle(oracle_mod, mesh, sb.plan(), **okw)
        for t in range(6):
            batch = _mixed_batch(mesh, pins, t, rng)
            target = rest + np.float32([0.02 * t, -0.01 * t, 0.015 * t])
            if t == 2:                    # a move of the pins before the apply: the apply lands it
                sb.set_kinematic_positions(pins, target); o.set_kinematic_positions(pins, target)
            v_before = o.v.copy()
            sb.apply_impulses(batch)
            impulse_ref.apply(o.x, o.v, o.w, batch)
            assert not np.array_equal(bits(v_before), bits(o.v)) and np.array_equal(bits(v_before[pins]), bits(o.v[pins]))
            if t == 4:                    # ... and after it: pending until the tick starts
                sb.set_kinematic_positions(pins, target); o.set_kinematic_positions(pins, target)
            if t & 1:
                assert np.array_equal(bits(sb.get_positions()), bits(o.x)), f"positions between the apply and the step of tick {t}"
            sb.step()
            o.step(0.02, S)
            if compare == "every_tick":
                _same(sb, o, f"{case}, after tick {t}")
        _same(sb, o, f"{case}, at the end")
        assert np.abs(o.v).max() > 0.05
    finally:
        sb.OnDestroy()


# ---- 2. SURFACE items in every render mode ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["full", "render_set", "embedding"])
def test_hits_fed_straight_back_in_every_render_mode(mode, oracle_mod, monkeypatch):
    from raycast_ref import make_rays
    from readback_bench import surface_triangles
    monkeypatch.setenv("SB_PEEK_MIN_TILES", "0")
    n, S = 12, 6
    mesh = jelly_cube(n)
    pins = np.nonzero(mesh.pos[:, 1] > mesh.pos[:, 1].max() - 0.5)[0].astype(np.int32)           # a hit may land on a pinned vertex
    mesh.inv_mass[pins] = 0.0
    rng = np.random.default_rng(13)
    R = 40
    o3 = rng.normal(size=(R, 3)); o3 = 5.5 + 20.0 * o3 / np.linalg.norm(o3, axis=1, keepdims=True)
    target = rng.uniform(0.0, 11.0, size=(R, 3))
    target[::5] = 5.5 + 2.0 * (o3[::5] - 5.5)                                                     # every fifth ray points away from the body
    rays = make_rays(o3, target - o3, np.inf)
    J = rng.uniform(-0.5, 0.5, size=(R, 3)).astype(np.float32)
    tri = surface_triangles(n)
    cage = w4 = None
    if mode == "embedding":
        m = 600
        cage = lattice_cell_cages(n, rng.integers(0, n - 1, size=(m, 3)), rng)
        w4 = rng.uniform(-0.5, 1.5, size=(m, 4)).astype(np.float32)
        tri = rng.integers(0, m, size=(1500, 3)).astype(np.int32)
    sb = Softbody(mesh, substeps=S, damping=0.05).Start()
    try:
        if mode == "embedding":
            sb.set_render_embedding(cage, w4, tri)
        else:
            sb.set_render_triangles(tri)
            sb.set_readback_render_set_only(mode == "render_set")
        o = make_oracle(oracle_mod, mesh, sb.plan(), damping=0.05)
        on_pin = 0
        for t in range(4):
            sb.readback_begin(); sb.readback_end()
            hits = sb.raycast(rays)
            assert (hits["triangle"] >= 0).any() and (hits["triangle"] < 0).any()
            items = impulse_hits(hits, J, velocity_change=bool(t & 1))
            if mode != "embedding":
                on_pin += int(np.isin(tri[hits["triangle"][hits["triangle"] >= 0]], pins).sum())
            sb.apply_impulses(items)
            v_before = o.v.copy()
            impulse_ref.apply(o.x, o.v, o.w, items, tri=tri, cage=cage, w4=w4)
            assert not np.array_equal(bits(v_before), bits(o.v))
            assert np.array_equal(bits(sb.get_velocities()), bits(o.v)), f"{mode}: velocities after the apply of tick {t}"
            sb.step(); o.step(0.02, S)
            _same(sb, o, f"{mode}, after tick {t}")
        assert mode == "embedding" or on_pin > 0
    finally:
        sb.OnDestroy()


# ---- 3. the float range, without stepping ----------------------------------------------------------------------------------------------------

def test_the_float_range():
    """Everything bit for bit, NaN included: a component that comes out of an impulse's addition as NaN is the canonical quiet NaN
    0x7fc00000 (SPEC.md 2c), and a particle no item can reach (pinned, or at a NaN / infinite position and not named by a PARTICLE item)
    keeps its velocity's bits, NaN payloads and signalling NaNs included."""
    n = 64
    sub, tiny, huge = np.float32(1e-40), np.float32(1e-30), np.float32(1e30)
    w = np.ones(n, np.float32)
    w[8:16] = [0, sub, np.float32(2.0 ** 100), np.float32(2.0 ** -100), np.float32(1e-45), 0.5, 3, 0]
    w[40:44] = [np.float32(2.0 ** 100), sub, 0, 7]
    x = np.zeros((n, 3), np.float32)
    x[:, 0] = np.linspace(-6, 6, n); x[:, 1] = np.linspace(3, -3, n) ** 3 / 9; x[:, 2] = 0.25
    x[0] = (0, 0, 0)                                   # on the centre
    x[1] = (1e-20, 0, 0)                               # r2 subnormal
    x[2] = (0, -3e-23, 1e-23)                          # r2 subnormal, two components
    x[3] = (tiny, 0, 0)                                # r2 underflows to 0
    x[4] = (huge, 0, 0)                                # r2 overflows to +inf
    x[5] = (8, 0, 0)                                   # r2 == R2 exactly
    x[6] = (0, -8, 0)
    x[7] = (np.nextafter(np.float32(8), np.float32(9)), 0, 0)
    x[8:12] = [(1, 1, 1), (1e-20, 1e-20, 0), (2, -1, 0.5), (0, 0, 1e-19)]      # pinned, subnormal mass, 2^100, 2^-100
    x[16] = (np.nan, 1, 1); x[17] = (1, np.inf, 1); x[18] = (1, 1, -np.inf); x[19] = (np.inf, np.inf, np.inf)
    x[20] = np.float32([0, 0, 0]); x[20].view(np.uint32)[:] = (0x7fc01234, 0xffc00001, 0x7f800001)      # NaN payloads
    v = np.zeros((n, 3), np.float32)
    v[:, 0] = np.linspace(1, -1, n)
    v[16:21] = 1.5
    v[20].view(np.uint32)[:] = (0x7fc0beef, 0xffc0dead, 0x7fa00000)
    v[21] = (np.inf, -np.inf, sub); v[22] = (sub, -sub, np.float32(1e-45)); v[23] = (-np.inf, np.inf, 0)
    v[40] = (np.inf, -np.inf, 0)                       # 2^100 inverse mass: huge J overflows, inf - inf
    v[10] = (-np.inf, 3e38, -3e38)
    named = np.array([1, 3, 8, 9, 10, 12, 21, 22, 23, 40, 41, 42, 43, 40, 10, 63, 17], np.int32)
    Jn = np.zeros((named.size, 3), np.float32)
    Jn[:] = (3e38, -3e38, 1e-42)
    Jn[1::2] = (1e-42, 3e38, -1e-45)
    items = _cat(impulse_explosion((0, 0, 0), 8.0, 2.0),
                 impulse_explosion((0, 0, 0), 8.0, 2.0, linear_falloff=True),
                 impulse_particles(named, Jn),
                 impulse_explosion((0, 0, 0), np.inf, -1.5, linear_falloff=True),
                 impulse_explosion((0, 0, 0), np.inf, 3e38, velocity_change=True),
                 impulse_particles(named[::-1], Jn, velocity_change=True),
                 impulse_explosion((1e-20, 0, 0), 1e-19, 1e-3, linear_falloff=True),
                 impulse_explosion((0.5, -0.25, 0.125), 3.0, 1e-41),
                 impulse_explosion((0.5, -0.25, 0.125), 1e19, -3e38, linear_falloff=True, velocity_change=True))
    sb = Softbody(_free_body(n, w), substeps=4).Start()
    try:
        sb.set_state(x, v)
        assert np.array_equal(bits(sb.get_positions()), bits(x)) and np.array_equal(bits(sb.get_velocities()), bits(v)), "sb_set_state changed a value"
        want = v.copy()
        impulse_ref.apply(x, want, w, items)
        sb.apply_impulses(items)
        got = sb.get_velocities()
        assert np.array_equal(bits(sb.get_positions()), bits(x)), "positions never change"
    finally:
        sb.OnDestroy()
    unreachable = (w == 0) | (~np.isfinite(x).all(axis=1) & ~np.isin(np.arange(n), named))
    assert unreachable[[8, 15, 16, 18, 19, 20, 42]].all() and np.array_equal(bits(want[unreachable]), bits(v[unreachable]))
    made = np.isnan(want) & ~unreachable[:, None]
    print("float range: %d components NaN after an addition, %d components changed, %d particles unreachable" %
          (made.sum(), (bits(want) != bits(v)).sum(), unreachable.sum()))
    assert made.any() and (bits(want)[made] == 0x7fc00000).all() and np.isinf(want).any() and (bits(want) != bits(v)).sum() > 100
    first = v.copy()
    impulse_ref.apply(x, first, w, items[:2])             # the two explosions at the origin alone: who is reached
    assert first[1, 0] != v[1, 0] and first[2, 1] != v[2, 1] and first[5, 0] != v[5, 0] and first[6, 1] != v[6, 1], "a subnormal r2 and r2 == R2 are reached"
    assert np.array_equal(bits(first[[0, 3, 4, 7]]), bits(v[[0, 3, 4, 7]])), "the centre, r2 = 0, r2 = +inf and r2 just above R2 are not"
    bad = bits(got) != bits(want)
    assert not bad.any(), [(int(p), int(c), hex(bits(got)[p, c]), hex(bits(want)[p, c])) for p, c in np.argwhere(bad)[:10]]


# ---- 4. chunking and sizes ----------------------------------------------------------------------------------------------------------------

def _still_body():
    """a free body of 8^3 particles with a given state; nothing steps"""
    n = 512
    rng = np.random.default_rng(3)
    w = rng.choice(np.float32([0, 0.5, 1, 2, 3]), size=n).astype(np.float32)
    x = rng.uniform(-2, 2, size=(n, 3)).astype(np.float32)
    v = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    return n, w, x, v, rng


def test_37_radial_items_in_one_call_equal_37_calls_and_the_reference():
    n, w, x, v, rng = _still_body()
    items = _cat(*[impulse_explosion(rng.uniform(-2, 2, size=3), rng.uniform(0.5, 4), rng.uniform(-1, 1), linear_falloff=bool(k % 3 == 0), velocity_change=bool(k % 4 == 1))
                   for k in range(37)])
    want = v.copy()
    impulse_ref.apply(x, want, w, items)
    got = []
    for one_call in (True, False):
        sb = Softbody(_free_body(n, w), substeps=4).Start()
        try:
            sb.set_state(x, v)
            if one_call:
                sb.apply_impulses(items)
            else:
                for k in range(37):
                    sb.apply_impulses(items[k:k + 1])
            got.append(sb.get_velocities())
        finally:
            sb.OnDestroy()
    assert np.array_equal(bits(got[0]), bits(got[1])) and np.array_equal(bits(got[0]), bits(want))
    assert (bits(want) != bits(v)).any(axis=1).sum() > n // 2


def test_a_long_particle_list_and_the_table_ring():
    n, w, x, v, rng = _still_body()
    ids = rng.choice(n, size=300, replace=False).astype(np.int32)          # more distinct particles than one 256-lane workgroup
    named = ids[rng.integers(0, 300, size=5000)]
    named[1000:1400] = ids[7]                                               # a long run of one particle
    J = rng.uniform(-1, 1, size=(5000, 3)).astype(np.float32) * np.float32(10.0) ** rng.integers(-6, 6, size=(5000, 1)).astype(np.float32)
    items = impulse_particles(named, J)
    items["flags"] = rng.integers(0, 2, size=5000)
    want = v.copy()
    impulse_ref.apply(x, want, w, items)
    sb = Softbody(_free_body(n, w), substeps=4).Start()
    try:
        sb.set_state(x, v)
        sb.apply_impulses(items)
        assert np.array_equal(bits(sb.get_velocities()), bits(want)), "5 000 entries over 300 particles"
        # 12 calls in a row without a step: the ring of tables wraps; the lists grow and shrink, sparse and radial runs alternate inside a call
        for k in range(12):
            part = _cat(items[100 * k:100 * k + 30 * (k % 5 + 1)], impulse_explosion((0, 0, 0), 1.0 + 0.1 * k, 0.1), items[4000 + 10 * k:4000 + 50 * k])
            sb.apply_impulses(part)
            impulse_ref.apply(x, want, w, part)
        assert np.array_equal(bits(sb.get_velocities()), bits(want)), "12 calls in a row"
        # one call of nine sparse runs between RADIAL items: more runs than the ring has tables (a call takes one table, whatever it holds)
        many = _cat(*[part for k in range(9) for part in (items[50 * k:50 * k + 20 + k], impulse_explosion((0.1 * k, 0, 0), 1.5, 0.05, linear_falloff=bool(k & 1)))])
        sb.apply_impulses(many)
        impulse_ref.apply(x, want, w, many)
        assert np.array_equal(bits(sb.get_velocities()), bits(want)), "nine sparse runs in one call"
        assert np.array_equal(bits(sb.get_positions()), bits(x))
    finally:
        sb.OnDestroy()


# ---- 5. errors ------------------------------------------------------------------------------------------------------------------------------

def test_every_error_and_nothing_changes():
    from readback_bench import surface_triangles
    L = native.lib()
    mesh = jelly_cube(8)
    tri = surface_triangles(8)
    m = tri.shape[0]
    good = impulse_particles([3], (1, 2, 3))
    rad = impulse_explosion((1, 1, 1), 2.0, 1.0)[0]
    par = good[0]
    hit = np.zeros(1, [("triangle", np.int32), ("t", np.float32), ("u", np.float32), ("v", np.float32)])
    hit["triangle"], hit["u"], hit["v"] = 5, 0.25, 0.25
    sur = impulse_hits(hit, (1, 0, 0))[0]

    def edit(item, **fields):
        out = np.array([item], IMPULSE)
        for k, val in fields.items():
            out[k][0] = val
        return out
    nan, inf = np.nan, np.inf
    rows = [(edit(par, kind=3), "unknown kind"), (edit(par, kind=-1), "unknown kind"),
            (edit(par, flags=4), "unknown flag"), (edit(rad, flags=0x80000000), "unknown flag"),
            (edit(par, flags=2), "LINEAR_FALLOFF"), (edit(sur, flags=3), "LINEAR_FALLOFF"),
            (edit(par, reserved=(0, 1)), "reserved"), (edit(rad, reserved=(-1, 0)), "reserved"),
            (edit(par, index=-1), "particle index out of range"), (edit(par, index=mesh.n), "particle index out of range"),
            (edit(sur, index=-2), "triangle index out of range"), (edit(sur, index=m), "triangle index out of range"),
            (edit(par, vec=(nan, 0, 0)), "vec"), (edit(sur, vec=(0, inf, 0)), "vec"), (edit(rad, vec=(0, 0, -inf)), "vec"), (edit(sur, index=-1, vec=(0, nan, 0)), "vec"),
            (edit(sur, u=nan), "barycentric"), (edit(sur, v=-inf), "barycentric"),
            (edit(rad, radius=nan), "radius"), (edit(rad, radius=0.0), "radius"), (edit(rad, radius=-1.0), "radius"), (edit(rad, radius=-inf), "radius"),
            (edit(rad, strength=nan), "strength"), (edit(rad, strength=inf), "strength")]
    sb = Softbody(mesh, substeps=4)
    sb.Start()
    try:
        sb.set_render_triangles(tri)
        sb.step()
        before = sb.get_velocities().copy()
        pos = sb.get_positions().copy()
        for bad, msg in rows:
            rc = _raw(sb._h, _cat(good, rad, bad, good))
            err = L.sb_last_error().decode()
            assert rc == native.SB_ERR_INVALID_ARG and msg in err and "sb_apply_impulses: item 2" in err, (msg, rc, err)
        assert _raw(None, good) == native.SB_ERR_INVALID_ARG
        assert L.sb_apply_impulses(sb._h, None, 1) == native.SB_ERR_INVALID_ARG and _raw(sb._h, good, count=-1) == native.SB_ERR_INVALID_ARG
        assert np.array_equal(bits(sb.get_velocities()), bits(before)), "the valid items in front of a bad one were applied"
        # fields a kind does not use are not looked at; a skipped SURFACE item's (u, v) neither; count = 0 is fine (null items too)
        ok = _cat(edit(par, u=nan, v=inf, radius=-1, strength=nan), edit(rad, index=-7, u=nan, v=nan), edit(sur, index=-1, u=nan, v=inf, radius=nan, strength=inf))
        assert _raw(sb._h, ok) == native.SB_OK
        assert L.sb_apply_impulses(sb._h, None, 0) == native.SB_OK and _raw(sb._h, good, count=0) == native.SB_OK
        want = before.copy()
        impulse_ref.apply(pos, want, np.asarray(mesh.inv_mass, np.float32), ok, tri=tri)
        assert np.array_equal(bits(sb.get_velocities()), bits(want)) and not np.array_equal(bits(want), bits(before))
        # SURFACE with no triangle list in force: none at all, an embedding without triangles
        sb.set_render_triangles(np.zeros((0, 3), np.int32))
        assert _raw(sb._h, _cat(good, sur)) == native.SB_ERR_STATE and "no triangle list is in force" in L.sb_last_error().decode()
        assert _raw(sb._h, _cat(good, edit(sur, index=-1))) == native.SB_ERR_STATE
        rng = np.random.default_rng(5)
        cage = lattice_cell_cages(8, rng.integers(0, 7, size=(50, 3)), rng)
        w4 = np.full((50, 4), 0.25, np.float32)
        sb.set_render_embedding(cage, w4)
        assert _raw(sb._h, _cat(good, sur)) == native.SB_ERR_STATE
        sb.set_render_embedding(cage, w4, np.array([[0, 1, 2]], np.int32))
        assert _raw(sb._h, edit(sur, index=1)) == native.SB_ERR_INVALID_ARG and _raw(sb._h, edit(sur, index=0)) == native.SB_OK
        impulse_ref.apply(pos, want, np.asarray(mesh.inv_mass, np.float32), edit(sur, index=0), tri=np.array([[0, 1, 2]]), cage=cage, w4=w4)
        assert np.array_equal(bits(sb.get_velocities()), bits(want))
        assert np.array_equal(bits(sb.get_positions()), bits(pos))
    finally:
        sb.OnDestroy()
    # before sb_finalize
    d = native.SbDesc(); L.sb_desc_default(C.byref(d))
    h = C.c_void_p()
    native.check(L.sb_create(C.byref(d), C.byref(h)))
    try:
        assert _raw(h, good) == native.SB_ERR_STATE and "before sb_finalize" in L.sb_last_error().decode()
    finally:
        L.sb_destroy(h)


# ---- 6. stats -------------------------------------------------------------------------------------------------------------------------------

def test_nothing_is_allocated_before_the_first_apply_and_the_next_step_starts_unfused():
    sb = Softbody(jelly_cube(12), substeps=6).Start()
    try:
        d0 = sb.stats()["device_bytes"]
        for _ in range(3):
            sb.step()
        st = sb.stats()
        f0 = st["ticks_fused"]
        assert st["device_bytes"] == d0 and f0 >= 1, st
        sb.apply_impulses(_cat(impulse_particles([5, 5, 9], (0, 1, 0)), impulse_explosion((5, 5, 5), 3.0, 1.0)))
        sb.step()
        assert sb.stats()["ticks_fused"] == f0, "the step after an apply starts unfused"
        sb.step(); sb.step()
        st = sb.stats()
        assert st["ticks_fused"] == f0 + 2, "the steps after it fuse again"
        assert st["device_bytes"] == d0, "the tables are pinned host memory: the device holds nothing more"
    finally:
        sb.OnDestroy()


# ---- 7. hosted ranks --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [2, 8])
def test_every_rank_applies_what_it_owns(world, oracle_mod):
    from hosted import HostedRanks
    from readback_bench import surface_triangles
    L = native.lib()
    mesh = jelly_cube(16)
    pins = np.nonzero(mesh.pos[:, 1] > mesh.pos[:, 1].max() - 0.5)[0].astype(np.int32)
    mesh.inv_mass[pins] = 0.0
    rng = np.random.default_rng(17)
    with HostedRanks(mesh, world, 6, tile_particles=64, damping=0.05) as H:
        o = make_oracle(oracle_mod, mesh, H.ranks[0].plan(), damping=0.05)
        owners = H.ranks[0].owner()
        assert len(np.unique(owners)) == world
        for t in range(3):
            batch = _mixed_batch(mesh, pins, t, rng)
            spread = impulse_particles(rng.integers(0, mesh.n, size=64), rng.uniform(-0.3, 0.3, size=(64, 3)))       # entries on every rank
            batch = _cat(batch[:5], spread, batch[5:])
            assert len(np.unique(owners[batch["index"][batch["kind"] == 0]])) == world
            for sb in H.ranks:
                sb.apply_impulses(batch)
            impulse_ref.apply(o.x, o.v, o.w, batch)
            H.tick(); o.step(0.02, 6)
            x, v, _ = H.merged_state()
            assert np.array_equal(bits(x), bits(o.x)) and np.array_equal(bits(v), bits(o.v)), f"world {world}, tick {t}"
        # a SURFACE item on a rank: unsupported, nothing changes
        hit = np.zeros(1, [("triangle", np.int32), ("t", np.float32), ("u", np.float32), ("v", np.float32)])
        hit["u"] = hit["v"] = 0.25
        for sb in H.ranks:
            sb.set_render_triangles(surface_triangles(16))
            rc = _raw(sb._h, _cat(batch[:3], impulse_hits(hit, (1, 0, 0))))
            assert rc == native.SB_ERR_UNSUPPORTED and "sb_group_apply_impulses" in L.sb_last_error().decode()
        x, v, _ = H.merged_state()
        assert np.array_equal(bits(x), bits(o.x)) and np.array_equal(bits(v), bits(o.v))


# ---- 8. group -------------------------------------------------------------------------------------------------------------------------------

_GROUP_CASE_ENDED_ABNORMALLY = []


@pytest.mark.parametrize("host", ["threads", "walk"])
def test_a_group_applies_impulses_in_whole_mesh_numbering(host):
    # two ranks of one process on one device, as tests/test_gpu_group.py runs them: a hardware queue per rank for the peer transport.
    # One subprocess under a timeout. 0 and 1 are the case's own exits (OK / MISMATCH); after any other exit or a timeout the other
    # host model's case is not started here.
    assert not _GROUP_CASE_ENDED_ABNORMALLY, f"not started: the case before ended abnormally ({_GROUP_CASE_ENDED_ABNORMALLY[0]})"
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16")
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "impulse_group_case.py"), host], env=env, capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired:
        _GROUP_CASE_ENDED_ABNORMALLY.append(f"{host}: timeout")
        raise
    if out.returncode not in (0, 1):
        _GROUP_CASE_ENDED_ABNORMALLY.append(f"{host}: exit {out.returncode}")
    assert out.returncode == 0 and "IMPULSE GROUP OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
