"""sb_group_apply_impulses in a process of its own (tests/test_gpu_impulses.py starts it, the way tests/test_gpu_raycast.py starts
tests/raycast_group_case.py): two ranks of one process on one device over the peer transport. PARTICLE, SURFACE and RADIAL items in the whole
mesh's numbering -- SURFACE against the render triangles and against an embedding whose cages straddle the rank boundary -- bit for bit the
oracle with tests/impulse_ref.py between its ticks (SPEC.md 2c), and bit for bit a single solver of the same mesh.
Prints `IMPULSE GROUP OK ...` or `IMPULSE GROUP MISMATCH ...`.

usage: impulse_group_case.py <threads|walk>
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))

import impulse_ref                                                      # noqa: E402
from oracle import oracle                                              # noqa: E402  (test infrastructure: the checker)
from embedding_ref import lattice_cell_cages                           # noqa: E402
from helpers import build_plan, make_oracle                            # noqa: E402
from impulse_ref import bits                                           # noqa: E402
from raycast_ref import make_rays                                      # noqa: E402
from readback_bench import surface_triangles                           # noqa: E402
from softbodyunity_amd import (IMPULSE, Softbody, SoftbodyGroup, impulse_explosion, impulse_hits, impulse_particles,  # noqa: E402
                               native)
from softbodyunity_amd.mesh import jelly_cube                          # noqa: E402

IP = C.POINTER(native.SbImpulse)


def main(host):
    n, S, ticks, tile = 24, 6, 2, 64
    mesh = jelly_cube(n)
    pins = np.nonzero(mesh.pos[:, 1] > mesh.pos[:, 1].max() - 0.5)[0].astype(np.int32)
    mesh.inv_mass[pins] = 0.0
    tune = native.SbTuning(); native.lib().sb_tuning_default(C.byref(tune)); tune.peek_min_tiles = 0       # small launches peek too
    rng = np.random.default_rng(41)
    why = []
    tri = surface_triangles(n)
    L = native.lib()
    R = 37
    o3 = rng.normal(size=(R, 3)); o3 = (n - 1) / 2 + 2.0 * n * o3 / np.linalg.norm(o3, axis=1, keepdims=True)
    target = rng.uniform(0.0, n - 1, size=(R, 3))
    target[::6] = (n - 1) / 2 + 2.0 * (o3[::6] - (n - 1) / 2)            # every sixth ray points away from the body
    rays = make_rays(o3, target - o3, np.inf)
    J = rng.uniform(-0.5, 0.5, size=(R, 3)).astype(np.float32)
    g = SoftbodyGroup(mesh, [0, 0], substeps=S, tile_particles=tile, damping=0.05, halo_transport=native.SB_TRANSPORT_PEER, walk=host == "walk", tuning=tune).Start()
    single = Softbody(mesh, substeps=S, tile_particles=tile, damping=0.05).Start()
    m = 0
    try:
        r0 = g.rank(0); r0.n = mesh.n            # (24^3 under the automatic partition: every rank numbers the whole mesh)
        owner = r0.owner()
        grid = owner.reshape(n, n, n)
        lo, hi = grid[:-1, :-1, :-1].copy(), grid[:-1, :-1, :-1].copy()
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    c = grid[dz:n - 1 + dz, dy:n - 1 + dy, dx:n - 1 + dx]
                    lo = np.minimum(lo, c); hi = np.maximum(hi, c)
        straddle = np.argwhere(lo != hi)[:, ::-1]      # (z, y, x) -> (x, y, z)
        interior = np.argwhere(lo == hi)[:, ::-1]
        if len(straddle) == 0:
            why.append("no cell straddles the rank boundary")
        cells = np.concatenate([straddle[rng.integers(0, max(len(straddle), 1), 350)], interior[rng.integers(0, len(interior), 350)]])
        cage = lattice_cell_cages(n, cells, rng)
        m = cage.shape[0]
        if not (owner[cage].min(axis=1) != owner[cage].max(axis=1)).any():
            why.append("no cage straddles the rank boundary")
        w4 = rng.uniform(-0.5, 1.5, size=(m, 4)).astype(np.float32)
        etri = rng.integers(0, m, size=(1500, 3)).astype(np.int32)
        o = make_oracle(oracle, mesh, build_plan(mesh, tile_particles=tile), damping=0.05)

        def raw(handle, items, count=None):
            items = np.ascontiguousarray(items, IMPULSE)
            return L.sb_group_apply_impulses(handle, items.ctypes.data_as(IP), items.shape[0] if count is None else count)
        some = impulse_particles([5], (1, 0, 0))
        miss = np.zeros(1, [("triangle", np.int32), ("t", np.float32), ("u", np.float32), ("v", np.float32)]); miss["triangle"] = -1
        if raw(None, some) != native.SB_ERR_INVALID_ARG or raw(g._g, some, -1) != native.SB_ERR_INVALID_ARG:
            why.append("null group or negative count accepted")
        if raw(g._g, np.concatenate([some, impulse_hits(miss, (1, 0, 0))])) != native.SB_ERR_STATE:
            why.append("a SURFACE item with no triangle list in force")
        bad = impulse_particles([mesh.n], (1, 0, 0))
        if raw(g._g, np.concatenate([some, bad])) != native.SB_ERR_INVALID_ARG or raw(g._g, some, 0) != native.SB_OK:
            why.append("an index out of range accepted, or count = 0 refused")
        if not np.array_equal(bits(g.get_velocities()), bits(o.v)):
            why.append("a refused call changed the velocities")
        mid = np.float32([(n - 1) / 2] * 3)

        def leg(name, tris, cg, wg):
            for t in range(ticks):
                g.readback_begin(); g.readback_end()
                hits = g.raycast(rays)
                if not ((hits["triangle"] >= 0).any() and (hits["triangle"] < 0).any()):
                    why.append(f"leg {name}, tick {t}: the rays all hit or all miss")
                ids = rng.integers(0, mesh.n, size=48).astype(np.int32)
                ids[5] = ids[9] = ids[0]
                if len(np.unique(owner[ids])) != 2:
                    why.append(f"leg {name}: the PARTICLE items sit on one rank")
                items = np.concatenate([impulse_particles(ids[:24], rng.uniform(-0.3, 0.3, size=(24, 3))),
                                        impulse_explosion(mid + rng.uniform(-6, 6, size=3).astype(np.float32), 9.0, 0.4, linear_falloff=True),
                                        impulse_hits(hits, J, velocity_change=bool(t & 1)),
                                        impulse_explosion(mid, 40.0, -0.1), impulse_explosion(mid, 5.0, 0.3, velocity_change=True),
                                        impulse_particles(ids[24:], rng.uniform(-0.3, 0.3, size=(24, 3)), velocity_change=True)])
                g.apply_impulses(items); single.apply_impulses(items)
                before = o.v.copy()
                impulse_ref.apply(o.x, o.v, o.w, items, tri=tris, cage=cg, w4=wg)
                if np.array_equal(bits(before), bits(o.v)):
                    why.append(f"leg {name}, tick {t}: the batch changed nothing")
                if t == 0 and not np.array_equal(bits(g.get_velocities()), bits(o.v)):
                    why.append(f"leg {name}: group velocities right after the apply")
                g.step(); single.step(); o.step(0.02, S)
                if not (np.array_equal(bits(g.get_positions()), bits(o.x)) and np.array_equal(bits(g.get_velocities()), bits(o.v))):
                    why.append(f"leg {name}, tick {t}: group state")
                if not (np.array_equal(bits(single.get_positions()), bits(o.x)) and np.array_equal(bits(single.get_velocities()), bits(o.v))):
                    why.append(f"leg {name}, tick {t}: single solver's state")
        g.set_render_triangles(tri); single.set_render_triangles(tri)
        leg("render triangles", tri, None, None)
        g.set_render_triangles(np.zeros((0, 3), np.int32)); single.set_render_triangles(np.zeros((0, 3), np.int32))
        g.set_render_embedding(cage, w4, etri); single.set_render_embedding(cage, w4, etri)
        leg("embedding", etri, cage, w4)
        # steps without an apply fuse again on every rank
        f0 = [g.rank(r).stats()["ticks_fused"] for r in (0, 1)]
        g.step(); g.step(); o.step(0.02, S); o.step(0.02, S)
        f1 = [g.rank(r).stats()["ticks_fused"] for r in (0, 1)]
        if not all(b > a for a, b in zip(f0, f1)):
            why.append(f"ticks_fused did not rise without an apply: {f0} -> {f1}")
        # an apply straight after a step meets every rank's held-back last kernel; the step after it starts unfused on every rank
        items = np.concatenate([impulse_explosion(mid, 7.0, 0.5, linear_falloff=True), impulse_particles(rng.integers(0, mesh.n, size=32), (0.1, -0.2, 0.3))])
        g.apply_impulses(items)
        impulse_ref.apply(o.x, o.v, o.w, items)
        g.step(); o.step(0.02, S)
        f2 = [g.rank(r).stats()["ticks_fused"] for r in (0, 1)]
        if f2 != f1:
            why.append(f"the step after an apply fused: {f1} -> {f2}")
        if not (np.array_equal(bits(g.get_positions()), bits(o.x)) and np.array_equal(bits(g.get_velocities()), bits(o.v))):
            why.append("final state")
    finally:
        single.OnDestroy()
        g.OnDestroy()
    ok = not why
    print(("IMPULSE GROUP OK" if ok else "IMPULSE GROUP MISMATCH " + "; ".join(why[:12])), f"host={host} render_vertices={m} rays={R}")
    return ok


if __name__ == "__main__":
    sys.exit(0 if main(sys.argv[1]) else 1)
