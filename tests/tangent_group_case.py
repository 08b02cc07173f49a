"""sb_group_set_render_uvs / sb_group_readback_get_tangents in a process of its own (tests/test_gpu_render_tangents.py starts it, the way
tests/test_gpu_render_embedding.py starts tests/embedding_group_case.py): two ranks of one process on one device over the peer transport.
Leg A: render triangles over the cube's surface, render-set-only. Leg B: an embedding whose cages straddle the rank boundary, triangles and
UVs over its render vertices. Tangents bit for bit the reference's (SPEC.md 6c) and a single solver's on the same mesh.
Prints `TANGENT GROUP OK ...` or `TANGENT GROUP MISMATCH leg ..., tick ..., vertex ...`.

usage: tangent_group_case.py <threads|walk>
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import oracle                                              # noqa: E402  (test infrastructure: the checker)
from embedding_ref import embedded_ref, lattice_cell_cages             # noqa: E402
from helpers import build_plan, make_oracle                            # noqa: E402
from readback_bench import surface_triangles                           # noqa: E402
from tangent_ref import bits, lattice_uvs, tangents_ref                # noqa: E402
from softbodyunity_amd import Softbody, SoftbodyGroup, native          # noqa: E402
from softbodyunity_amd.mesh import jelly_cube                          # noqa: E402


def first_difference(got, want):
    """'' when the arrays agree bit for bit, else the first row that differs"""
    if got.shape != want.shape:
        return f"shape {got.shape} for {want.shape}"
    bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
    return "" if bad.size == 0 else f"vertex {int(bad[0])} ({bad.size} differ)"


def run_leg(body, leg, ticks, o, tri, uv, cage=None, w=None):
    """ticks x (step, readback) on a Softbody or a SoftbodyGroup -> per-tick (positions, normals, tangents); o: oracle stepped alongside, or None"""
    why, got = [], []
    if leg == "A":
        body.set_render_triangles(tri); body.set_readback_render_set_only(True)
    else:
        body.set_render_embedding(cage, w, tri)
    body.set_render_uvs(uv)
    for t in range(ticks):
        body.step()
        body.readback_begin()
        pos, nrm, tan = (a.copy() for a in body.readback_end(normals=True, tangents=True))
        got.append((pos, nrm, tan))
        if o is None:
            continue
        o.step(0.02, body.substeps)
        if leg == "A":
            rows = body.render_set().copy()
            p_all = o.x
            want_p, want_n = p_all[rows], oracle.vertex_normals(p_all, tri)
            want_t = tangents_ref(p_all, want_n, tri, uv)[rows]
            want_n = want_n[rows]
            if not np.array_equal(rows, np.unique(tri)):
                why.append(f"leg A, tick {t}: render set")
        else:
            want_p = embedded_ref(o.x, cage, w)
            want_n = oracle.vertex_normals(want_p, tri)
            want_t = tangents_ref(want_p, want_n, tri, uv)
        for name, a, b in (("positions", pos, want_p), ("normals", nrm, want_n), ("tangents", tan, want_t)):
            d = first_difference(a, b)
            if d:
                why.append(f"leg {leg}, tick {t}, {name}: {d}")
    return got, why


def main(host):
    n, S, ticks, tile = 24, 6, 3, 64
    mesh = jelly_cube(n)
    tune = native.SbTuning(); native.lib().sb_tuning_default(C.byref(tune)); tune.peek_min_tiles = 0       # small launches peek too
    rng = np.random.default_rng(14)
    why = []
    tri_a, uv_a = surface_triangles(n), lattice_uvs(n)
    L = native.lib()
    g = SoftbodyGroup(mesh, [0, 0], substeps=S, tile_particles=tile, halo_transport=native.SB_TRANSPORT_PEER, walk=host == "walk", tuning=tune).Start()
    try:
        r0 = g.rank(0); r0.n = mesh.n            # (24^3 under the automatic partition: every rank numbers the whole mesh)
        owner = r0.owner().reshape(n, n, n)
        lo, hi = owner[:-1, :-1, :-1].copy(), owner[:-1, :-1, :-1].copy()
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    c = owner[dz:n - 1 + dz, dy:n - 1 + dy, dx:n - 1 + dx]
                    lo = np.minimum(lo, c); hi = np.maximum(hi, c)
        straddle = np.argwhere(lo != hi)[:, ::-1]      # (z, y, x) -> (x, y, z)
        interior = np.argwhere(lo == hi)[:, ::-1]
        if len(straddle) == 0:
            why.append("no cell straddles the rank boundary")
        cells = np.concatenate([straddle[rng.integers(0, max(len(straddle), 1), 350)], interior[rng.integers(0, len(interior), 350)]])
        cage = lattice_cell_cages(n, cells, rng)
        both = sum(len(set(owner.reshape(-1)[r])) == 2 for r in cage)
        m = cage.shape[0]
        w = rng.uniform(-0.5, 1.5, size=(m, 4)).astype(np.float32)
        tri_b = rng.integers(0, m, size=(1500, 3)).astype(np.int32)
        uv_b = rng.uniform(0, 1, size=(m, 2)).astype(np.float32)
        o = make_oracle(oracle, mesh, build_plan(mesh, tile_particles=tile))
        # the contract holds on a group as well
        fp = C.POINTER(C.c_float)
        q = fp()
        if L.sb_group_set_render_uvs(g._g, uv_a.ctypes.data_as(fp), mesh.n) != native.SB_ERR_STATE:
            why.append("UVs accepted without a render mode")
        got_a, y = run_leg(g, "A", ticks, o, tri_a, uv_a); why += y
        if L.sb_group_set_render_uvs(g._g, uv_a.ctypes.data_as(fp), mesh.n - 1) != native.SB_ERR_INVALID_ARG:
            why.append("wrong count accepted")
        bad = uv_a.copy(); bad[5, 0] = np.nan
        if L.sb_group_set_render_uvs(g._g, bad.ctypes.data_as(fp), mesh.n) != native.SB_ERR_INVALID_ARG:
            why.append("NaN UV accepted")
        g.readback_begin()
        if L.sb_group_set_render_uvs(g._g, uv_a.ctypes.data_as(fp), mesh.n) != native.SB_ERR_STATE:
            why.append("UVs accepted while a readback is pending")
        pos, nrm, tan = g.readback_end(normals=True, tangents=True)
        if first_difference(tan, got_a[-1][2]):
            why.append("leg A: refused calls changed the tangents")
        g.set_readback_render_set_only(False)
        g.set_render_triangles(np.zeros((0, 3), np.int32))       # (clears the UVs)
        g.readback_begin(); g.readback_end()
        if L.sb_group_readback_get_tangents(g._g, C.byref(q)) != native.SB_ERR_STATE:
            why.append("tangents delivered after the render mode was switched off")
        got_b, y = run_leg(g, "B", ticks, o, tri_b, uv_b, cage, w); why += y
        if not (np.array_equal(bits(g.get_positions()), bits(o.x)) and np.array_equal(bits(g.get_velocities()), bits(o.v))):
            why.append("final state")
    finally:
        g.OnDestroy()
    # ... and the single solver gives the same bits
    sb = Softbody(mesh, substeps=S, tile_particles=tile, tuning=tune).Start()
    try:
        one_a, _ = run_leg(sb, "A", ticks, None, tri_a, uv_a)
        sb.set_readback_render_set_only(False)
        sb.set_render_triangles(np.zeros((0, 3), np.int32))
        one_b, _ = run_leg(sb, "B", ticks, None, tri_b, uv_b, cage, w)
        for leg, grp, one in (("A", got_a, one_a), ("B", got_b, one_b)):
            for t in range(ticks):
                for name, a, b in zip(("positions", "normals", "tangents"), grp[t], one[t]):
                    d = first_difference(a, b)
                    if d:
                        why.append(f"leg {leg}, tick {t}, {name} against the single solver: {d}")
    finally:
        sb.OnDestroy()
    ok = not why
    print(("TANGENT GROUP OK" if ok else "TANGENT GROUP MISMATCH " + "; ".join(why[:12])), f"host={host} render_set={np.unique(tri_a).size} render_vertices={m} "
          f"cages_on_both_ranks={both}")
    return ok


if __name__ == "__main__":
    sys.exit(0 if main(sys.argv[1]) else 1)
