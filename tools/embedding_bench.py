#!/usr/bin/env python3
"""What an embedded render mesh (SPEC.md 6b, sb_set_render_embedding) costs per tick, beside the render-set readback it replaces.

Two bodies: the 100 k tet surrogate with its boundary faces split into four (a visual mesh finer than the cage), and jelly_cube(256)
with a visual mesh of the same kind over its surface cells. Three legs each, same process, same box, readbacks pipelined one tick behind
as a renderer does:
  (a) no readback,  (b) render-set readback with normals every tick,  (c) embedded readback with normals every tick.
Timed with HIP events on the solver's stream (sb_profile_begin / sb_profile_end), legs interleaved and repeated, best and median of the
repeats reported, the box's clocks beside them. One JSON line; --out FILE also writes it there.

usage: embedding_bench.py [--bodies bunny,cube] [--cube-n 256] [--bunny-verts 100000] [--ticks 40] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def tet_boundary_faces(tets):
    """Boundary faces of a tet mesh (faces that belong to one tet only), wound outwards for positively oriented tets."""
    t = np.asarray(tets, np.int64).reshape(-1, 4)
    faces = np.concatenate([t[:, [1, 2, 3]], t[:, [0, 3, 2]], t[:, [0, 1, 3]], t[:, [0, 2, 1]]])
    key = np.sort(faces, axis=1)
    _, idx, cnt = np.unique(key, axis=0, return_index=True, return_counts=True)
    return faces[idx[cnt == 1]].astype(np.int32)


def subdivided_surface(nodes, faces):
    """A visual mesh finer than the cage: every triangle of `faces` (indices into nodes) split into four by its edge midpoints.
    -> (vertices float64 (m,3): the nodes the faces use, then one midpoint per edge; triangles int32 (4F,3) over those vertices)."""
    P = np.asarray(nodes, np.float64).reshape(-1, 3)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    used = np.unique(F)
    vid = np.full(P.shape[0], -1, np.int64); vid[used] = np.arange(used.size)
    e = np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]), axis=1)
    edges, inv = np.unique(e, axis=0, return_inverse=True)
    inv = inv.ravel()
    nf = F.shape[0]
    mab, mbc, mca = (used.size + inv[k * nf:(k + 1) * nf] for k in range(3))
    a, b, c = vid[F[:, 0]], vid[F[:, 1]], vid[F[:, 2]]
    tri = np.concatenate([np.stack([a, mab, mca], 1), np.stack([mab, b, mbc], 1), np.stack([mca, mbc, c], 1), np.stack([mab, mbc, mca], 1)])
    verts = np.concatenate([P[used], 0.5 * (P[edges[:, 0]] + P[edges[:, 1]])])
    return verts, tri.astype(np.int32)


def lattice_embedding(n, vertices, spacing=1.0):
    """Cages and weights of `vertices` (rest pose, inside the n^3 lattice's box) in jelly_cube(n): each vertex is bound to four corners
    of its lattice cell -- the cell's origin corner and its three axis neighbours, an affine frame: w = (1 - u - v - t, u, v, t)."""
    V = np.asarray(vertices, np.float64).reshape(-1, 3) / spacing
    cell = np.clip(np.floor(V).astype(np.int64), 0, n - 2)
    f = V - cell
    base = (cell[:, 2] * n + cell[:, 1]) * n + cell[:, 0]
    cage = np.stack([base, base + 1, base + n, base + n * n], axis=1).astype(np.int32)
    w = np.concatenate([1.0 - f.sum(axis=1, keepdims=True), f], axis=1).astype(np.float32)
    return cage, w


def _clocks():
    """What the amdgpu driver shows an ordinary user of device 0 right now: clock levels, power, temperatures (tools/clock_probe.py)."""
    import glob
    import clock_probe
    devs = sorted(d for d in glob.glob("/sys/class/drm/card*/device") if os.path.exists(os.path.join(d, "pp_dpm_sclk")) or glob.glob(os.path.join(d, "hwmon", "hwmon*")))
    own = clock_probe.own_card(devs)
    return {own: clock_probe.sample(own)} if own else {d: clock_probe.sample(d) for d in devs}


def _legs(mesh, tri_particles, cage, weights, tri_vertices, substeps, ticks, repeats, **kw):
    from softbodyunity_amd import Softbody

    def piped(sb, n_ticks, normals):
        for k in range(n_ticks):
            sb.step(); sb.readback_begin()
            if k:
                sb.readback_end(normals=normals)
        sb.readback_end(normals=normals)

    def plain(sb, n_ticks, normals):
        for _ in range(n_ticks):
            sb.step()

    legs = {}
    solvers = {}
    try:
        for name in ("a_no_readback", "b_render_set", "c_embedded"):
            sb = Softbody(mesh, substeps=substeps, **kw).Start()
            solvers[name] = sb
            if name == "b_render_set":
                sb.set_render_triangles(tri_particles); sb.set_readback_render_set_only(True)
            elif name == "c_embedded":
                sb.set_render_embedding(cage, weights, tri_vertices)
            run = plain if name == "a_no_readback" else piped
            run(sb, 5, True); sb.synchronize()          # warm-up: first launches, buffers, the peek's tile subset
            legs[name] = (sb, run, [])
        for _ in range(repeats):                         # interleaved: a drift of the box's clocks lands on every leg alike
            for name, (sb, run, ms) in legs.items():
                sb.profile_begin()
                run(sb, ticks, True)
                ms.append(sb.profile_end() / ticks)
        out = {}
        for name, (sb, run, ms) in legs.items():
            st = sb.stats()
            out[name] = {"ms_per_tick_best": min(ms), "ms_per_tick_median": float(np.median(ms)), "ms_per_tick_all": [round(v, 5) for v in ms],
                         "readback_peek_tiles": st["readback_peek_tiles"], "t0_tiles": st["n_tiles"][0], "ticks_fused": st["ticks_fused"]}
        return out
    finally:
        for sb in solvers.values():
            sb.OnDestroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", default="bunny,cube")
    ap.add_argument("--cube-n", type=int, default=256)
    ap.add_argument("--bunny-verts", type=int, default=100_000)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from softbodyunity_amd import bunny_surrogate, embed_vertices, jelly_cube
    from readback_bench import surface_triangles
    res = {"tool": "embedding_bench", "ticks": a.ticks, "repeats": a.repeats, "timing": "HIP events on the solver's stream, per tick", "clocks_before": _clocks()}
    for body in a.bodies.split(","):
        if body == "bunny":
            mesh = bunny_surrogate(target_verts=a.bunny_verts)
            faces = tet_boundary_faces(mesh.vol_ijkl)
            verts, tri_v = subdivided_surface(mesh.rest_pos, faces)
            cage, w = embed_vertices(mesh.rest_pos, mesh.vol_ijkl, verts)
            kw = dict(distance_compliance=1e-7, volume_compliance=1e-7, bending_compliance=1e-4)
            r = _legs(mesh, faces, cage, w, tri_v, 20, a.ticks, a.repeats, **kw)
        else:
            n = a.cube_n
            mesh = jelly_cube(n)
            faces = surface_triangles(n)
            verts, tri_v = subdivided_surface(mesh.rest_pos, faces)
            cage, w = lattice_embedding(n, verts)
            r = _legs(mesh, faces, cage, w, tri_v, 20, a.ticks, a.repeats)
        r.update(particles=int(mesh.n), render_set_particles=int(np.unique(faces).size), render_vertices=int(verts.shape[0]),
                 render_triangles=int(tri_v.shape[0]), cage_particles=int(np.unique(cage).size), substeps=20)
        res[body] = r
    res["clocks_after"] = _clocks()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
