"""sb_group_set_render_embedding in a process of its own (tests/test_gpu_render_embedding.py starts it, the way tests/test_gpu_group.py
starts tests/group_case.py): two ranks of one process on one device over the peer transport. Cages from lattice cells that straddle the
rank boundary and from interior ones, triangles over the render vertices: vertices and normals bit for bit the single solver's and the
reference's. Prints `EMBEDDING GROUP OK ...` or `EMBEDDING GROUP MISMATCH ...`.

usage: embedding_group_case.py <threads|walk>
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import oracle                                              # noqa: E402  (test infrastructure: the checker)
from embedding_ref import bits, embedded_ref, lattice_cell_cages       # noqa: E402
from helpers import build_plan, make_oracle                            # noqa: E402
from softbodyunity_amd import Softbody, SoftbodyGroup, native          # noqa: E402
from softbodyunity_amd.mesh import jelly_cube                          # noqa: E402


def main(host):
    n, S, ticks, tile = 24, 6, 4, 64
    mesh = jelly_cube(n)
    tune = native.SbTuning(); native.lib().sb_tuning_default(C.byref(tune)); tune.peek_min_tiles = 0       # small launches peek too
    rng = np.random.default_rng(12)
    why = []
    g = SoftbodyGroup(mesh, [0, 0], substeps=S, tile_particles=tile, halo_transport=native.SB_TRANSPORT_PEER, walk=host == "walk", tuning=tune).Start()
    try:
        r0 = g.rank(0); r0.n = mesh.n            # (24^3 under the automatic partition: every rank numbers the whole mesh)
        owner = r0.owner().reshape(n, n, n)
        # cells whose 8 corners belong to both ranks / to one rank
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
        cells = np.concatenate([straddle[rng.integers(0, max(len(straddle), 1), 400)], interior[rng.integers(0, len(interior), 400)]])
        cage = lattice_cell_cages(n, cells, rng)
        both = sum(len(set(owner.reshape(-1)[r])) == 2 for r in cage)
        m = cage.shape[0]
        w = rng.uniform(-0.5, 1.5, size=(m, 4)).astype(np.float32)
        tri = rng.integers(0, m, size=(1500, 3)).astype(np.int32)
        g.set_render_embedding(cage, w, tri)
        o = make_oracle(oracle, mesh, build_plan(mesh, tile_particles=tile))
        got = []
        for t in range(ticks):
            g.step(); o.step(0.02, S)
            g.readback_begin()
            pos, nrm = (a.copy() for a in g.readback_end(normals=True))
            got.append((pos, nrm))
            want = embedded_ref(o.x, cage, w)
            if pos.shape != (m, 3) or not np.array_equal(bits(pos), bits(want)):
                why.append(f"vertices of tick {t}")
            if not np.array_equal(bits(nrm), bits(oracle.vertex_normals(want, tri))):
                why.append(f"normals of tick {t}")
        if not (np.array_equal(bits(g.get_positions()), bits(o.x)) and np.array_equal(bits(g.get_velocities()), bits(o.v))):
            why.append("final state")
        st = [g.rank(r).stats() for r in range(2)]
        peeks = [s["readback_peeks"] for s in st]; peek_tiles = [s["readback_peek_tiles"] for s in st]; t0 = [s["n_tiles"][0] for s in st]
        if not all(p >= ticks for p in peeks) or not all(0 < a <= b for a, b in zip(peek_tiles, t0)):
            why.append(f"peeks {peeks}, peek tiles {peek_tiles} of {t0}")
        # the mode rules hold on a group as well
        L = native.lib()
        t3 = np.zeros((1, 3), np.int32)
        if L.sb_group_set_render_triangles(g._g, t3.ctypes.data_as(C.POINTER(C.c_int32)), 1) != native.SB_ERR_STATE:
            why.append("render triangles accepted beside an embedding")
        bad = w.copy(); bad[3, 0] = np.nan
        try:
            g.set_render_embedding(cage, bad, tri); why.append("NaN weight accepted")
        except native.SoftbodyError as e:
            if e.code != native.SB_ERR_INVALID_ARG:
                why.append("NaN weight: wrong error")
        g.set_render_embedding(None, None)
        g.readback_begin()
        if not np.array_equal(bits(g.readback_end()), bits(o.x)):
            why.append("particle readback after the embedding was switched off")
    finally:
        g.OnDestroy()
    # ... and the single solver gives the same bits
    sb = Softbody(mesh, substeps=S, tile_particles=tile, tuning=tune).Start()
    try:
        sb.set_render_embedding(cage, w, tri)
        for t in range(ticks):
            sb.step(); sb.readback_begin()
            pos, nrm = sb.readback_end(normals=True)
            if not (np.array_equal(bits(pos), bits(got[t][0])) and np.array_equal(bits(nrm), bits(got[t][1]))):
                why.append(f"single solver differs at tick {t}")
    finally:
        sb.OnDestroy()
    ok = not why
    print(("EMBEDDING GROUP OK" if ok else "EMBEDDING GROUP MISMATCH " + "; ".join(why)), f"host={host} render_vertices={m} cages_on_both_ranks={both} "
          f"peek_tiles={peek_tiles} of {t0}")
    return ok


if __name__ == "__main__":
    sys.exit(0 if main(sys.argv[1]) else 1)
