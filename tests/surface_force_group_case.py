"""sb_group_apply_surface_forces on a group of two ranks, in a process of its own (tests/test_gpu_surface_forces.py starts it, the way
tests/test_gpu_placement.py starts tests/placement_group_case.py): two ranks of one process on one device over the peer transport.
A partitioned body is a deliberate limit of SPEC.md 2e: the call returns SB_ERR_UNSUPPORTED on every tick state, allocates nothing,
leaves every bit of the state and the tick's held-back last kernel alone -- the ticks around it stay bit for bit the oracle's and keep
fusing. Prints `SURFACE FORCE GROUP OK ...` or `SURFACE FORCE GROUP MISMATCH ...`.

usage: surface_force_group_case.py <threads|walk>
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import oracle                                                  # noqa: E402  (test infrastructure: the checker)
from helpers import build_plan, make_oracle                                # noqa: E402
from readback_bench import surface_triangles                               # noqa: E402
from softbodyunity_amd import SoftbodyGroup, make_surface_force, native    # noqa: E402
from softbodyunity_amd.mesh import jelly_cube                              # noqa: E402
from surface_force_ref import bits                                         # noqa: E402


def main(host):
    why = []
    n, S, tile = 16, 6, 64
    L = native.lib()
    mesh = jelly_cube(n)
    tri = np.asarray(surface_triangles(n), np.int32)
    force = make_surface_force(wind=(1.5, -0.75, 2.25), normal=3.0, tangential=0.75, pressure=-1.25, dt=0.02)
    g = SoftbodyGroup(mesh, [0, 0], halo_transport=native.SB_TRANSPORT_PEER, walk=host == "walk", substeps=S, tile_particles=tile, damping=0.05).Start()
    try:
        stats = lambda: [g.rank(r).stats() for r in range(2)]       # noqa: E731
        if sum(s["n_particles_owned"] for s in stats()) != mesh.n or min(s["n_particles_owned"] for s in stats()) == 0:
            why.append("the two ranks do not share the mesh")
        o = make_oracle(oracle, mesh, build_plan(mesh, tile_particles=tile), damping=0.05)

        def refused(what):
            rc = L.sb_group_apply_surface_forces(g._g, C.byref(force))
            if rc != native.SB_ERR_UNSUPPORTED or b"more than one rank" not in L.sb_last_error():
                why.append(f"{what}: returned {rc}: {L.sb_last_error().decode()}")
        g.set_render_triangles(tri)
        d0 = [s["device_bytes"] for s in stats()]
        refused("before the first tick")
        for t in range(4):
            g.step(); o.step(0.02, S)
            refused(f"after tick {t}")
        f0 = [s["ticks_fused"] for s in stats()]
        g.step(); o.step(0.02, S)
        f1 = [s["ticks_fused"] for s in stats()]
        if not all(b == a + 1 for a, b in zip(f0, f1)):
            why.append(f"the step after a refused call did not fuse: {f0} -> {f1}")
        if [s["device_bytes"] for s in stats()] != d0:
            why.append("a refused call allocated device memory")
        if not (np.array_equal(bits(g.get_positions()), bits(o.x)) and np.array_equal(bits(g.get_velocities()), bits(o.v))):
            why.append("the state differs from the oracle's")
        refused("after the state was read")
        if not np.array_equal(bits(g.get_velocities()), bits(o.v)):
            why.append("a refused call changed a velocity")
    finally:
        g.OnDestroy()
    ok = not why
    print(("SURFACE FORCE GROUP OK" if ok else "SURFACE FORCE GROUP MISMATCH " + "; ".join(why[:12])), f"host={host}")
    return ok


if __name__ == "__main__":
    sys.exit(0 if main(sys.argv[1]) else 1)
