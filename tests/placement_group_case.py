"""sb_group_place in a process of its own (tests/test_gpu_placement.py starts it, the way tests/test_gpu_impulses.py starts
tests/impulse_group_case.py): ranks of one process on one device over the peer transport. A move, a FROM_REFERENCE respawn and a
KEEP_PINNED move between the ticks of a 24^3 cube with a pinned top layer -- under the automatic partition (every rank holds the whole
mesh), under SB_PARTITION_BLOCKS (ranks hold windows: the ghosts' reference poses come from the window) and on four ranks -- bit for bit
the oracle with tests/placement_ref.py between its ticks (SPEC.md 2d), and bit for bit a group of one device.
Prints `PLACEMENT GROUP OK ...` or `PLACEMENT GROUP MISMATCH ...`.

usage: placement_group_case.py <threads|walk>
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import placement_ref                                                   # noqa: E402
from oracle import oracle                                              # noqa: E402  (test infrastructure: the checker)
from helpers import build_plan, make_oracle                            # noqa: E402
from placement_ref import FROM_REFERENCE, KEEP_PINNED, bits            # noqa: E402
from softbodyunity_amd import SoftbodyGroup, make_placement, native    # noqa: E402
from softbodyunity_amd.mesh import jelly_cube                          # noqa: E402


def place(groups, o, q, kw, flags):
    p = make_placement(kw.get("m"), kw.get("frm", (0, 0, 0)), kw.get("to", (0, 0, 0)), kw.get("lin", (0, 0, 0)), kw.get("ang", (0, 0, 0)))
    p.flags = flags
    for g in groups:
        g.place(p)
    placement_ref.apply(o.x, o.v, o.w, q, flags=flags, **kw)


def leg(name, host, devices, partition, why):
    n, S, tile = 24, 6, 64
    mesh = jelly_cube(n)
    pins = np.nonzero(mesh.pos[:, 1] > mesh.pos[:, 1].max() - 0.5)[0].astype(np.int32)
    mesh.inv_mass[pins] = 0.0
    q = np.ascontiguousarray(mesh.rest_pos if mesh.rest_pos is not None else mesh.pos, np.float32).reshape(-1, 3).copy()      # the reference pose
    W = len(devices)
    tune = native.SbTuning(); native.lib().sb_tuning_default(C.byref(tune)); tune.peek_min_tiles = 0       # small launches peek too
    kw = dict(substeps=S, tile_particles=tile, damping=0.05, tuning=tune)
    g = SoftbodyGroup(mesh, devices, halo_transport=native.SB_TRANSPORT_PEER, walk=host == "walk", partition=partition, **kw).Start()
    one = SoftbodyGroup(mesh, [0], **kw).Start()
    try:
        stats = lambda: [g.rank(r).stats() for r in range(W)]       # noqa: E731
        st0 = stats()
        ghosts = sum(s["n_particles_local"] - s["n_particles_owned"] for s in st0)
        if ghosts <= 0 or sum(s["n_particles_owned"] for s in st0) != mesh.n:
            why.append(f"leg {name}: no ghosts, or the ranks do not own the mesh once")
        o = make_oracle(oracle, mesh, build_plan(mesh, tile_particles=tile), damping=0.05)

        def same(what):
            for who, h in (("group", g), ("one device", one)):
                if not (np.array_equal(bits(h.get_positions()), bits(o.x)) and np.array_equal(bits(h.get_velocities()), bits(o.v))):
                    why.append(f"leg {name}: {who}: {what}")
        mid = np.float32([(n - 1) / 2] * 3)
        plan = [(dict(m=placement_ref.rotation((0.3, -0.2, 0.1, 0.9)), frm=mid, to=mid + np.float32([2.0, 0.5, -1.0])), 0),
                (dict(m=placement_ref.rotation((-0.1, 0.4, 0.2, 0.85)), frm=mid, to=mid + np.float32([-3.0, 1.0, 0.5]), lin=(0.2, 0.0, -0.1), ang=(0.0, 0.3, 0.1)), FROM_REFERENCE),
                (dict(m=placement_ref.rotation((0.01, 0.02, -0.01, 1.0)), frm=mid + np.float32([-3.0, 1.0, 0.5]), to=mid + np.float32([-2.97, 1.0, 0.52])), KEEP_PINNED)]
        g.step(); one.step(); o.step(0.02, S)
        for t, (pkw, flags) in enumerate(plan):
            before = o.x.copy()
            d0 = [s["device_bytes"] for s in stats()]
            place((g, one), o, q, pkw, flags)           # (the place meets every rank's held-back last kernel)
            if np.array_equal(bits(before), bits(o.x)) or (flags & KEEP_PINNED and not np.array_equal(bits(before[pins]), bits(o.x[pins]))):
                why.append(f"leg {name}, placement {t}: the reference changed nothing, or moved a kept pin")
            grown = [s["device_bytes"] - d for s, d in zip(stats(), d0)]
            if grown != [12 * s["n_particles_local"] if t == 1 else 0 for s in st0]:       # the first FROM_REFERENCE: every local particle's pose
                why.append(f"leg {name}, placement {t}: device bytes grew by {grown}")
            if t == 1:
                same("state right after the respawn")
            g.step(); one.step(); o.step(0.02, S)
            same(f"state after the tick behind placement {t}")
        # steps without a place fuse again on every rank; the step after a place starts unfused on every rank
        g.step(); o.step(0.02, S)
        f0 = [s["ticks_fused"] for s in stats()]
        g.step(); g.step(); o.step(0.02, S); o.step(0.02, S)
        f1 = [s["ticks_fused"] for s in stats()]
        if not all(b == a + 2 for a, b in zip(f0, f1)):
            why.append(f"leg {name}: ticks_fused without a place: {f0} -> {f1}")
        place((g,), o, q, dict(to=(0.5, 0.0, 0.25)), 0)
        g.step(); o.step(0.02, S)
        f2 = [s["ticks_fused"] for s in stats()]
        if f2 != f1:
            why.append(f"leg {name}: the step after a place fused: {f1} -> {f2}")
        g.step(); o.step(0.02, S)
        f3 = [s["ticks_fused"] for s in stats()]
        if not all(b == a + 1 for a, b in zip(f2, f3)):
            why.append(f"leg {name}: the second step after a place did not fuse: {f2} -> {f3}")
        if not (np.array_equal(bits(g.get_positions()), bits(o.x)) and np.array_equal(bits(g.get_velocities()), bits(o.v))):
            why.append(f"leg {name}: final state")
        return ghosts
    finally:
        one.OnDestroy()
        g.OnDestroy()


def main(host):
    why = []
    ghosts = [leg("whole mesh on 2", host, [0, 0], native.SB_PARTITION_AUTO, why),
              leg("windows on 2", host, [0, 0], native.SB_PARTITION_BLOCKS, why),
              leg("whole mesh on 4", host, [0, 0, 0, 0], native.SB_PARTITION_AUTO, why)]
    ok = not why
    print(("PLACEMENT GROUP OK" if ok else "PLACEMENT GROUP MISMATCH " + "; ".join(why[:12])), f"host={host} ghosts={ghosts}")
    return ok


if __name__ == "__main__":
    sys.exit(0 if main(sys.argv[1]) else 1)
