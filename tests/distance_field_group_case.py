"""sb_group_set_distance_field / sb_group_collide_distance_field in a process of their own (tests/test_gpu_distance_field.py starts it, the
way tests/test_gpu_heightfield.py starts tests/heightfield_group_case.py): ranks of one process on one device over the peer transport.
Three calls -- a sampled sphere rising and turning through the cuts between the ranks' blocks, the same slot at a second pose, a plane
field in another slot -- between the ticks of a 24^3 cube with a pinned top layer -- under the automatic partition (every rank holds the
whole mesh), under SB_PARTITION_BLOCKS (ranks hold windows: every rank walks its ghosts too) and on four ranks -- bit for bit the oracle
with tests/distance_field_ref.py between its ticks (SPEC.md 2i), and bit for bit a group of one device.
Prints `DISTANCE FIELD GROUP OK ...` or `DISTANCE FIELD GROUP MISMATCH ...`.

usage: distance_field_group_case.py <threads|walk>
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import distance_field_cases                                            # noqa: E402
import distance_field_ref                                              # noqa: E402
from oracle import oracle                                              # noqa: E402  (test infrastructure: the checker)
from helpers import build_plan, make_oracle                            # noqa: E402
from distance_field_ref import bits, pose_to_native, to_native         # noqa: E402
from softbodyunity_amd import SoftbodyGroup, native                    # noqa: E402
from softbodyunity_amd.mesh import jelly_cube                          # noqa: E402

N, S, TILE, DT = 24, 6, 64, 0.02


def plan_of_calls():
    """(slot, table, pose) of the three calls: each crosses the cuts between the ranks' blocks (the cube's middle planes)"""
    ball, side = distance_field_cases.sampled_sphere(9.0, n=25, thickness=4.0)
    y = -10.0 + 10.0 * np.arange(5)
    plane = distance_field_ref.make(np.broadcast_to((y - 2.5)[None, :, None], (4, 5, 6)), (10.0, 10.0, 14.0), 0.25, 0.8)      # phi = y - 2.5
    rise, ang = (0.0, 3.0, 0.0), (0.3, 0.8, -0.2)
    return [(0, ball, distance_field_cases.pose_about((11.5, -4.0, 11.5), side, (0.05, 0.3, 0.08, 1.0), lin=rise, ang=ang, friction=0.5, restitution=0.1)),
            (0, ball, distance_field_cases.pose_about((14.0, 1.0, 9.0), side, (0.3, -0.5, 0.2, 0.7), ang=ang, friction=0.2, restitution=0.0)),
            (2, plane, distance_field_ref.pose((-10.0, -10.0, -10.0), friction=0.0, restitution=0.6))]


def collide(groups, o, call):
    slot, df, ps = call
    for g in groups:
        g.set_distance_field(slot, *to_native(df))
        g.collide_distance_field(slot, pose_to_native(ps))
    return distance_field_ref.apply(o.x, o.v, o.w, df, ps)


def leg(name, host, devices, partition, why):
    mesh = jelly_cube(N)
    pins = np.nonzero(mesh.pos[:, 1] > mesh.pos[:, 1].max() - 0.5)[0].astype(np.int32)
    mesh.inv_mass[pins] = 0.0
    W = len(devices)
    tune = native.SbTuning(); native.lib().sb_tuning_default(C.byref(tune)); tune.peek_min_tiles = 0       # small launches peek too
    kw = dict(substeps=S, tile_particles=TILE, damping=0.05, tuning=tune)
    g = SoftbodyGroup(mesh, devices, halo_transport=native.SB_TRANSPORT_PEER, walk=host == "walk", partition=partition, **kw).Start()
    one = SoftbodyGroup(mesh, [0], **kw).Start()
    try:
        stats = lambda: [g.rank(r).stats() for r in range(W)]       # noqa: E731
        st0 = stats()
        held = {}                                       # slot -> bytes of the table the ranks hold there
        ghosts = sum(s["n_particles_local"] - s["n_particles_owned"] for s in st0)
        if ghosts <= 0 or sum(s["n_particles_owned"] for s in st0) != mesh.n:
            why.append(f"leg {name}: no ghosts, or the ranks do not own the mesh once")
        o = make_oracle(oracle, mesh, build_plan(mesh, tile_particles=TILE), damping=0.05)

        def same(what):
            for who, h in (("group", g), ("one device", one)):
                if not (np.array_equal(bits(h.get_positions()), bits(o.x)) and np.array_equal(bits(h.get_velocities()), bits(o.v))):
                    why.append(f"leg {name}: {who}: {what}")
        g.step(); one.step(); o.step(DT, S)
        calls = plan_of_calls()
        for t, call in enumerate(calls):
            before = (o.x.copy(), o.v.copy())
            d0 = [s["device_bytes"] for s in stats()]
            hit = collide((g, one), o, call)            # (the call meets every rank's held-back last kernel)
            slot, table = call[0], 4 * call[1]["s"].size
            if [s["device_bytes"] for s in stats()] != [d - held.get(slot, 0) + table for d in d0]:       # (around the calls alone: a state read may allocate its staging)
                why.append(f"leg {name}, call {t}: every rank holds one table per slot, and only the one set last")
            held[slot] = table
            if hit.sum() < 200 or np.array_equal(bits(before[1]), bits(o.v)) or not np.array_equal(bits(before[0][pins]), bits(o.x[pins])):
                why.append(f"leg {name}, call {t}: the reference changed too little ({hit.sum()} hits), or moved a pin")
            if t == 1:
                same("state right after the call")
            g.step(); one.step(); o.step(DT, S)
            same(f"state after the tick behind call {t}")
        # steps without a call fuse again on every rank; a set and a clear change nothing of that; with nothing set in the slot a call does
        # nothing; the step after a call starts unfused on every rank
        g.step(); o.step(DT, S)
        f0 = [s["ticks_fused"] for s in stats()]
        d0 = [s["device_bytes"] - sum(held.values()) for s in stats()]
        g.step(); g.set_distance_field(1, *to_native(calls[2][1])); g.step()
        for slot in (0, 1, 2):
            g.clear_distance_field(slot)
        g.collide_distance_field(1, pose_to_native(calls[2][2])); g.step()
        o.step(DT, S); o.step(DT, S); o.step(DT, S)
        f1 = [s["ticks_fused"] for s in stats()]
        if not all(b == a + 3 for a, b in zip(f0, f1)):
            why.append(f"leg {name}: ticks_fused across a set, the clears and a call with nothing set: {f0} -> {f1}")
        if [s["device_bytes"] for s in stats()] != d0:
            why.append(f"leg {name}: device bytes after the clears")
        collide((g,), o, calls[0])
        g.step(); o.step(DT, S)
        f2 = [s["ticks_fused"] for s in stats()]
        if f2 != f1:
            why.append(f"leg {name}: the step after a call fused: {f1} -> {f2}")
        g.step(); o.step(DT, S)
        f3 = [s["ticks_fused"] for s in stats()]
        if not all(b == a + 1 for a, b in zip(f2, f3)):
            why.append(f"leg {name}: the second step after a call did not fuse: {f2} -> {f3}")
        if not (np.array_equal(bits(g.get_positions()), bits(o.x)) and np.array_equal(bits(g.get_velocities()), bits(o.v))):
            why.append(f"leg {name}: final state")
        if not np.isfinite(o.x).all():
            why.append(f"leg {name}: the oracle's state is not finite")
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
    print(("DISTANCE FIELD GROUP OK" if ok else "DISTANCE FIELD GROUP MISMATCH " + "; ".join(why[:12])), f"host={host} ghosts={ghosts}")
    return ok


if __name__ == "__main__":
    sys.exit(0 if main(sys.argv[1]) else 1)
