"""sb_group_collide in a process of its own (tests/test_gpu_colliders.py starts it, the way tests/test_gpu_placement.py starts
tests/placement_group_case.py): ranks of one process on one device over the peer transport. A rising, spinning sphere, a tilted box and a
list longer than two batches between the ticks of a 24^3 cube with a pinned top layer -- under the automatic partition (every rank holds
the whole mesh), under SB_PARTITION_BLOCKS (ranks hold windows: every rank walks its ghosts too) and on four ranks -- bit for bit the
oracle with tests/collider_ref.py between its ticks (SPEC.md 2f), and bit for bit a group of one device.
Prints `COLLIDER GROUP OK ...` or `COLLIDER GROUP MISMATCH ...`.

usage: collider_group_case.py <threads|walk>
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import collider_ref                                                    # noqa: E402
import placement_ref                                                   # noqa: E402
from oracle import oracle                                              # noqa: E402  (test infrastructure: the checker)
from helpers import build_plan, make_oracle                            # noqa: E402
from collider_ref import bits, to_native                               # noqa: E402
from softbodyunity_amd import SoftbodyGroup, native                    # noqa: E402
from softbodyunity_amd.mesh import jelly_cube                          # noqa: E402

N, S, TILE, DT = 24, 6, 64, 0.02


def plan_of_calls():
    """the lists of the three calls: the colliders cross the cuts between the ranks' blocks (the cube's middle planes)"""
    mid = np.float32([(N - 1) / 2] * 3)
    rng = np.random.default_rng(21)
    ball = collider_ref.sphere(mid + np.float32([0.3, -9.0, -0.2]), 6.0, lin=(0.5, 20.0, -0.25), ang=(0.0, 3.0, 1.0), friction=0.4, restitution=0.2)
    slab = collider_ref.box(mid + np.float32([1.0, -11.0, 0.5]), placement_ref.rotation((0.05, 0.0, 0.08, 1.0)), (14.0, 2.0, 14.0), friction=0.8, restitution=0.0)
    rod = collider_ref.capsule(mid + np.float32([-14.0, 2.0, 0.4]), mid + np.float32([14.0, 3.0, -0.6]), 2.5, lin=(0.0, -2.0, 0.0), friction=0.1, restitution=0.6)
    many = []
    for k in range(2 * 16 + 1):
        c = rng.uniform(2.0, N - 3.0, size=3).astype(np.float32)
        many.append(collider_ref.sphere(c, float(rng.uniform(1.0, 2.5)), lin=rng.uniform(-2, 2, size=3), friction=(0.0, 0.5)[k % 2], restitution=(1.0, 0.3, 0.0)[k % 3]))
    return [[ball, slab], [rod], many]


def collide(groups, o, cols):
    items = [to_native(c) for c in cols]
    for g in groups:
        g.collide(items)
    return collider_ref.apply(o.x, o.v, o.w, cols)


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
        ghosts = sum(s["n_particles_local"] - s["n_particles_owned"] for s in st0)
        if ghosts <= 0 or sum(s["n_particles_owned"] for s in st0) != mesh.n:
            why.append(f"leg {name}: no ghosts, or the ranks do not own the mesh once")
        o = make_oracle(oracle, mesh, build_plan(mesh, tile_particles=TILE), damping=0.05)

        def same(what):
            for who, h in (("group", g), ("one device", one)):
                if not (np.array_equal(bits(h.get_positions()), bits(o.x)) and np.array_equal(bits(h.get_velocities()), bits(o.v))):
                    why.append(f"leg {name}: {who}: {what}")
        g.step(); one.step(); o.step(DT, S)
        for t, cols in enumerate(plan_of_calls()):
            before = (o.x.copy(), o.v.copy())
            d0 = [s["device_bytes"] for s in stats()]
            hits = collide((g, one), o, cols)           # (the call meets every rank's held-back last kernel)
            if [s["device_bytes"] for s in stats()] != d0:       # (around the call alone: a state read may allocate its staging)
                why.append(f"leg {name}, call {t}: device bytes changed")
            if t < 2 and not hits.any(axis=1).all():
                why.append(f"leg {name}, call {t}: a collider touched nothing")
            if hits.sum() < 200 or np.array_equal(bits(before[1]), bits(o.v)) or not np.array_equal(bits(before[0][pins]), bits(o.x[pins])):
                why.append(f"leg {name}, call {t}: the reference changed too little, or moved a pin")
            if t == 1:
                same("state right after the call")
            g.step(); one.step(); o.step(DT, S)
            same(f"state after the tick behind call {t}")
        # steps without a call fuse again on every rank; an empty call changes nothing; the step after a call starts unfused on every rank
        g.step(); o.step(DT, S)
        f0 = [s["ticks_fused"] for s in stats()]
        g.step(); g.collide([]); g.step(); o.step(DT, S); o.step(DT, S)
        f1 = [s["ticks_fused"] for s in stats()]
        if not all(b == a + 2 for a, b in zip(f0, f1)):
            why.append(f"leg {name}: ticks_fused without a call: {f0} -> {f1}")
        collide((g,), o, plan_of_calls()[1])
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
    print(("COLLIDER GROUP OK" if ok else "COLLIDER GROUP MISMATCH " + "; ".join(why[:12])), f"host={host} ghosts={ghosts}")
    return ok


if __name__ == "__main__":
    sys.exit(0 if main(sys.argv[1]) else 1)
