"""sb_group_collide_reactions / sb_group_get_collider_reactions in a process of its own (tests/test_gpu_collider_reactions.py starts it, the
way tests/test_gpu_colliders.py starts tests/collider_group_case.py): ranks of one process on one device over the peer transport. The
lists of tests/collider_group_case.py -- colliders that straddle the cuts between the ranks -- between the ticks of a 24^3 cube with a
pinned top layer, under the automatic partition (every rank holds the whole mesh), under SB_PARTITION_BLOCKS (ranks hold windows) and on
four ranks. The state is bit for bit the oracle's with tests/collider_ref.py between its ticks; the records, the ranks' rows added in
rank order, are within SPEC.md 2g's bound of the WHOLE body's reference and their counts are exact: a particle that is a ghost on some
rank is counted once, by its owner.
Prints `COLLIDER REACTION GROUP OK ...` or `COLLIDER REACTION GROUP MISMATCH ...`.

usage: collider_reaction_group_case.py <threads|walk>
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import collider_reaction_ref as rref                                   # noqa: E402
from oracle import oracle                                              # noqa: E402  (test infrastructure: the checker)
from helpers import build_plan, make_oracle                            # noqa: E402
from collider_group_case import DT, N, S, TILE, plan_of_calls          # noqa: E402
from collider_ref import bits, to_native                               # noqa: E402
from softbodyunity_amd import SoftbodyGroup, native                    # noqa: E402
from softbodyunity_amd.mesh import jelly_cube                          # noqa: E402


def ghosts_among(hit, owner):
    """how many of the hit particles have a lattice neighbour along an axis that another rank owns: each is a ghost on that rank"""
    grid, h = owner.reshape(N, N, N), hit.reshape(N, N, N)
    other = np.zeros((N, N, N), bool)
    for ax in range(3):
        a, b = [slice(None)] * 3, [slice(None)] * 3
        a[ax], b[ax] = slice(0, N - 1), slice(1, N)
        differ = grid[tuple(a)] != grid[tuple(b)]
        other[tuple(a)] |= differ; other[tuple(b)] |= differ
    return int((h & other).sum())


def leg(name, host, devices, partition, why):
    mesh = jelly_cube(N)
    pins = np.nonzero(mesh.pos[:, 1] > mesh.pos[:, 1].max() - 0.5)[0].astype(np.int32)
    mesh.inv_mass[pins] = 0.0
    W = len(devices)
    tune = native.SbTuning(); native.lib().sb_tuning_default(C.byref(tune)); tune.peek_min_tiles = 0       # small launches peek too
    kw = dict(substeps=S, tile_particles=TILE, damping=0.05, tuning=tune)
    g = SoftbodyGroup(mesh, devices, halo_transport=native.SB_TRANSPORT_PEER, walk=host == "walk", partition=partition, **kw).Start()
    try:
        stats = lambda: [g.rank(r).stats() for r in range(W)]       # noqa: E731
        st0 = stats()
        ghosts = sum(s["n_particles_local"] - s["n_particles_owned"] for s in st0)
        if ghosts <= 0 or sum(s["n_particles_owned"] for s in st0) != mesh.n:
            why.append(f"leg {name}: no ghosts, or the ranks do not own the mesh once")
        owner = None
        if partition == native.SB_PARTITION_AUTO:       # every rank numbers the whole mesh: rank 0 knows every particle's owner
            r0 = g.rank(0); r0.n = mesh.n
            owner = r0.owner()
            if len(set(owner.tolist())) != W:
                why.append(f"leg {name}: {len(set(owner.tolist()))} owners for {W} ranks")
        o = make_oracle(oracle, mesh, build_plan(mesh, tile_particles=TILE), damping=0.05)
        g.step(); o.step(DT, S)
        worst, hit_ghosts = 0.0, 0
        for t, cols in enumerate(plan_of_calls()):
            d0 = [s["device_bytes"] for s in stats()]       # (around the call alone: a state read may allocate its staging)
            g.collide_with_reactions([to_native(c) for c in cols])
            d1 = [s["device_bytes"] for s in stats()]
            hits, refs = rref.apply(o.x, o.v, o.w, cols)
            if t == 0 and not all(b > a for a, b in zip(d0, d1)):
                why.append(f"leg {name}: the first call allocated nothing on some rank")
            if t > 0 and d1 != d0:
                why.append(f"leg {name}, call {t}: device bytes changed")
            if t < 2 and not hits.any(axis=1).all():
                why.append(f"leg {name}, call {t}: a collider touched nothing")
            if owner is not None:
                hit_ghosts += ghosts_among(hits.any(axis=0), owner)
            else:       # windows: blocks are cut at the cube's middle planes, whichever axes; a hit particle beside each of them
                near = np.abs(mesh.pos[hits.any(axis=0)] - (N - 1) / 2) < 1.0
                hit_ghosts += int(near.any(axis=0).all()) * int(near.any(axis=1).sum())
            got = g.collider_reactions()
            again = g.collider_reactions()
            if got.tobytes() != again.tobytes() or len(got) != len(cols):
                why.append(f"leg {name}, call {t}: the fetch does not repeat, or its length is not the list's")
                continue
            for k, (rec, ref) in enumerate(zip(got, refs)):
                for complaint in rref.check(rec, ref):
                    why.append(f"leg {name}, call {t}, collider {k}: {complaint}")
                worst = max(worst, rref.worst_ratio(rec, ref))
            if t < 2 and not (np.any(got["impulse"] != 0) and np.any(got["angular_impulse"] != 0)):
                why.append(f"leg {name}, call {t}: no impulse or no torque")
            g.step(); o.step(DT, S)
            if got.tobytes() != g.collider_reactions().tobytes():
                why.append(f"leg {name}, call {t}: the records changed behind a step")
            if not (np.array_equal(bits(g.get_positions()), bits(o.x)) and np.array_equal(bits(g.get_velocities()), bits(o.v))):
                why.append(f"leg {name}: state after the tick behind call {t}")
        if hit_ghosts <= 0:
            why.append(f"leg {name}: no hit particle is a ghost on another rank")
        # the step after a reactions call starts unfused on every rank, the one after it fuses; a fetch in between costs nothing
        g.step(); o.step(DT, S)
        g.collide_with_reactions([to_native(c) for c in plan_of_calls()[1]]); rref.apply(o.x, o.v, o.w, plan_of_calls()[1])
        f0 = [s["ticks_fused"] for s in stats()]
        g.step(); o.step(DT, S)
        f1 = [s["ticks_fused"] for s in stats()]
        g.collider_reactions()
        g.step(); o.step(DT, S)
        f2 = [s["ticks_fused"] for s in stats()]
        if f1 != f0 or not all(b == a + 1 for a, b in zip(f1, f2)):
            why.append(f"leg {name}: ticks_fused around a call and a fetch: {f0} -> {f1} -> {f2}")
        if not (np.array_equal(bits(g.get_positions()), bits(o.x)) and np.array_equal(bits(g.get_velocities()), bits(o.v))):
            why.append(f"leg {name}: final state")
        if not np.isfinite(o.x).all():
            why.append(f"leg {name}: the oracle's state is not finite")
        return ghosts, hit_ghosts, round(worst, 3)
    finally:
        g.OnDestroy()


def main(host):
    why = []
    seen = [leg("whole mesh on 2", host, [0, 0], native.SB_PARTITION_AUTO, why),
            leg("windows on 2", host, [0, 0], native.SB_PARTITION_BLOCKS, why),
            leg("whole mesh on 4", host, [0, 0, 0, 0], native.SB_PARTITION_AUTO, why)]
    ok = not why
    print(("COLLIDER REACTION GROUP OK" if ok else "COLLIDER REACTION GROUP MISMATCH " + "; ".join(why[:12])), f"host={host} (ghosts, hit ghosts, worst error / bound)={seen}")
    return ok


if __name__ == "__main__":
    sys.exit(0 if main(sys.argv[1]) else 1)
