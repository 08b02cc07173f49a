"""sb_group_get_body_state on a group of several ranks, in a process of its own (tests/test_gpu_body_state.py starts it, the way
tests/test_gpu_bounds.py starts tests/bounds_group_case.py): a ticking 24^3 cube on 1, 2 and 4 ranks of one process on one device over the peer
transport. Every rank reduces what it owns and the host adds the ranks' sums in rank order, so the group's sums are checked against
tests/body_state_ref.py on the oracle's state within SPEC.md 6f's bound, the counts add up to the body, and the derived fields agree with the
one-rank group's.

Tolerance of that last comparison: 64 * 2^-53 of each field's natural scale (body_state_ref.field_scales: the two groups differ by the order
of a few dozen additions per sum, a handful of roundings of A_k, and this body is well conditioned -- a cube's inertia and pose matrix are
close to multiples of the identity); angular_velocity and rotation through the condition of their 3x3 solves, M L Uv / lambda_min(I) and
2 M L Lq / (sigma_2 + sigma_3). Prints `BODY STATE GROUP OK ...` or `BODY STATE GROUP MISMATCH ...`.

usage: body_state_group_case.py <threads|walk>
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import oracle                                              # noqa: E402  (test infrastructure: the checker)
import body_state_ref as B                                             # noqa: E402
from helpers import build_plan, make_oracle                            # noqa: E402
from softbodyunity_amd import SoftbodyGroup, native                    # noqa: E402
from softbodyunity_amd.mesh import jelly_cube                          # noqa: E402

BOTH = B.POSE | B.MOTION
TOL = 64 * B.U


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def main(host):
    n, S, ticks, tile = 24, 6, 2, 64
    mesh = jelly_cube(n)
    tune = native.SbTuning(); native.lib().sb_tuning_default(C.byref(tune)); tune.peek_min_tiles = 0       # small launches peek too
    why = []
    # the oracle's state after every tick, once
    o = make_oracle(oracle, mesh, build_plan(mesh, tile_particles=tile))
    xs, vs = [], []
    for _ in range(ticks):
        o.step(0.02, S)
        xs.append(o.x.copy()); vs.append(o.v.copy())
    answers = {}
    worst_sum, worst_field = 0.0, 0.0
    for ranks in (1, 2, 4):
        g = SoftbodyGroup(mesh, [0] * ranks, substeps=S, tile_particles=tile, halo_transport=native.SB_TRANSPORT_PEER, walk=host == "walk", tuning=tune).Start()
        try:
            owned = [g.rank(r).stats()["n_particles_owned"] for r in range(ranks)]
            if sum(owned) != mesh.n or min(owned) <= 0:
                why.append(f"{ranks} ranks: owned {owned}")
            for t in range(ticks):
                g.step()
                for what in ((B.POSE,) if t == 0 else (B.POSE, B.MOTION, BOTH)):
                    st = g.get_body_state(what)
                    ref = B.sums_ref(xs[t], vs[t], mesh.inv_mass, mesh.rest_pos, what)
                    worst_sum = max(worst_sum, B.worst_ratio(st["sums"], ref, what))
                    why += [f"{ranks} ranks, tick {t}, what {what}: {w}" for w in B.check_sums(st["sums"], ref, what)[:4]]
                    if st["n_dynamic"] + st["n_pinned"] != mesh.n or st["n_pinned"] != 0:
                        why.append(f"{ranks} ranks, tick {t}: counts {st['n_dynamic']} + {st['n_pinned']} for {mesh.n}")
                    if st["flags"] != 0:
                        why.append(f"{ranks} ranks, tick {t}: flags {st['flags']}")
                    again = g.get_body_state(what)
                    if not np.array_equal(st["sums"].view(np.uint64), again["sums"].view(np.uint64)):
                        why.append(f"{ranks} ranks, tick {t}, what {what}: two calls on one state differ")
                    if ranks == 1:
                        answers[(t, what)] = st
                        continue
                    one = answers[(t, what)]
                    full = B.sums_ref(xs[t], vs[t], mesh.inv_mass, mesh.rest_pos, BOTH)["sums"].astype(np.float64)
                    sc = B.field_scales(full, mesh.n)
                    M, L, Lq, Uv = sc["M"], sc["L"], sc["Lq"], sc["Uv"]
                    lam_min = np.linalg.eigvalsh(B.inertia_of(one["second_moment"]))[0]
                    scale = dict(mass=M, com=L, second_moment=M * L * L)
                    if what & B.POSE:
                        sg = np.linalg.svd(one["apq"], compute_uv=False)
                        scale.update(ref_com=Lq, apq=M * L * Lq, rotation=2 * M * L * Lq / (sg[1] + sg[2]))
                    if what & B.MOTION:
                        scale.update(momentum=M * Uv, velocity=Uv, angular_momentum=M * L * Uv, kinetic_energy=M * Uv * Uv,
                                     angular_velocity=M * L * Uv / lam_min)
                    for f, s in scale.items():
                        err = float(np.max(np.abs(np.asarray(st[f]) - np.asarray(one[f])))) / (TOL * s)
                        worst_field = max(worst_field, err)
                        if not err <= 1.0:
                            why.append(f"{ranks} ranks, tick {t}, what {what}: {f} differs from the one-rank group's by {err:.3g} tolerances")
            if ranks > 1 and sum(g.rank(r).stats()["readback_peeks"] for r in range(ranks)) == 0:
                why.append(f"{ranks} ranks: no rank ever peeked")
            if not (np.array_equal(bits(g.get_positions()), bits(xs[-1])) and np.array_equal(bits(g.get_velocities()), bits(vs[-1]))):
                why.append(f"{ranks} ranks: final state")
        finally:
            g.OnDestroy()
    ok = not why
    print(("BODY STATE GROUP OK" if ok else "BODY STATE GROUP MISMATCH " + "; ".join(why[:12])),
          f"host={host} worst sum error / bound {worst_sum:.3e}, worst field difference / tolerance {worst_field:.3e}")
    return ok


if __name__ == "__main__":
    if not B.longdouble_is_extended():
        print("BODY STATE GROUP MISMATCH np.longdouble has no 64-bit mantissa here: no reference")
        sys.exit(1)
    sys.exit(0 if main(sys.argv[1]) else 1)
