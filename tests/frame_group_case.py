"""Frame sequences on a group of several ranks, in a process of their own (tests/test_gpu_frame_sequences.py starts it, the way
tests/test_gpu_heightfield.py starts tests/heightfield_group_case.py): ranks of one process on one device over the peer transport, walking
scripts of tests/frame_sequence_cases.py's fixed slice -- surface forces turned into the refusal they are there (SPEC.md 2e) -- with every
rank holding the whole mesh (the automatic partition) and with ranks holding windows (SB_PARTITION_BLOCKS). Every observation is compared
with the reference driver's as on one rank; of the counters ticks_fused must agree on every rank and with the model, and
ticks_fused_kinematic is the largest of the ranks' (a rank that owns none of the targets carries none along: its set_kinematic returns
early, and a state-changing call behind the move must still complete its tick). A fourth leg per case comes from the slice's second block:
a kinematic move right in front of a collide_distance_field on a full slot (SPEC.md 2i) -- the table copied to every rank, ghosts treated by
their holder, and every rank's tick completed whether or not it owns a pin.
Prints `FRAME GROUP OK ...` or `FRAME GROUP MISMATCH ...`.

usage: frame_group_case.py <threads|walk> <ranks>
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import frame_sequence_cases as fc                                      # noqa: E402
from oracle import oracle                                              # noqa: E402  (test infrastructure: the checker)
from softbodyunity_amd import native                                   # noqa: E402


def scripts_for(case):
    """-> [(seed, partition)]: scenarios of the slice in which a kinematic move stands right in front of a state-changing call, on the lattice
    bodies (windows are cut from lattices), one per partition; and one randomly drawn scenario on whatever body it drew"""
    moved = {"cube16": [], "cube10": []}
    for seed in range(fc.N_PAIRS + fc.N_PLANTED):
        sc = fc.make_scenario(seed)
        names = [fc.coverage_name(n, a) for n, a in sc["script"]]
        if sc["body"] in moved and any(p == "set_kinematic_positions" and q in fc.STATE_CHANGING for p, q in zip(names, names[1:])):
            moved[sc["body"]].append(seed)
    # ... and of the second block one in which the move stands right in front of a signed-distance call on a full slot: cases 0 and 2 on the
    # 16-cube with the automatic partition, cases 1 and 3 on the 10-cube in windows
    props = {"cube16": [], "cube10": []}
    for seed in fc.SECOND_BLOCK[:fc.N2_PAIRS + fc.N2_PLANTED]:
        sc = fc.make_scenario(seed)
        full = set()
        for k, (name, a) in enumerate(sc["script"]):
            if name == "set_distance_field":
                full.add(a["slot"])
            elif name == "clear_distance_field":
                full.discard(a["slot"])
            elif name == fc.D and a["slot"] in full and sc["script"][k - 1][0] == "set_kinematic_positions" and sc["body"] in props and seed not in props[sc["body"]]:
                props[sc["body"]].append(seed)
    prop = (props["cube10"][case // 2], native.SB_PARTITION_BLOCKS) if case % 2 else (props["cube16"][case // 2], native.SB_PARTITION_AUTO)
    # the 16-cube's pins are one edge, which the last rank owns alone under either partition: the early return of set_kinematic on the others
    return [(moved["cube16"][case], native.SB_PARTITION_AUTO), (moved["cube10"][case], native.SB_PARTITION_BLOCKS),
            (fc.N_PAIRS + fc.N_PLANTED + case, native.SB_PARTITION_AUTO), prop]


def main(host, ranks):
    oracle.build()
    case = 2 * (host == "walk") + (ranks == 4)
    why, notes = [], []
    some_rank_owns_no_pin = False
    for seed, partition in scripts_for(case):
        sc = fc.for_ranks(fc.make_scenario(seed))
        want = fc.run_reference(oracle, sc, world=ranks)
        t0 = time.perf_counter()
        g = fc.open_group(sc, devices=[0] * ranks, halo_transport=native.SB_TRANSPORT_PEER, walk=host == "walk", partition=partition)
        try:
            st = [g.rank(r).stats() for r in range(ranks)]
            if sum(s["n_particles_owned"] for s in st) != g.n:
                why.append(f"seed {seed}: the ranks do not own the mesh once")
            if partition == native.SB_PARTITION_AUTO:       # every rank numbers the whole mesh: rank 0 knows every particle's owner
                r0 = g.rank(0); r0.n = g.n
                owners = set(r0.owner()[fc.body(sc["body"])["pins"]].tolist())
                some_rank_owns_no_pin = some_rank_owns_no_pin or len(owners) < ranks
            got = fc.run_group(g, sc)
        finally:
            g.OnDestroy()
        bad = fc.first_mismatch(want, got)
        if bad:
            why.append(fc.report(sc, want, got, *bad, command=f"python tests/frame_group_case.py {host} {ranks}"))
        notes.append(f"seed {seed} ({sc['body']}, partition {partition}, {len(sc['script'])} steps, {time.perf_counter() - t0:.1f} s)")
    if not some_rank_owns_no_pin:
        why.append("in no leg did a rank own none of the pinned particles: the early return of set_kinematic was not met")
    ok = not why
    print(("FRAME GROUP OK" if ok else "FRAME GROUP MISMATCH " + "\n".join(why[:4])), f"host={host} ranks={ranks}: " + ", ".join(notes))
    return ok


if __name__ == "__main__":
    sys.exit(0 if main(sys.argv[1], int(sys.argv[2])) else 1)
