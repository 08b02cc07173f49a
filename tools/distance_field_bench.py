#!/usr/bin/env python3
"""What contacts with a signed-distance volume between ticks cost (SPEC.md 2i, sb_group_collide_distance_field), beside the tick they sit in
front of, the lost fusion alone, the collider pass (which reads the same 16 B per particle) and the route they replace.

jelly_cube(n), `substeps` substeps per tick, every leg in a FRESH group of one device (a prop the body lies on changes the state the next
leg would start from), same process, same box. The table has `grid`^3 samples of a sphere's distance. Legs, ms per tick:
  (1) no call: the lazy tick boundary stays fused
  (2) one PARTICLE impulse of nothing on one particle before every tick: the lost fusion alone
  (3) sb_group_collide with one box clear of the body: the lost fusion plus one pass that reads 16 B per particle and writes nothing --
      THE FIGURE TO HOLD LEGS 4 - 6 AGAINST, in the same run
  (4) the table's footprint clear of the body: every lane returns before any gather
  (5) the body resting on the sphere, the middle of its bottom layers in contact
  (6) the whole body inside the footprint but outside the contact band (the sphere is small and far): every particle gathers its eight
      samples and none responds
  (7) the route it replaces: get_positions + get_velocities + tests/distance_field_ref.py in numpy + set_state before every tick
Legs 1 - 6 are timed with HIP events on the rank's stream (sb_profile_begin / sb_profile_end) and with the wall clock around the loop
(ending in a synchronize), `repeats` times each: the median, and the spread (max - min) as the margin. Leg 7 spends its time on the host
and over PCIe, so its wall clock is the figure, over fewer ticks. Beside them the pass alone -- the HIP-event time of one call on a
completed tick, the state set back to the start before it -- for legs 3 - 6, with the particles the reference finds hit at that call.
One JSON line; --out FILE also writes it there. (A kernel trace is a run of its own: rocprofv3 --kernel-trace --stats -- python
tools/distance_field_bench.py --repeats 1 --skip-state-round-trip.)

usage: distance_field_bench.py [--cube-n 256] [--substeps 20] [--ticks 20] [--repeats 3] [--grid 128] [--skip-state-round-trip] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

WARM_TICKS = 3


def _stat(ms):
    return {"median": float(np.median(ms)), "spread": float(max(ms) - min(ms)), "all": [round(v, 5) for v in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cube-n", type=int, default=256)
    ap.add_argument("--substeps", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--skip-state-round-trip", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import collider_ref
    import distance_field_cases
    import distance_field_ref
    from embedding_bench import _clocks
    from softbodyunity_amd import SoftbodyGroup, impulse_particles, jelly_cube
    n = a.cube_n
    mesh = jelly_cube(n)
    w = np.ascontiguousarray(mesh.inv_mass, np.float32)
    lo, hi = mesh.pos.min(axis=0).astype(np.float64), mesh.pos.max(axis=0).astype(np.float64)
    ext, mid = float((hi - lo).max()), (lo + hi) / 2
    spacing = ext / max(1, n - 1)
    G = a.grid
    big, big_side = distance_field_cases.sampled_sphere(2.0 * ext, n=G, pad=0.1, thickness=0.02 * ext)       # the body rests on its top
    small, small_side = distance_field_cases.sampled_sphere(0.2 * ext, n=G, pad=9.0, thickness=0.02 * ext)  # side 4 ext: the body fits in one octant
    at = distance_field_cases.pose_about
    props = {"4_footprint_clear": (big, at(hi + 10.0 * ext, big_side, (0, 0, 0, 1), friction=0.5)),
             "5_resting_on_a_sphere": (big, at((mid[0], lo[1] - 2.0 * ext + 1.5 * spacing, mid[2]), big_side, (0, 0, 0, 1), friction=0.5)),
             "6_every_particle_gathers_none_responds": (small, at(lo - 0.5 * ext, small_side, (0, 0, 0, 1), friction=0.5))}
    clear = [collider_ref.box(hi + 10.0 * ext, np.eye(3), (0.25 * ext,) * 3, friction=0.5, restitution=0.0)]
    nothing = impulse_particles([0], (0.0, 0.0, 0.0))
    legs = {"1_no_call": None, "2_particle_impulse": "impulse", "3_collide_one_box_clear": "box", **props}
    res = {"tool": "distance_field_bench", "ticks": a.ticks, "repeats": a.repeats, "substeps": a.substeps, "particles": int(mesh.n), "grid": G,
           "table_bytes": 4 * G ** 3,
           "timing": "ms per tick: HIP events on the rank's stream and wall clock around the loop (legs 1-6, each in a fresh group), wall clock (leg 7); per call (the pass alone)",
           "clocks_before": _clocks()}
    dev, wall, fused, alone, hit_particles, inside = {}, {}, {}, {}, {}, {}
    for name, what in legs.items():
        print(f"leg {name} ...", file=sys.stderr, flush=True)
        g = SoftbodyGroup(mesh, [0], substeps=a.substeps).Start()
        try:
            r0 = g.rank(0)
            box = [collider_ref.to_native(c) for c in clear] if what == "box" else None
            prop = what if isinstance(what, tuple) else None
            if prop is not None:
                g.set_distance_field(0, *distance_field_ref.to_native(prop[0]))
                pose = distance_field_ref.pose_to_native(prop[1])

            def call():
                if prop is not None:
                    g.collide_distance_field(0, pose)
                elif box is not None:
                    g.collide(box)
                elif what == "impulse":
                    g.apply_impulses(nothing)

            def run(ticks):
                for _ in range(ticks):
                    call()
                    g.step()
            x0, v0 = g.get_positions().copy(), g.get_velocities().copy()
            run(WARM_TICKS + 1); g.synchronize()
            dev[name], wall[name] = [], []
            for _ in range(a.repeats):
                f0 = r0.stats()["ticks_fused"]
                g.synchronize()
                t0 = time.perf_counter()
                r0.profile_begin()
                run(a.ticks)
                dev[name].append(r0.profile_end() / a.ticks)
                g.synchronize()
                wall[name].append((time.perf_counter() - t0) * 1e3 / a.ticks)
                fused[name] = r0.stats()["ticks_fused"] - f0
            if prop is not None or box is not None:              # the pass alone, on a completed tick, from the state of the start
                alone[name] = []
                if prop is not None:
                    inside[name] = int(distance_field_ref.surface(prop[0], prop[1], x0)["inside"].sum())
                    hit_particles[name] = int(distance_field_ref.apply(x0.copy(), v0.copy(), w, *prop).sum())
                else:
                    hit_particles[name] = int(collider_ref.apply(x0.copy(), v0.copy(), w, clear).any(axis=0).sum())
                for k in range(a.repeats + 2):
                    g.set_state(x0, v0); g.synchronize()
                    r0.profile_begin(); call(); alone[name].append(r0.profile_end())
                alone[name] = alone[name][2:]
        finally:
            g.OnDestroy()
    res["legs_device_ms_per_tick"] = {k: _stat(v) for k, v in dev.items()}
    res["legs_wall_ms_per_tick"] = {k: _stat(v) for k, v in wall.items()}
    res["ticks_fused_per_leg"] = fused
    med = {k: res["legs_device_ms_per_tick"][k]["median"] for k in legs}
    res["added_device_ms_per_tick_over_no_call"] = {k: med[k] - med["1_no_call"] for k in legs if k != "1_no_call"}
    res["added_device_ms_per_tick_over_collide_clear"] = {k: med[k] - med["3_collide_one_box_clear"] for k in props}
    res["leg_4_inside_leg_3_spread"] = bool(abs(med["4_footprint_clear"] - med["3_collide_one_box_clear"]) <= res["legs_device_ms_per_tick"]["3_collide_one_box_clear"]["spread"])
    res["alone_device_ms"] = {k: _stat(v) for k, v in alone.items()}
    res["particles_inside_the_footprint_at_the_lone_call"] = inside
    res["particles_hit_at_the_lone_call"] = hit_particles
    res["what_bounds_leg_6"] = "not measured"                    # (needs a kernel trace from a run of its own)
    if not a.skip_state_round_trip:
        print("leg 7 ...", file=sys.stderr, flush=True)
        g = SoftbodyGroup(mesh, [0], substeps=a.substeps).Start()
        try:
            prop = props["5_resting_on_a_sphere"]
            x = np.zeros((mesh.n, 3), np.float32); v = np.zeros((mesh.n, 3), np.float32)
            ticks7 = max(2, a.ticks // 10)
            ms, parts = [], []
            for rep in range(2):
                g.synchronize()
                part = {"get_positions": 0.0, "get_velocities": 0.0, "numpy": 0.0, "set_state": 0.0}
                t0 = time.perf_counter()
                for t in range(ticks7):
                    ta = time.perf_counter(); g.get_positions(x)
                    tb = time.perf_counter(); g.get_velocities(v)
                    tc = time.perf_counter(); distance_field_ref.apply(x, v, w, *prop)
                    td = time.perf_counter(); g.set_state(x, v)
                    te = time.perf_counter()
                    for key, d in (("get_positions", tb - ta), ("get_velocities", tc - tb), ("numpy", td - tc), ("set_state", te - td)):
                        part[key] += d * 1e3 / ticks7
                    g.step()
                g.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3 / ticks7)
                parts.append(part)
                print(f"leg 7 repeat {rep}: {ms[-1]:.0f} ms per tick", file=sys.stderr, flush=True)
            res["7_replaced_route_wall_ms_per_tick"] = {"all": _stat(ms[1:]), "calls_ms": parts[-1], "ticks": ticks7,
                                                        "bytes_over_pcie": {"get_positions": 12 * mesh.n, "get_velocities": 12 * mesh.n, "set_state": 24 * mesh.n}}
            res["call_wall_ms_per_tick_vs_replaced_route"] = {"resting_on_a_sphere": res["legs_wall_ms_per_tick"]["5_resting_on_a_sphere"]["median"],
                                                              "replaced_route": float(np.median(ms[1:]))}
        finally:
            g.OnDestroy()
    res["clocks_after"] = _clocks()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
