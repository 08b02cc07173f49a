#!/usr/bin/env python3
"""What collider contacts between ticks cost (SPEC.md 2f, sb_group_collide), beside the tick they sit in front of, the lost fusion alone
and the route they replace.

jelly_cube(n), `substeps` substeps per tick, every leg in a FRESH group of one device (a collider through the body changes the state the
next leg would start from), same process, same box. Legs, ms per tick:
  (1) no call: the lazy tick boundary stays fused
  (2) one call with 1 collider clear of the body: the lost fusion plus one pass that reads 16 B per particle and writes nothing
  (3) one call with 1 collider through the body's middle (a sphere of an eighth of the cube's volume; the constraints pull the particles
      back in during the tick, so the contacts are there again at every call)
  (4) one call with 16 colliders (spheres spread through the body): one launch, the particles carried in registers across the list
  (5) one PARTICLE impulse of nothing on one particle before every tick: the lost fusion alone
  (6) the route it replaces: get_positions + get_velocities + tests/collider_ref.py in numpy + set_state before every tick
Legs 1 - 5 are timed with HIP events on the rank's stream (sb_profile_begin / sb_profile_end) and with the wall clock around the loop
(ending in a synchronize), `repeats` times each; leg 6 spends its time on the host and over PCIe, so its wall clock is the figure, over
fewer ticks. The per-tick cost of a call is reported against leg 1 and against leg 5 of the same run. Beside them the pass alone -- the
HIP-event time of one call on a completed tick -- for legs 2 - 4 with the bytes of the model (16 B per particle read; a lane of four
particles with a hit reads its 48 B of velocities and writes back the 16-byte words a contact changed: counted from the reference as
(12 + 24) B per particle hit, a floor). One JSON line; --out FILE also writes it there.

usage: collider_bench.py [--cube-n 256] [--substeps 20] [--ticks 20] [--repeats 3] [--skip-state-round-trip] [--out FILE]
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
    return {"best": min(ms), "median": float(np.median(ms)), "all": [round(v, 5) for v in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cube-n", type=int, default=256)
    ap.add_argument("--substeps", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-state-round-trip", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import collider_ref
    from collider_ref import to_native
    from embedding_bench import _clocks
    from softbodyunity_amd import SoftbodyGroup, impulse_particles, jelly_cube
    n = a.cube_n
    mesh = jelly_cube(n)
    lo, hi = mesh.pos.min(axis=0).astype(np.float64), mesh.pos.max(axis=0).astype(np.float64)
    mid, ext = (lo + hi) / 2, float((hi - lo).max())
    rng = np.random.default_rng(1)
    kw = dict(friction=0.5, restitution=0.0)
    clear = [collider_ref.sphere(hi + 10.0 * ext, 0.25 * ext, **kw)]
    middle = [collider_ref.sphere(mid, 0.31 * ext, **kw)]                                         # 4/3 pi 0.31^3 = an eighth of the cube
    sixteen = [collider_ref.sphere(lo + (hi - lo) * rng.uniform(0.15, 0.85, size=3), 0.08 * ext, **kw) for _ in range(16)]
    nothing = impulse_particles([0], (0.0, 0.0, 0.0))
    legs = {"1_no_call": None, "2_one_collider_clear": clear, "3_one_collider_through_the_middle": middle, "4_sixteen_colliders": sixteen,
            "5_particle_impulse": "impulse"}
    res = {"tool": "collider_bench", "ticks": a.ticks, "repeats": a.repeats, "substeps": a.substeps, "particles": int(mesh.n),
           "timing": "ms per tick: HIP events on the rank's stream and wall clock around the loop (legs 1-5, each in a fresh group), wall clock (leg 6); per call (the pass alone)",
           "clocks_before": _clocks()}
    dev, wall, fused, alone, hit_particles = {}, {}, {}, {}, {}
    for name, what in legs.items():
        g = SoftbodyGroup(mesh, [0], substeps=a.substeps).Start()
        try:
            r0 = g.rank(0)
            items = [to_native(c) for c in what] if isinstance(what, list) else None

            def run(ticks):
                for _ in range(ticks):
                    if items is not None:
                        g.collide(items)
                    elif what == "impulse":
                        g.apply_impulses(nothing)
                    g.step()
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
            if items is not None:                                # the pass alone, on a completed tick
                alone[name] = []
                for k in range(a.repeats + 2):
                    g.step(); x = g.get_positions(); g.get_velocities()
                    if k == 0:
                        v = g.get_velocities()
                        hit_particles[name] = int(collider_ref.apply(x.copy(), v.copy(), np.asarray(mesh.inv_mass, np.float32), what).any(axis=0).sum())
                    r0.profile_begin(); g.collide(items); alone[name].append(r0.profile_end())
                alone[name] = alone[name][2:]
        finally:
            g.OnDestroy()
    res["legs_device_ms_per_tick"] = {k: _stat(v) for k, v in dev.items()}
    res["legs_wall_ms_per_tick"] = {k: _stat(v) for k, v in wall.items()}
    res["ticks_fused_per_leg"] = fused
    med = {k: res["legs_device_ms_per_tick"][k]["median"] for k in legs}
    res["added_device_ms_per_tick_over_no_call"] = {k: med[k] - med["1_no_call"] for k in legs if k != "1_no_call"}
    res["added_device_ms_per_tick_over_particle_impulse"] = {k: med[k] - med["5_particle_impulse"] for k in legs if k[0] in "234"}
    res["alone_device_ms"] = {k: _stat(v) for k, v in alone.items()}
    res["particles_hit_at_the_first_lone_call"] = hit_particles
    model = {k: 16 * mesh.n + 36 * hit_particles[k] for k in alone}
    res["model_bytes_floor"] = model
    res["model_gb_per_s"] = {k: model[k] / (res["alone_device_ms"][k]["median"] * 1e-3) / 1e9 for k in model}
    if not a.skip_state_round_trip:
        g = SoftbodyGroup(mesh, [0], substeps=a.substeps).Start()
        try:
            x = np.zeros((mesh.n, 3), np.float32); v = np.zeros((mesh.n, 3), np.float32)
            w = np.ascontiguousarray(mesh.inv_mass, np.float32)
            ticks6 = max(2, a.ticks // 10)
            ms, parts = [], []
            for rep in range(2):
                g.synchronize()
                part = {"get_positions": 0.0, "get_velocities": 0.0, "numpy": 0.0, "set_state": 0.0}
                t0 = time.perf_counter()
                for t in range(ticks6):
                    ta = time.perf_counter(); g.get_positions(x)
                    tb = time.perf_counter(); g.get_velocities(v)
                    tc = time.perf_counter(); collider_ref.apply(x, v, w, middle)
                    td = time.perf_counter(); g.set_state(x, v)
                    te = time.perf_counter()
                    for key, d in (("get_positions", tb - ta), ("get_velocities", tc - tb), ("numpy", td - tc), ("set_state", te - td)):
                        part[key] += d * 1e3 / ticks6
                    g.step()
                g.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3 / ticks6)
                parts.append(part)
            res["6_replaced_route_wall_ms_per_tick"] = {"all": _stat(ms[1:]), "calls_ms": parts[-1], "ticks": ticks6, "colliders": 1,
                                                        "bytes_over_pcie": {"get_positions": 12 * mesh.n, "get_velocities": 12 * mesh.n, "set_state": 24 * mesh.n}}
            res["call_wall_ms_per_tick_vs_replaced_route"] = {"one_collider_through_the_middle": res["legs_wall_ms_per_tick"]["3_one_collider_through_the_middle"]["median"],
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
