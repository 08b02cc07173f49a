#!/usr/bin/env python3
"""What impulses between ticks cost (SPEC.md 2c, sb_apply_impulses), beside the tick they sit in front of.

jelly_cube(n), ONE solver, same process, same box, `substeps` substeps per tick. Legs, ms per tick:
  (1) no call: the lazy tick boundary stays fused
  (2) one PARTICLE item before every tick: (2) - (1) is the price of the lost fusion (the boundary's last kernel and the next tick's first
      kernel run apart) plus the sparse launch
  (3) one RADIAL item before every tick that reaches half the body
  (4) 16 RADIAL items in one call before every tick
  (5) sb_get_velocities + sb_set_state before every tick: the only way to change a velocity without sb_apply_impulses
Legs 1 - 4 are interleaved and repeated, timed with HIP events on the solver's stream (sb_profile_begin / sb_profile_end) and with the
wall clock around the loop (ending in sb_synchronize); leg 5 spends its time on the host and over PCIe, so its wall clock is the figure, over
fewer ticks. Beside them the radial pass alone -- the HIP-event time of one sb_apply_impulses on a completed tick, 1 and 16 items -- with
its modelled bytes (16 B per owned particle + 24 B per particle reached), and snapshot_kernel (sb_readback_begin on a completed tick,
24 B per particle) measured the same way in the same run. The impulses are tiny (the body keeps its shape over the run).
One JSON line; --out FILE also writes it there.

The KERNEL time of the radial pass comes from a trace, in a run of its own (an event pair around a call also holds the launch overhead):
  rocprofv3 --kernel-trace --stats -d DIR -o kt --output-format csv -- python3 tools/impulse_bench.py --ticks 4 --repeats 2 --skip-state-round-trip
  python3 tools/impulse_bench.py --trace DIR/kt_kernel_trace.csv --ticks 4 --repeats 2 [--out FILE]
The second command needs no GPU: it walks the trace's impulse_radial_kernel dispatches in start order and labels them by the order this tool
launches them in (warm-up, the interleaved legs 3 and 4, then 1 and 16 items alternating on completed ticks).

usage: impulse_bench.py [--cube-n 256] [--substeps 20] [--ticks 20] [--repeats 3] [--skip-state-round-trip] [--trace CSV] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stat(ms):
    return {"best": min(ms), "median": float(np.median(ms)), "all": [round(v, 5) for v in ms]}


WARM_TICKS = 3


def summarise_trace(path, n, ticks, repeats):
    """kernel times (us) of the radial pass and of snapshot_kernel from a rocprofv3 kernel trace of this tool run with the same --ticks / --repeats"""
    import csv
    radial, snap = [], []
    with open(path) as f:
        for r in csv.DictReader(f):
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            if "impulse_radial_kernel" in r["Kernel_Name"]:
                radial.append((int(r["Start_Timestamp"]), us))
            elif "snapshot_kernel" in r["Kernel_Name"]:
                snap.append(us)
    radial = [us for _, us in sorted(radial)]
    labels = ["warm_1"] * WARM_TICKS + ["warm_16"] * WARM_TICKS + (["tick_1"] * ticks + ["tick_16"] * ticks) * repeats + ["alone_1", "alone_16"] * (repeats + 2)
    if len(labels) != len(radial):
        raise SystemExit(f"the trace holds {len(radial)} radial passes, this tool launches {len(labels)} with --ticks {ticks} --repeats {repeats}")
    by = {}
    for lab, us in zip(labels, radial):
        by.setdefault(lab, []).append(us)
    particles = n ** 3
    out = {"tool": "impulse_bench --trace", "ticks": ticks, "repeats": repeats, "particles": particles,
           "radial_kernel_us": {k: _stat(v) for k, v in by.items() if not k.startswith("warm")},
           "snapshot_kernel_us": _stat(snap), "snapshot_kernel_bytes": 24 * particles,
           "snapshot_kernel_gb_per_s": 24 * particles / (float(np.median(snap)) * 1e-6) / 1e9,
           "labels": "tick_*: in front of a tick, behind its held-back last kernel; alone_*: on a completed tick; 1 / 16 = RADIAL items in the pass"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", default=None, help="summarise a rocprofv3 kernel trace of this tool instead of running (no GPU needed)")
    ap.add_argument("--cube-n", type=int, default=256)
    ap.add_argument("--substeps", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-state-round-trip", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace:
        line = json.dumps(summarise_trace(a.trace, a.cube_n, a.ticks, a.repeats))
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    from softbodyunity_amd import Softbody, impulse_explosion, impulse_particles, jelly_cube
    from embedding_bench import _clocks
    n = a.cube_n
    mesh = jelly_cube(n)
    lo, hi = mesh.pos.min(axis=0), mesh.pos.max(axis=0)
    mid = ((lo + hi) / 2).astype(np.float32)
    half_radius = float((3.0 / (8.0 * np.pi)) ** (1.0 / 3.0) * (hi - lo + 1.0).max())      # a sphere of half the cube's volume
    r2 = ((mesh.pos - mid) ** 2).sum(axis=1)
    one_particle = impulse_particles([mesh.n // 2], (0.0, 1e-6, 0.0))
    one_radial = impulse_explosion(mid, half_radius, 1e-7, linear_falloff=True)
    rng = np.random.default_rng(1)
    radii = rng.uniform(0.2, 1.0, size=16) * half_radius
    sixteen = np.concatenate([impulse_explosion(mid + rng.uniform(-0.2, 0.2, size=3).astype(np.float32) * (hi - lo), radii[k], 1e-7 * (-1) ** k, linear_falloff=bool(k & 1))
                              for k in range(16)])
    reached = {"one_radial": int(((r2 > 0) & (r2 <= np.float32(half_radius) ** 2)).sum()),
               "sixteen_radial_any": int(np.any([(((mesh.pos - it["vec"]) ** 2).sum(axis=1) <= it["radius"] ** 2) for it in sixteen], axis=0).sum())}
    res = {"tool": "impulse_bench", "ticks": a.ticks, "repeats": a.repeats, "substeps": a.substeps, "particles": int(mesh.n),
           "timing": "ms per tick: HIP events on the solver's stream and wall clock around the loop (legs 1-4), wall clock (leg 5); per call (radial pass, snapshot_kernel)",
           "reached": reached, "clocks_before": _clocks()}
    sb = Softbody(mesh, substeps=a.substeps).Start()
    try:
        legs = {"1_no_call": None, "2_one_particle": one_particle, "3_one_radial_half_body": one_radial, "4_sixteen_radial": sixteen}
        dev = {k: [] for k in legs}
        wall = {k: [] for k in legs}
        fused = {}

        def run(items, ticks):
            for _ in range(ticks):
                if items is not None:
                    sb.apply_impulses(items)
                sb.step()
        for name, items in legs.items():                         # warm-up: first launches, the table ring, the graph of either tick shape
            run(items, WARM_TICKS); sb.synchronize()
        for _ in range(a.repeats):                               # interleaved: a drift of the box's clocks lands on every leg alike
            for name, items in legs.items():
                f0 = sb.stats()["ticks_fused"]
                sb.synchronize()
                t0 = time.perf_counter()
                sb.profile_begin()
                run(items, a.ticks)
                dev[name].append(sb.profile_end() / a.ticks)
                sb.synchronize()
                wall[name].append((time.perf_counter() - t0) * 1e3 / a.ticks)
                fused[name] = sb.stats()["ticks_fused"] - f0
        res["legs_device_ms_per_tick"] = {k: _stat(v) for k, v in dev.items()}
        res["legs_wall_ms_per_tick"] = {k: _stat(v) for k, v in wall.items()}
        res["ticks_fused_per_leg"] = fused
        base = res["legs_device_ms_per_tick"]["1_no_call"]["median"]
        res["added_device_ms_per_tick"] = {k: res["legs_device_ms_per_tick"][k]["median"] - base for k in legs if k != "1_no_call"}
        # the radial pass alone, and snapshot_kernel, on a completed tick
        alone = {"radial_1_item": [], "radial_16_items": [], "particle_1_item": [], "snapshot_kernel": []}
        for _ in range(a.repeats + 2):
            for name, items in (("radial_1_item", one_radial), ("radial_16_items", sixteen), ("particle_1_item", one_particle)):
                sb.step(); sb.get_velocities()                   # (completes the tick: no held-back kernel in the timed span)
                sb.profile_begin(); sb.apply_impulses(items); alone[name].append(sb.profile_end())
            sb.step(); sb.get_velocities()
            sb.profile_begin(); sb.readback_begin(); alone["snapshot_kernel"].append(sb.profile_end())
            sb.readback_end()
        res["alone_device_ms"] = {k: _stat(v[2:]) for k, v in alone.items()}
        model = {"radial_1_item": 16 * mesh.n + 24 * reached["one_radial"], "radial_16_items": 16 * mesh.n + 24 * reached["sixteen_radial_any"],
                 "snapshot_kernel": 24 * mesh.n}
        res["model_bytes"] = model
        res["model_gb_per_s"] = {k: model[k] / (res["alone_device_ms"][k]["median"] * 1e-3) / 1e9 for k in model}
        if not a.skip_state_round_trip:
            v = np.zeros((mesh.n, 3), np.float32); x = np.zeros((mesh.n, 3), np.float32)
            ticks5 = max(2, a.ticks // 5)
            ms, parts = [], []
            for rep in range(a.repeats + 1):
                sb.synchronize()
                part = {"sb_get_positions": 0.0, "sb_get_velocities": 0.0, "sb_set_state": 0.0}
                t0 = time.perf_counter()
                for _ in range(ticks5):
                    ta = time.perf_counter(); sb.get_positions(x)          # (sb_set_state takes positions too: a host that does not hold the tick-end positions reads them)
                    tb = time.perf_counter(); sb.get_velocities(v)
                    v[mesh.n // 2, 1] += np.float32(1e-6)
                    tc = time.perf_counter(); sb.set_state(x, v)
                    td = time.perf_counter()
                    part["sb_get_positions"] += (tb - ta) * 1e3 / ticks5; part["sb_get_velocities"] += (tc - tb) * 1e3 / ticks5; part["sb_set_state"] += (td - tc) * 1e3 / ticks5
                    sb.step()
                sb.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3 / ticks5)
                parts.append(part)
            without_positions = [m - p["sb_get_positions"] for m, p in zip(ms, parts)]
            res["5_state_round_trip_wall_ms_per_tick"] = {"with_sb_get_positions": _stat(ms[1:]), "sb_get_velocities_and_sb_set_state_only": _stat(without_positions[1:]),
                                                          "calls_ms": {k: float(np.median([p[k] for p in parts[1:]])) for k in parts[0]}, "ticks": ticks5,
                                                          "bytes_over_pcie": {"sb_get_velocities": 12 * mesh.n, "sb_set_state": 24 * mesh.n, "sb_get_positions": 12 * mesh.n}}
    finally:
        sb.OnDestroy()
    res["clocks_after"] = _clocks()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
