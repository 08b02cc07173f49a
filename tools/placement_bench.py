#!/usr/bin/env python3
"""What a placement between ticks costs (SPEC.md 2d, sb_group_place), beside the tick it sits in front of and the route it replaces.

jelly_cube(n), ONE group of one device, same process, same box, `substeps` substeps per tick. Legs, ms per tick:
  (1) no call: the lazy tick boundary stays fused
  (2) a rigid move before every tick (a small rotation about the cube's centre and back: the body keeps its place over the run):
      (2) - (1) is the price of the lost fusion (the boundary's last kernel and the next tick's first kernel run apart) plus one pass
  (3) a FROM_REFERENCE respawn at rest before every tick
  (4) the route it replaces: get_positions + get_velocities + the same map in numpy + set_state before every tick
Legs 1 - 3 are interleaved and repeated, timed with HIP events on the rank's stream (sb_profile_begin / sb_profile_end) and with the wall
clock around the loop (ending in a synchronize); leg 4 spends its time on the host and over PCIe, so its wall clock is the figure, over
fewer ticks. Beside them the pass alone -- the HIP-event time of one call on a completed tick, move and respawn -- with its modelled bytes
(move: 28 B read + 24 B written per particle; respawn of a body without pins: 16 B read + 24 B written), and snapshot_kernel
(readback_begin on a completed tick, 24 B per particle) and one RADIAL impulse that reaches half the body, measured the same way in the
same run. One JSON line; --out FILE also writes it there.

The KERNEL time of the pass comes from a trace, in a run of its own (an event pair around a call also holds the launch overhead):
  rocprofv3 --kernel-trace --stats -d DIR -o kt --output-format csv -- python3 tools/placement_bench.py --ticks 4 --repeats 2 --skip-state-round-trip
  python3 tools/placement_bench.py --trace DIR/kt_kernel_trace.csv [--out FILE]
The second command needs no GPU: it groups the trace's dispatches of place_kernel (by instantiation), snapshot_kernel and
impulse_radial_kernel and divides each one's modelled bytes by its median time.

usage: placement_bench.py [--cube-n 256] [--substeps 20] [--ticks 20] [--repeats 3] [--skip-state-round-trip] [--trace CSV] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM_TICKS = 3
MOVE_BYTES, RESPAWN_BYTES, SNAPSHOT_BYTES = 52, 40, 24          # per particle, by the model


def _stat(ms):
    return {"best": min(ms), "median": float(np.median(ms)), "all": [round(v, 5) for v in ms]}


def _half_radius(n):
    return float((3.0 / (8.0 * np.pi)) ** (1.0 / 3.0) * n)      # a sphere of half the cube's volume


def summarise_trace(path, n):
    """kernel times (us) and model bytes / time of the placement pass, snapshot_kernel and impulse_radial_kernel from one rocprofv3 kernel trace"""
    import csv
    us = {"place_move": [], "place_respawn": [], "snapshot_kernel": [], "impulse_radial_kernel": []}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"].replace(" ", "")
            t = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            if "place_kernel<false,false,false>" in name:
                us["place_move"].append(t)
            elif "place_kernel<true,true,false>" in name:
                us["place_respawn"].append(t)
            elif "snapshot_kernel" in name:
                us["snapshot_kernel"].append(t)
            elif "impulse_radial_kernel" in name:
                us["impulse_radial_kernel"].append(t)
    empty = [k for k, v in us.items() if not v]
    if empty:
        raise SystemExit(f"the trace holds no dispatch of {empty}")
    particles = n ** 3
    from softbodyunity_amd import jelly_cube
    mesh = jelly_cube(n)
    mid = ((mesh.pos.min(axis=0) + mesh.pos.max(axis=0)) / 2).astype(np.float32)
    r2 = ((mesh.pos - mid) ** 2).sum(axis=1)
    reached = int(((r2 > 0) & (r2 <= np.float32(_half_radius(n)) ** 2)).sum())
    model = {"place_move": MOVE_BYTES * particles, "place_respawn": RESPAWN_BYTES * particles, "snapshot_kernel": SNAPSHOT_BYTES * particles,
             "impulse_radial_kernel": 16 * particles + 24 * reached}
    return {"tool": "placement_bench --trace", "particles": particles, "kernel_us": {k: _stat(v) for k, v in us.items()}, "dispatches": {k: len(v) for k, v in us.items()},
            "model_bytes": model, "model_gb_per_s": {k: model[k] / (float(np.median(us[k])) * 1e-6) / 1e9 for k in us},
            "labels": "place_move = place_kernel<false, false, false>, place_respawn = place_kernel<true, true, false>; every dispatch of the run, warm-up included"}


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
        line = json.dumps(summarise_trace(a.trace, a.cube_n))
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    from softbodyunity_amd import SoftbodyGroup, impulse_explosion, jelly_cube, make_placement, placement_from_rotation
    from embedding_bench import _clocks
    n = a.cube_n
    mesh = jelly_cube(n)
    mid = ((mesh.pos.min(axis=0) + mesh.pos.max(axis=0)) / 2).astype(np.float32)
    turn = [placement_from_rotation((0.0, s * 0.001, 0.0, 1.0)) for s in (1, -1)]              # there and back: the body stays where it is
    moves = [make_placement(m, frm=mid, to=mid) for m in turn]
    respawn = make_placement(from_reference=True)
    one_radial = impulse_explosion(mid, _half_radius(n), 1e-7, linear_falloff=True)
    res = {"tool": "placement_bench", "ticks": a.ticks, "repeats": a.repeats, "substeps": a.substeps, "particles": int(mesh.n),
           "timing": "ms per tick: HIP events on the rank's stream and wall clock around the loop (legs 1-3), wall clock (leg 4); per call (the pass alone, snapshot_kernel, radial impulse)",
           "clocks_before": _clocks()}
    g = SoftbodyGroup(mesh, [0], substeps=a.substeps).Start()
    try:
        r0 = g.rank(0)
        legs = {"1_no_call": None, "2_rigid_move": moves, "3_respawn_from_reference": [respawn, respawn]}
        dev = {k: [] for k in legs}
        wall = {k: [] for k in legs}
        fused = {}

        def run(ps, ticks):
            for t in range(ticks):
                if ps is not None:
                    g.place(ps[t & 1])
                g.step()
        for name, ps in legs.items():                            # warm-up: first launches, the reference pose's upload, the graph of either tick shape
            run(ps, WARM_TICKS + 1); g.synchronize()
        for _ in range(a.repeats):                               # interleaved: a drift of the box's clocks lands on every leg alike
            for name, ps in legs.items():
                f0 = r0.stats()["ticks_fused"]
                g.synchronize()
                t0 = time.perf_counter()
                r0.profile_begin()
                run(ps, a.ticks)
                dev[name].append(r0.profile_end() / a.ticks)
                g.synchronize()
                wall[name].append((time.perf_counter() - t0) * 1e3 / a.ticks)
                fused[name] = r0.stats()["ticks_fused"] - f0
        res["legs_device_ms_per_tick"] = {k: _stat(v) for k, v in dev.items()}
        res["legs_wall_ms_per_tick"] = {k: _stat(v) for k, v in wall.items()}
        res["ticks_fused_per_leg"] = fused
        base = res["legs_device_ms_per_tick"]["1_no_call"]["median"]
        res["added_device_ms_per_tick"] = {k: res["legs_device_ms_per_tick"][k]["median"] - base for k in legs if k != "1_no_call"}
        # the pass alone, snapshot_kernel and one radial impulse, each on a completed tick
        alone = {"place_move": [], "place_respawn": [], "radial_1_item": [], "snapshot_kernel": []}
        for k in range(a.repeats + 2):
            for name, call in (("place_move", lambda: g.place(moves[k & 1])), ("place_respawn", lambda: g.place(respawn)), ("radial_1_item", lambda: g.apply_impulses(one_radial))):
                g.step(); g.get_velocities()                     # (completes the tick: no held-back kernel in the timed span)
                r0.profile_begin(); call(); alone[name].append(r0.profile_end())
            g.step(); g.get_velocities()
            r0.profile_begin(); g.readback_begin(); alone["snapshot_kernel"].append(r0.profile_end())
            g.readback_end()
        res["alone_device_ms"] = {k: _stat(v[2:]) for k, v in alone.items()}
        model = {"place_move": MOVE_BYTES * mesh.n, "place_respawn": RESPAWN_BYTES * mesh.n, "snapshot_kernel": SNAPSHOT_BYTES * mesh.n}
        res["model_bytes"] = model
        res["model_gb_per_s"] = {k: model[k] / (res["alone_device_ms"][k]["median"] * 1e-3) / 1e9 for k in model}
        if not a.skip_state_round_trip:
            x = np.zeros((mesh.n, 3), np.float32); v = np.zeros((mesh.n, 3), np.float32)
            ticks4 = max(2, a.ticks // 5)
            ms, parts = [], []
            for rep in range(a.repeats + 1):
                g.synchronize()
                part = {"get_positions": 0.0, "get_velocities": 0.0, "numpy": 0.0, "set_state": 0.0}
                t0 = time.perf_counter()
                for t in range(ticks4):
                    ta = time.perf_counter(); g.get_positions(x)
                    tb = time.perf_counter(); g.get_velocities(v)
                    tc = time.perf_counter()
                    R = turn[t & 1]
                    x[:] = (x - mid) @ R.T + mid                 # (float32 throughout; a BLAS product, not SPEC 2d's bracketing: the cost is what counts here)
                    v[:] = v @ R.T
                    td = time.perf_counter(); g.set_state(x, v)
                    te = time.perf_counter()
                    for key, d in (("get_positions", tb - ta), ("get_velocities", tc - tb), ("numpy", td - tc), ("set_state", te - td)):
                        part[key] += d * 1e3 / ticks4
                    g.step()
                g.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3 / ticks4)
                parts.append(part)
            res["4_replaced_route_wall_ms_per_tick"] = {"all": _stat(ms[1:]), "calls_ms": {k: float(np.median([p[k] for p in parts[1:]])) for k in parts[0]}, "ticks": ticks4,
                                                        "bytes_over_pcie": {"get_positions": 12 * mesh.n, "get_velocities": 12 * mesh.n, "set_state": 24 * mesh.n}}
            res["move_wall_ms_per_tick_vs_replaced_route"] = {"move": res["legs_wall_ms_per_tick"]["2_rigid_move"]["median"], "replaced_route": float(np.median(ms[1:]))}
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
