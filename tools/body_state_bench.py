#!/usr/bin/env python3
"""What the body state (SPEC.md 6f, sb_group_get_body_state) costs per tick, beside the route it replaces.

jelly_cube(n), ONE group on one device, same process, same box. Legs, a query after every tick:
  (1) no query,  (2) POSE,  (3) MOTION,  (4) POSE | MOTION,
interleaved and repeated, timed with HIP events on the rank's stream (sb_profile_begin / sb_profile_end on the borrowed rank handle), best
and median of the repeats, and the difference of each leg's median to leg (1) of the same run. A query is synchronous, so legs (2) - (4)
also carry the launch latency the host's wait exposes once per tick; a MOTION query costs the next tick its fused start on top.
  (5) the device time of ONE query on a completed tick (HIP events around the call), with the bytes the kernel reads by the model --
      28 B per particle for one bit, 40 B for both -- as bytes per second;
  (6) the route a host has without the query: sb_group_get_positions + sb_group_get_velocities + the same sums in numpy float64, wall clock.
One JSON line; --out FILE also writes it there. --trace runs only a handful of queries and one snapshot on a completed tick, for a
`rocprofv3 --kernel-trace --stats` run of its own (kernel times of body_sums_partial_kernel beside snapshot_kernel).

usage: body_state_bench.py [--cube-n 256] [--ticks 20] [--repeats 5] [--out FILE] [--trace]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

POSE, MOTION = 1, 2
LEGS = (("1_no_query", 0), ("2_pose", POSE), ("3_motion", MOTION), ("4_pose_motion", POSE | MOTION))
MODEL_BYTES = {POSE: 28, MOTION: 28, POSE | MOTION: 40}


def _stat(ms):
    return {"best": min(ms), "median": float(np.median(ms)), "all": [round(v, 5) for v in ms]}


def _ticks(g, n_ticks, what):
    for _ in range(n_ticks):
        g.step()
        if what:
            g.get_body_state(what)


def _per_tick(g, r0, ticks, repeats):
    for _, what in LEGS:                                     # warm-up: first launches, the query's buffers, the peek
        _ticks(g, 3, what); g.synchronize()
    ms = {name: [] for name, _ in LEGS}
    for _ in range(repeats):                                 # interleaved: a drift of the box's clocks lands on every leg alike
        for name, what in LEGS:
            g.synchronize()
            r0.profile_begin()
            _ticks(g, ticks, what)
            ms[name].append(r0.profile_end() / ticks)
    out = {name: _stat(v) for name, v in ms.items()}
    for name, _ in LEGS[1:]:
        out[name]["ms_per_tick_over_no_query"] = out[name]["median"] - out["1_no_query"]["median"]
    return out


def _one_query(g, r0, n, repeats):
    out = {}
    for name, what in LEGS[1:]:
        dev = []
        for _ in range(repeats + 1):
            g.step(); g.get_body_state(MOTION)               # (completes the tick and waits for it: no peek, no held-back kernel in the timed span)
            r0.profile_begin(); g.get_body_state(what); dev.append(r0.profile_end())
        st = _stat(dev[1:])
        st["model_bytes"] = MODEL_BYTES[what] * n
        st["model_TB_per_s"] = st["model_bytes"] / (st["median"] * 1e-3) / 1e12
        out[name] = st
    return out


def _host_route(g, mesh, repeats):
    """positions + velocities over PCIe, then the sums on the host"""
    n = mesh.n
    pos = np.zeros((n, 3), np.float32); vel = np.zeros((n, 3), np.float32)
    m = 1.0 / mesh.inv_mass.astype(np.float64)
    q = mesh.rest_pos.astype(np.float64)
    copy, total = [], []
    for _ in range(repeats + 1):
        g.step(); g.synchronize()
        t0 = time.perf_counter()
        g.get_positions(pos); g.get_velocities(vel)
        t1 = time.perf_counter()
        x = pos.astype(np.float64); v = vel.astype(np.float64)
        s = [m.sum(), m @ x, m @ q, np.einsum("p,pa,pb->ab", m, x, x), np.einsum("p,pa,pb->ab", m, x, q), m @ v, m @ np.cross(x, v), m @ np.einsum("pa,pa->p", v, v)]
        t2 = time.perf_counter()
        copy.append((t1 - t0) * 1e3); total.append((t2 - t0) * 1e3)
        del x, v, s
    return {"copies_wall_ms": _stat(copy[1:]), "copies_and_numpy_wall_ms": _stat(total[1:]), "bytes_to_host": 24 * n, "bytes_to_host_query": 592}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cube-n", type=int, default=256)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    from softbodyunity_amd import SoftbodyGroup, jelly_cube
    n = a.cube_n
    mesh = jelly_cube(n)
    g = SoftbodyGroup(mesh, [0], substeps=20).Start()
    try:
        if a.trace:
            for _ in range(3):
                g.step(); g.get_body_state(MOTION)
                for what in (POSE, MOTION, POSE | MOTION):
                    g.get_body_state(what)
                g.readback_begin(); g.readback_end()                # snapshot_kernel on the completed tick, for the comparison
            print(json.dumps({"tool": "body_state_bench", "trace": True, "particles": int(mesh.n)}))
            return
        from embedding_bench import _clocks
        res = {"tool": "body_state_bench", "ticks": a.ticks, "repeats": a.repeats, "substeps": 20, "particles": int(mesh.n),
               "timing": "HIP events on the rank's stream, per tick (legs 1-4) and per call (one_query); wall clock (host_route)", "clocks_before": _clocks()}
        r0 = g.rank(0)
        res["per_tick_ms"] = _per_tick(g, r0, a.ticks, a.repeats)
        res["one_query_on_a_completed_tick_ms"] = _one_query(g, r0, mesh.n, a.repeats)
        res["host_route"] = _host_route(g, mesh, min(a.repeats, 2))
        st = g.get_body_state(POSE | MOTION)
        res["state"] = {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in st.items() if k != "sums"}
        res["clocks_after"] = _clocks()
    finally:
        g.OnDestroy()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
