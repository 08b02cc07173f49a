#!/usr/bin/env python3
"""What the reactions of SPEC.md 2g cost (sb_group_collide_reactions / sb_group_get_collider_reactions) beside sb_group_collide with the same
list, beside the tick both sit in front of, and beside the route they replace.

jelly_cube(n), `substeps` substeps per tick, every leg in a FRESH group of one device, same process, same box. Legs, ms per tick:
  (1)  no call: the lazy tick boundary stays fused
  (2)  collide, 1 collider clear of the body            (3)  reactions, the same collider: no wave reduces anything
  (4)  collide, 1 sphere through the body's middle      (5)  reactions, the same sphere
  (6a) collide, 16 spheres spread through the body      (6b) reactions, the same 16
  (7)  reactions with the sphere of (5) and a fetch at once, every tick: the host waits for the pass before it launches the tick
  (8)  the route it replaces, on the wall clock: get_velocities before the collide call, get_velocities and get_positions after it, and
       the seven sums in numpy float64
Legs 1 - 7 are timed with HIP events on the rank's stream (sb_profile_begin / sb_profile_end) and with the wall clock around the loop
(ending in a synchronize), `repeats` times each: the spread of the repeats is the run's own margin. Beside them the calls alone -- the
HIP-event time of one call on a completed tick: the pass and, for the reactions, the launches that add its rows up -- with the bytes of
the model: collide's floor (16 B per particle read, (12 + 24) B per particle hit) plus, for the reactions, the masks (4 B per workgroup
written and read) and 1 KiB written and read per workgroup that holds a contact, counted as the workgroups of 1 024 consecutive particles
with a hit. --collide-only runs legs 1, 2, 4 and 6a alone: the form that also runs on a commit without the reactions, for the same
session's comparison. --only LEG runs one leg for `ticks` ticks and prints nothing else (for a kernel trace).
One JSON line; --out FILE also writes it there.

usage: collider_reaction_bench.py [--cube-n 256] [--substeps 20] [--ticks 20] [--repeats 3] [--collide-only] [--skip-replaced-route] [--only LEG] [--out FILE]
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
WORKGROUP = 1024


def _stat(ms):
    return {"best": min(ms), "median": float(np.median(ms)), "spread": max(ms) - min(ms), "all": [round(v, 5) for v in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cube-n", type=int, default=256)
    ap.add_argument("--substeps", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--collide-only", action="store_true")
    ap.add_argument("--skip-replaced-route", action="store_true")
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import collider_ref
    from collider_ref import to_native
    from embedding_bench import _clocks
    from softbodyunity_amd import SoftbodyGroup, jelly_cube
    n = a.cube_n
    mesh = jelly_cube(n)
    lo, hi = mesh.pos.min(axis=0).astype(np.float64), mesh.pos.max(axis=0).astype(np.float64)
    mid, ext = (lo + hi) / 2, float((hi - lo).max())
    rng = np.random.default_rng(1)
    kw = dict(friction=0.5, restitution=0.0)
    clear = [collider_ref.sphere(hi + 10.0 * ext, 0.25 * ext, **kw)]
    middle = [collider_ref.sphere(mid, 0.31 * ext, **kw)]                                         # 4/3 pi 0.31^3 = an eighth of the cube
    sixteen = [collider_ref.sphere(lo + (hi - lo) * rng.uniform(0.15, 0.85, size=3), 0.08 * ext, **kw) for _ in range(16)]
    legs = {"1_no_call": (None, None), "2_collide_clear": ("collide", clear), "3_reactions_clear": ("reactions", clear),
            "4_collide_middle": ("collide", middle), "5_reactions_middle": ("reactions", middle), "6a_collide_sixteen": ("collide", sixteen),
            "6b_reactions_sixteen": ("reactions", sixteen), "7_reactions_middle_fetch_every_tick": ("reactions+fetch", middle)}
    if a.collide_only:
        legs = {k: v for k, v in legs.items() if v[0] in (None, "collide")}
    if a.only:
        legs = {a.only: legs[a.only]}
    res = {"tool": "collider_reaction_bench", "ticks": a.ticks, "repeats": a.repeats, "substeps": a.substeps, "particles": int(mesh.n),
           "collide_only": bool(a.collide_only),
           "timing": "ms per tick: HIP events on the rank's stream and wall clock around the loop (legs 1-7, each in a fresh group), wall clock (leg 8); per call (alone)",
           "clocks_before": _clocks()}
    dev, wall, fused, alone, hit_particles, hit_groups = {}, {}, {}, {}, {}, {}
    for name, (how, what) in legs.items():
        g = SoftbodyGroup(mesh, [0], substeps=a.substeps).Start()
        try:
            r0 = g.rank(0)
            items = [to_native(c) for c in what] if what else None

            def call():
                if how == "collide":
                    g.collide(items)
                elif how is not None:
                    g.collide_with_reactions(items)
                    if how == "reactions+fetch":
                        g.collider_reactions()

            def run(ticks):
                for _ in range(ticks):
                    call()
                    g.step()
            run(WARM_TICKS + 1); g.synchronize()
            if a.only:
                run(a.ticks); g.synchronize()
                continue
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
            if how in ("collide", "reactions"):                  # the call alone, on a completed tick
                alone[name] = []
                for k in range(a.repeats + 2):
                    g.step(); x = g.get_positions(); g.get_velocities()
                    if k == 0:
                        v = g.get_velocities()
                        hit = collider_ref.apply(x.copy(), v.copy(), np.asarray(mesh.inv_mass, np.float32), what).any(axis=0)
                        hit_particles[name] = int(hit.sum())
                        rows = -(-mesh.n // WORKGROUP)
                        hit_groups[name] = int(np.add.reduceat(hit, np.arange(rows) * WORKGROUP).astype(bool).sum())      # (caller order: an estimate of device order)
                    r0.profile_begin(); call(); alone[name].append(r0.profile_end())
                alone[name] = alone[name][2:]
        finally:
            g.OnDestroy()
    if a.only:
        return
    res["legs_device_ms_per_tick"] = {k: _stat(v) for k, v in dev.items()}
    res["legs_wall_ms_per_tick"] = {k: _stat(v) for k, v in wall.items()}
    res["ticks_fused_per_leg"] = fused
    med = {k: res["legs_device_ms_per_tick"][k]["median"] for k in legs}
    res["added_device_ms_per_tick_over_no_call"] = {k: med[k] - med["1_no_call"] for k in legs if k != "1_no_call"}
    if not a.collide_only:
        pairs = (("2_collide_clear", "3_reactions_clear"), ("4_collide_middle", "5_reactions_middle"), ("6a_collide_sixteen", "6b_reactions_sixteen"))
        res["reactions_minus_collide_device_ms_per_tick"] = {
            b: {"difference": med[b] - med[c], "margin_spread_of_either": max(res["legs_device_ms_per_tick"][b]["spread"], res["legs_device_ms_per_tick"][c]["spread"])}
            for c, b in pairs}
    res["alone_device_ms"] = {k: _stat(v) for k, v in alone.items()}
    res["particles_hit_at_the_first_lone_call"] = hit_particles
    rows = -(-mesh.n // WORKGROUP)
    model = {}
    for k in alone:
        model[k] = 16 * mesh.n + 36 * hit_particles[k]
        if legs[k][0] == "reactions":
            model[k] += 2 * 4 * rows + 2 * 1024 * hit_groups[k]
    res["workgroups_with_a_hit_estimate"] = hit_groups
    res["model_bytes_floor"] = model
    res["model_gb_per_s"] = {k: model[k] / (res["alone_device_ms"][k]["median"] * 1e-3) / 1e9 for k in model}
    if not a.skip_replaced_route and not a.collide_only:
        g = SoftbodyGroup(mesh, [0], substeps=a.substeps).Start()
        try:
            x = np.zeros((mesh.n, 3), np.float32); vb = np.zeros((mesh.n, 3), np.float32); va = np.zeros((mesh.n, 3), np.float32)
            m = 1.0 / np.ascontiguousarray(mesh.inv_mass, np.float64)
            items = [to_native(c) for c in middle]
            centre = np.asarray(middle[0]["a"], np.float64)
            ticks8 = max(2, a.ticks // 10)
            ms = []
            for rep in range(3):
                g.synchronize()
                t0 = time.perf_counter()
                for t in range(ticks8):
                    g.get_velocities(vb)
                    g.collide(items)
                    g.get_velocities(va); g.get_positions(x)
                    touched = np.nonzero((vb != va).any(axis=1))[0]      # (the route cannot even see a separating contact)
                    j = m[touched, None] * (vb[touched].astype(np.float64) - va[touched])
                    out = (j.sum(axis=0), np.cross(x[touched] - centre, j).sum(axis=0), m[touched].sum(), touched.size)
                    g.step()
                g.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3 / ticks8)
            assert out[3] >= 0
            res["8_replaced_route_wall_ms_per_tick"] = {"all": _stat(ms[1:]), "ticks": ticks8, "colliders": 1,
                                                        "bytes_over_pcie": {"get_velocities": 2 * 12 * mesh.n, "get_positions": 12 * mesh.n}}
            res["wall_ms_per_tick_vs_replaced_route"] = {"7_reactions_middle_fetch_every_tick": res["legs_wall_ms_per_tick"]["7_reactions_middle_fetch_every_tick"]["median"],
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
