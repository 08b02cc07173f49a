#!/usr/bin/env python3
"""Randomised differential test of FRAME SEQUENCES: the open-ended form of tests/test_gpu_frame_sequences.py. Every seed is a scenario of
tests/frame_sequence_cases.py -- a small body, a render mode, and a script that interleaves every between-tick call of the group API
(impulses, placement, surface forces, collider, heightfield and signed-distance contacts with the tables' set / replace / clear, reactions,
state queries, kinematic moves, readbacks, ray casts, closest points) with ticks of changing shape -- walked on a SoftbodyGroup of one rank and on the CPU oracle with the tests/*_ref.py
modules; every observation is compared under its rule, the sb_stats counters against the counter model. Seeds 0 .. 279 are the fixed
slice pytest runs (0 .. 199 its first block, generated without a signed-distance step; every seed from 200 on draws them too); the default
start lies behind them.

One child process per batch of scenarios. The child exits on the first HIP error, and after a child that died abnormally the parent
starts nothing further (a GPU fault is a finding to read, not to run again).
usage: python tests/fuzz/fuzz_frames.py [--seconds 240] [--seed 1000] [--max N] [--only SEED] [--batch 40]"""
import argparse
import os
import subprocess
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def describe(sc):
    return ", ".join(f"{k}={v}" for k, v in sc.items() if k != "script") + f", {len(sc['script'])} steps"


def run(sc):
    """-> (verdict, detail): OK / MISMATCH / ERROR; raises native.SoftbodyError for a HIP error (the child ends there)"""
    import frame_sequence_cases as fc
    from oracle import oracle
    from softbodyunity_amd import native
    want = fc.run_reference(oracle, sc)
    try:
        g = fc.open_group(sc)
        try:
            got = fc.run_group(g, sc)
        finally:
            g.OnDestroy()
    except native.SoftbodyError as e:
        if e.code == native.SB_ERR_HIP:
            raise
        return "ERROR", str(e)[:300]
    bad = fc.first_mismatch(want, got)
    if bad:
        return "MISMATCH", fc.report(sc, want, got, *bad, command=f"python tests/fuzz/fuzz_frames.py --only {sc['seed']}").replace("\n", "\n            ")
    return "OK", ""


def child(a):
    """Scenarios in THIS process until the batch or the time is up; one line before and one after each (the parent tells a crash from the
    missing second)."""
    import frame_sequence_cases as fc
    from oracle import oracle
    from softbodyunity_amd import native
    oracle.build()
    t_end = time.time() + a.seconds
    for seed in range(a.seed, a.seed + a.max):
        if time.time() > t_end:
            break
        sc = fc.make_scenario(seed)
        print(f"START {seed} {describe(sc)}", flush=True)
        t0 = time.time()
        try:
            verdict, detail = run(sc)
        except native.SoftbodyError as e:      # a HIP error: nothing more is started on this device from here
            print(f"DONE {seed} ERROR {time.time() - t0:.1f}s HIP error, the child ends here: {str(e)[:300]}".replace("\n", " "), flush=True)
            sys.exit(3)
        except Exception as e:                 # a bug of the harness: report, go on
            verdict, detail = "ERROR", f"{type(e).__name__}: {e} | {traceback.format_exc().splitlines()[-3:]}"
        print(f"DONE {seed} {verdict} {time.time() - t0:.1f}s " + detail.replace("\n", "\\n"), flush=True)
    print("END", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--only", type=int, default=None)
    ap.add_argument("--max", type=int, default=10 ** 9)
    ap.add_argument("--batch", type=int, default=40)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    t_end = time.time() + a.seconds
    tally, n = {}, 0
    seed = a.only if a.only is not None else a.seed
    last = seed + (1 if a.only is not None else a.max)
    stopped = ""
    while seed < last and time.time() < t_end and not stopped:
        cmd = [sys.executable, "-X", "faulthandler", os.path.abspath(__file__), "--child", "--seed", str(seed), "--max", str(min(a.batch, last - seed)),
               "--seconds", str(max(1.0, t_end - time.time()))]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        started, desc, ended = None, "", False
        for line in p.stdout:
            line = line.rstrip("\n")
            if line.startswith("START "):
                _, sd, desc = line.split(" ", 2); started = int(sd)
            elif line.startswith("DONE "):
                _, sd, verdict, secs, *rest = line.split(" ", 4)
                detail = rest[0].replace("\\n", "\n            ") if rest else ""
                tally[verdict] = tally.get(verdict, 0) + 1; n += 1
                print(f"{verdict:8s} {secs:>6s}  {desc}" + (f"\n         -> {detail}" if detail else ""), flush=True)
                seed = int(sd) + 1; started = None
            elif line == "END":
                ended = True
        err = p.stderr.read()
        rc = p.wait()
        if started is not None:      # died inside a scenario
            tally["CRASH"] = tally.get("CRASH", 0) + 1; n += 1
            print(f"CRASH    rc={rc}  {desc}\n         -> {err[-1500:]}", flush=True)
            stopped = f"a child died inside seed {started} (rc {rc})"
        elif rc != 0 or not ended:
            stopped = f"a child ended with rc {rc}: {err[-800:]}"
    if stopped:
        print(f"fuzz_frames: nothing further is started: {stopped}", flush=True)
    print(f"SUMMARY {n} scenarios: " + ", ".join(f"{k} {v}" for k, v in sorted(tally.items())), flush=True)
    return 1 if (stopped or tally.get("MISMATCH", 0) or tally.get("ERROR", 0) or tally.get("CRASH", 0)) else 0


if __name__ == "__main__":
    sys.exit(main())
