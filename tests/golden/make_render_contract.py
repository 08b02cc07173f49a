"""Records tests/golden/render_contract.json on a GPU: what tests/render_contract_case.py's walk over the render API gives with the
library that is built now -- every refusal's status code and whole sb_last_error text, for a solver and for a group of two ranks, and the
solver's sb_stats.device_bytes deltas along the fixed sequence of render modes. tests/test_gpu_render_contract.py only reads the file.

Record it BEFORE a change that is meant to leave all of this alone (first recorded ahead of moving the render readback into render.hip),
and again only when a text, a status code or an allocation is changed on purpose:

    python tests/golden/make_render_contract.py
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_contract_case as case  # noqa: E402

OUT = os.path.join(HERE, "render_contract.json")


def main():
    table = {"solver": case.solver_contract()}
    groups = {}
    for host in ("threads", "walk"):
        groups[host] = case.run_group(host)
    if groups["threads"] != groups["walk"]:
        raise SystemExit("the two group hosts answer differently: nothing written")
    table["group"] = groups["threads"]
    with open(OUT, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    n = sum(len(v["calls"]) if isinstance(v, dict) else len(v) for part in table.values() for v in part.values())
    print(f"{OUT}: {n} calls recorded")


if __name__ == "__main__":
    main()
