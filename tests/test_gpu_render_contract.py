"""The render API answers a user exactly as it did when tests/golden/render_contract.json was recorded (tests/golden/make_render_contract.py,
ahead of the move of the render readback into csrc/render.hip): every refusal of sb_readback_* / sb_set_render_* / sb_set_readback_* and of
their sb_group_* twins -- null and bad arguments, calls out of order, the two render modes excluding each other, getters with nothing
finished or the wrong mode, UV and embedding argument checks, what a rank of a partitioned solver refuses -- with its status code and
the WHOLE sb_last_error text (the other tests look at fragments), and a solver's sb_stats.device_bytes after each step of a fixed sequence
of render modes, as deltas from its value right after Start(). The walk itself is tests/render_contract_case.py."""
import json
import os

import pytest

import render_contract_case as case

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_contract.json")) as f:
    GOLDEN = json.load(f)


def _same(got, want, where):
    assert sorted(got) == sorted(want), where
    for part in want:
        g, w = got[part], want[part]
        if isinstance(w, dict):
            _same(g, w, f"{where}.{part}")
            continue
        for k, (a, b) in enumerate(zip(g, w)):
            assert a == b, f"{where}.{part}[{k}]: got {a}, recorded {b}"
        assert len(g) == len(w), f"{where}.{part}: {len(g)} entries, recorded {len(w)}"


def test_a_solver_refuses_in_the_recorded_words_and_holds_the_recorded_device_memory():
    got = case.solver_contract()
    for body in ("cube8", "tets"):
        for step, (what, delta) in enumerate(got[body]["device_bytes"]):
            print(f"{body} device_bytes after {what}: {delta:+d} (recorded {GOLDEN['solver'][body]['device_bytes'][step][1]:+d})")
    _same(got, GOLDEN["solver"], "solver")


@pytest.mark.parametrize("host", ["threads", "walk"])
def test_a_group_of_two_ranks_refuses_in_the_recorded_words(host):
    _same(case.run_group(host), GOLDEN["group"], f"group[{host}]")
