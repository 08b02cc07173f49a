"""Which solvers run the lean coded tile kernels (softbodyunity_amd/csrc/launch_shape.hpp use_lean_coded), checked on the CPU:
tests/sanitize/lean_rule_check.cpp walks a cross product of tiling scalars and solver inputs -- lean implies previous-position codes;
any unpacked tile in either tiling, a program above kRegRoundsNarrow, a halo slot, world > 1 or a T2 layer each switch it off; an empty
second tiling does not -- and the LDS a lean launch asks for. The number of points is counted here independently: the driver may skip none."""
import itertools
import os
import subprocess

from test_tables_digest import CSRC, FLAGS, SAN


def _points():
    n = 0
    for n0, n1, miss0, miss1, lanes0, lanes1, rounds, world, halo, between, wpal, tile_lanes in itertools.product(
            range(3), (0, 1, 32778), (0, 1), (0, 1), range(3), range(3), range(4), (1, 2), (0, 1), (0, 1), (0, 1), range(3)):
        if miss1 and n1 == 0:
            continue
        n += 1
    return n


def test_the_lean_rule_implies_codes_and_every_tile_lane_packed(tmp_path):
    exe = os.path.join(str(tmp_path), "lean_rule_check")
    subprocess.check_call(["g++", *FLAGS, "-Werror", "-I", CSRC, os.path.join(SAN, "lean_rule_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = dict(line.split() for line in out.stdout.splitlines())
    assert int(got["points"]) == _points() > 0
    assert 0 < int(got["lean"]) < int(got["points"])
