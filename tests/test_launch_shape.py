"""Which tile_kernel instantiation a launch runs (softbodyunity_amd/csrc/launch_shape.hpp), checked on the CPU:
tests/sanitize/launch_shape_check.cpp walks the whole cross product of tiling scalars, tuning values and launch sizes and compares
every point with the rule as it stood inside launch_tile before it became a function (transcribed into the driver), checks the
contract the table builder and the kernel rely on, and that every shape the kernels are built for is reached. The number of points
is counted here independently: the driver may skip none."""
import itertools
import os
import subprocess

from test_tables_digest import CSRC, FLAGS, SAN


def _points():
    n = 0
    for max_local, has_quads, packed, tile_lanes, quad_lanes, nmt, ghosts in itertools.product(
            (1, 512, 513, 1024), (0, 1), (0, 128, 256), (0, 128, 256, 512), (256, 512), (1, 769, 10240), (0, 1)):
        if packed and not (max_local <= 512 and not has_quads):
            continue
        if ghosts and has_quads:
            continue
        n += sum(1 for k in (1, 768, 769, nmt - 1, nmt, 40000) if k > 0)
    return n


def test_the_launch_shape_equals_the_parents_rule_and_keeps_the_contract(tmp_path):
    exe = os.path.join(str(tmp_path), "launch_shape_check")
    subprocess.check_call(["g++", *FLAGS, "-Werror", "-I", CSRC, os.path.join(SAN, "launch_shape_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = dict(line.split() for line in out.stdout.splitlines())
    assert int(got["points"]) == _points() > 0
    assert int(got["shapes"]) == 9      # (128,4) (256,2) (256,4) (512,1) with and without quads, (512,2) with quads
