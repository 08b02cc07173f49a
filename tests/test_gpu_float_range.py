"""The five device forms of the tet and hinge projections (softbodyunity_amd/csrc/device_math.hip.hpp) on the inputs of
tests/float_range_cases.py, bitwise against the C oracle on the solver's own plan: scales 2^-44 .. 2^40 (dot(g, g), q1, q2 ~ L^4 subnormal,
zero and infinite), coincident hinge edges, wings on the edge, flat and four times pinned tets, with and without compliance -- what
test_spring_lengths_across_the_float_range does for springs. And the state itself subnormal (SPEC.md 1: denormals preserved) through
integrate, collide and velocity of the tile kernels. tests/test_float_range_oracles.py checks the same inputs on the CPU.

Which form a configuration reaches (no stat tells the wave items from the generic loop; the engines are the three branches of
tile_kernel.hip.hpp titled "engine 1, register-resident rounds", "engine 2, wave items" and "engine 3, windowed group walk"):
  items     default                  engine 2, wave items (`QUADS && kTileThreads == 64 * A.item_waves && td.n_steps > 0 && d_hi - d_lo <= win`):
                                     project_bending_row for kItemBending, project_volume_quad for kItemVolume; 512-lane workgroups
                                     (schedule.hip launch_tile: quad8)
  items256  SB_QUAD_LANES=256        the same engine in 4-wave workgroups (item_waves = 4)
  groups    SB_NO_WAVE_ITEMS=1       no items in the stream (n_steps = 0, item_waves = 0): engine 3, windowed group walk, its
                                     `if (QUADS)` part: project_bending_quad / project_volume_quad by wave slot
  window    SB_WIN_DWORDS=1024       the window of every tiling is set to 1024 dwords (tables_host.cpp tiling_limits). The constraints here
                                     are independent, so a workgroup holds a pack of at most 16 four-particle components, 64 dwords of
                                     slots: every pack fits, the window refill of engine 3 is NOT taken and the wave items run over another LDS
                                     carve. Refills of the generic loop are reached by test_hub_with_tets_and_hinges_walks_more_than_64_steps,
                                     at ordinary scales only.
  global    tile_particles=-1        no tile holds a constraint: global_quad_kernel (aux_kernels.hip.hpp) with the one-lane project_volume /
                                     project_bending, global_distance_kernel for the springs; n_global_colours > 0 says so

The planner cuts space by rest positions, and the scales here differ by 2^84: nearly every constraint is a connected component of its
own and goes to the T2 layers (kKindLayer of the tile kernel), a few hundred share T0 / T1 tiles around the origin (mixed: springs, tets and
hinges in one group there). Either way the engine above is the one that projects them.
"""
import numpy as np
import pytest

import float_range_cases as frc
from softbodyunity_amd import Softbody
from helpers import make_oracle

pytestmark = pytest.mark.gpu

CONFIGS = {          # id -> (environment switches read by native.tuning_from_env, tile_particles)
    "items": ({}, 0),
    "items256": ({"SB_QUAD_LANES": "256"}, 0),
    "groups": ({"SB_NO_WAVE_ITEMS": "1"}, 0),
    "window": ({"SB_WIN_DWORDS": "1024"}, 0),
    "global": ({}, -1),
}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(oracle_mod, mesh, ticks, substeps, tile, compliance=(0.0, 0.0, 0.0), gravity=frc.NO_GRAVITY, damping=0.0, ground_plane=None):
    """-> (x, v, oracle x, oracle v, stats) after `ticks` ticks on the GPU and on the C oracle walking the solver's own plan."""
    sb = Softbody(mesh, substeps=substeps, fixed_delta_time=frc.DT, gravity=gravity, damping=damping, distance_compliance=compliance[0],
                  volume_compliance=compliance[1], bending_compliance=compliance[2], tile_particles=tile, ground_plane=ground_plane).Start()
    try:
        o = make_oracle(oracle_mod, mesh, sb.plan(), gravity=gravity, damping=damping, compliance=compliance, ground_plane=ground_plane)
        for _ in range(ticks):
            sb.step(); o.step(frc.DT, substeps)
        return sb.get_positions(), sb.get_velocities(), o.x, o.v, sb.stats()
    finally:
        sb.OnDestroy()


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("compliance", list(frc.COMPLIANCES))
@pytest.mark.parametrize("name", frc.SWEEP_CASES)
def test_tets_and_hinges_across_the_float_range(oracle_mod, monkeypatch, name, compliance, config):
    env, tile = CONFIGS[config]
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    mesh = frc.case(name)
    x, v, ox, ov, st = _run(oracle_mod, mesh, frc.SWEEP_TICKS, frc.SWEEP_SUBSTEPS, tile, compliance=frc.COMPLIANCES[compliance])
    if config == "global":
        assert st["n_global_colours"] > 0 and st["constraints_in_tiles"] == 0
    else:
        assert st["n_global_colours"] == 0 and st["constraints_in_global"] == 0
    assert np.array_equal(_bits(x), _bits(ox)), frc.describe_mismatch(mesh, x, ox, "GPU x against the oracle")
    assert np.array_equal(_bits(v), _bits(ov)), frc.describe_mismatch(mesh, v, ov, "GPU v against the oracle")
    assert np.isfinite(v).all()
    frc.check_sweep_conditions(mesh, x, rigid=compliance == "rigid")


@pytest.mark.parametrize("tile", [512, -1])
def test_subnormal_positions_and_velocities_are_preserved(oracle_mod, tile):
    mesh = frc.case("subnormal")
    run = frc.SUBNORMAL_RUN
    x, v, ox, ov, _ = _run(oracle_mod, mesh, run["ticks"], run["substeps"], tile, gravity=run["gravity"], damping=run["damping"],
                           ground_plane=run["ground_plane"])
    assert np.array_equal(_bits(x), _bits(ox)), frc.describe_mismatch(mesh, x, ox, "GPU x against the oracle")
    assert np.array_equal(_bits(v), _bits(ov)), frc.describe_mismatch(mesh, v, ov, "GPU v against the oracle")
    frc.check_subnormal_conditions(mesh, x, v)
