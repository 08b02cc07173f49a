"""The two CPU restatements of SPEC.md on the inputs of tests/float_range_cases.py: tets and hinges over the whole binary32 range of
scales with exact degeneracies (every skip predicate of SPEC.md 5 and 6 false and true), and free particles whose state is subnormal.
oracle.c and oracle_np.NumpySolver must agree bit for bit there as they do on ordinary meshes, and the inputs must do what
tests/test_gpu_float_range.py relies on: stay finite, move where L^4 is representable, rest where it is not, keep subnormal state subnormal.

The constraints of a case share no particle, so every order is the same sweep: the C oracle walks its natural order, the numpy solver
takes one class per constraint type.

Measured (seeds 5, 6, 7; `pytest -s` prints them): share of the constraints with -34 < e < 26 and a free particle that moved, rigid:
tets 0.982 .. 0.987, hinges 0.988 .. 0.992, springs 1.0 (required: 0.95); share of the free particles of the subnormal case that end with
a subnormal coordinate: x 0.944 .. 0.947, v 0.887 .. 0.899 (required: 0.8); no output is non-finite.
"""
import numpy as np
import pytest

import float_range_cases as frc
from oracle import oracle_np
from helpers import build_plan, make_oracle

SEEDS = (5, 6, 7)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _numpy_solver(mesh, gravity, damping=0.0, compliance=(0.0, 0.0, 0.0), plane=None):
    p = oracle_np.NumpySolver(mesh.pos, mesh.vel, mesh.inv_mass, gravity, damping)
    if len(mesh.dist_rest):
        p.set_distance(mesh.dist_ij, mesh.dist_rest, compliance[0])
    if len(mesh.vol_rest):
        p.set_volume(mesh.vol_ijkl, mesh.vol_rest, compliance[1])
    if len(mesh.bend_rest):
        p.set_bending(mesh.bend_ijkl, mesh.bend_rest, compliance[2])
    if plane is not None:
        p.set_ground_plane(plane[:3], plane[3])
    counts = [len(mesh.dist_rest), len(mesh.vol_rest), len(mesh.bend_rest)]
    types = np.repeat(np.arange(3, dtype=np.uint8), counts)
    ids = np.concatenate([np.arange(c) for c in counts]).astype(np.int32)
    p.set_classes(types, ids, np.concatenate([[0], np.cumsum(counts)]))       # one class per constraint type
    return p


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("compliance", list(frc.COMPLIANCES))
@pytest.mark.parametrize("name", frc.SWEEP_CASES)
def test_oracles_agree_on_tets_and_hinges_across_the_float_range(oracle_mod, name, compliance, seed):
    mesh = frc.case(name, seed)
    comp = frc.COMPLIANCES[compliance]
    c = make_oracle(oracle_mod, mesh, None, gravity=frc.NO_GRAVITY, compliance=comp)
    p = _numpy_solver(mesh, frc.NO_GRAVITY, compliance=comp)
    with np.errstate(all="ignore"):          # (L^4 overflows on purpose)
        for _ in range(frc.SWEEP_TICKS):
            c.step(frc.DT, frc.SWEEP_SUBSTEPS); p.step(frc.DT, frc.SWEEP_SUBSTEPS)
    assert np.array_equal(_bits(c.x), _bits(p.x)), frc.describe_mismatch(mesh, p.x, c.x, "numpy x against C x")
    assert np.array_equal(_bits(c.v), _bits(p.v)), frc.describe_mismatch(mesh, p.v, c.v, "numpy v against C v")
    assert np.isfinite(c.v).all()
    shares = frc.check_sweep_conditions(mesh, c.x, rigid=compliance == "rigid")
    print(f"{name} seed {seed} {compliance}: moved share of the constraints in range " + ", ".join(f"{u.kind} {s:.4f}" for u, s in zip(mesh.units, shares)))


def test_every_skip_predicate_is_reached_by_the_degenerate_rows():
    # the exact degeneracies are what they claim to be, in binary32, whatever the scale did to them
    for name in ("vol", "bend"):
        mesh = frc.case(name)
        u = mesh.units[0]
        x = mesh.pos[u.particles]
        assert np.array_equal(x[0:16, 1], x[0:16, 0]) and np.array_equal(x[32:48, 3], x[32:48, 0]) and not x[48:64, :, 2].any()
        assert frc.n_degenerate(len(u.e)) == 64 and (u.row_class[:64] == 0).all() and set(u.row_class[64:]) == {1, 2, 3}
        pinned = (mesh.inv_mass[u.particles] == 0).all(axis=1)
        assert pinned.sum() >= 4          # den = 0 at zero compliance, den = at with compliance


def test_mixed_case_has_groups_with_springs_tets_and_hinges_side_by_side():
    # the planner (host only) on the mixed mesh at the solver's default tile size: around the origin, where the scales meet, tiles hold
    # groups of all three types -- hinge rows, tet quads and spring lanes of one tile kernel step side by side
    plan = build_plan(frc.case("mixed"), tile_particles=0)
    types, _ = plan.order(0)
    groups = plan.groups(0)
    kinds = [set(types[a:b].tolist()) for a, b in zip(groups[:-1], groups[1:])]
    assert sum(k == {0, 1, 2} for k in kinds) >= 1 and not any(p["kind"] == 0 for p in plan.phases(0))


@pytest.mark.parametrize("seed", SEEDS)
def test_oracles_agree_on_subnormal_particles(oracle_mod, seed):
    mesh = frc.case("subnormal", seed)
    run = frc.SUBNORMAL_RUN
    c = make_oracle(oracle_mod, mesh, None, gravity=run["gravity"], damping=run["damping"], ground_plane=run["ground_plane"])
    p = _numpy_solver(mesh, run["gravity"], damping=run["damping"], plane=run["ground_plane"])
    with np.errstate(all="ignore"):          # (underflow is the point)
        for _ in range(run["ticks"]):
            c.step(frc.DT, run["substeps"]); p.step(frc.DT, run["substeps"])
    assert np.array_equal(_bits(c.x), _bits(p.x)), frc.describe_mismatch(mesh, p.x, c.x, "numpy x against C x")
    assert np.array_equal(_bits(c.v), _bits(p.v)), frc.describe_mismatch(mesh, p.v, c.v, "numpy v against C v")
    sx, sv = frc.check_subnormal_conditions(mesh, c.x, c.v)
    print(f"subnormal seed {seed}: share of the free particles with a subnormal coordinate: x {sx:.4f}, v {sv:.4f}")
    # the plane was met from below: some free particle was lifted back to y = 0 by a subnormal penetration
    assert (c.x[mesh.inv_mass > 0, 1] >= 0).all() and (mesh.vel[mesh.inv_mass > 0, 1] < 0).any()
