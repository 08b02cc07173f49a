"""Every launch shape of the tile kernel (csrc/launch_shape.hpp: 128 x 4, 256 x 2, 256 x 4, 512 x 1, 512 x 2 lanes x particles per lane, with and
without tets / hinges, with and without ghosts read from the receive buffer) on the smallest meshes that reach it: 2 ticks of 3 substeps,
positions and velocities bitwise against the oracle. Which shape a case asks for is the rule tests/test_launch_shape.py pins on the CPU;
a launch at another width than the tables were built for decodes a window that was never staged, i.e. gives other bits.
(kKindPeek with a descriptor table and kKindMidKinematic run at forced widths in test_gpu_peek.py and test_gpu_kinematic.py.)"""
import numpy as np
import pytest

from helpers import build_plan, make_oracle
from softbodyunity_amd import Softbody, comm_unique_id, native
from softbodyunity_amd.mesh import bunny_surrogate, jelly_cube

pytestmark = pytest.mark.gpu
TICKS, SUBSTEPS, DT = 2, 3, 0.02
TET_COMPLIANCE = (1e-7, 1e-7, 1e-5)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _set(monkeypatch, name, value):
    if value:
        monkeypatch.setenv(name, value)
    else:
        monkeypatch.delenv(name, raising=False)


def _largest_tile(mesh, plan):
    """most particles the constraints of one T0 / T1 tile touch (a device tile holds at least those)"""
    cons = (mesh.dist_ij, mesh.vol_ijkl, mesh.bend_ijkl)
    worst = 0
    for parity in (0, 1):
        t, ids = plan.order(parity)
        tasks, off = plan.tasks(parity), plan.phase_task_offsets(parity)
        for k, ph in enumerate(plan.phases(parity)):
            if ph["kind"] not in (1, 2):
                continue
            for q in range(off[k], off[k + 1]):
                b, e = tasks[q], tasks[q + 1]
                touched = [cons[ty][ids[b:e][t[b:e] == ty]].ravel() for ty in range(3)]
                worst = max(worst, len(np.unique(np.concatenate(touched))))
    return worst


@pytest.fixture(scope="module")
def reference(oracle_mod):
    """(mesh, tile_particles, compliance) -> the oracle's state after the ticks, its plan's largest tile; computed once per key"""
    meshes = {"cube10": jelly_cube(10), "cube12": jelly_cube(12), "tets": bunny_surrogate(target_verts=2000, seed=9)}
    done = {}

    def get(name, tile, compliance=(0.0, 0.0, 0.0)):
        if (name, tile) not in done:
            mesh = meshes[name]
            plan = build_plan(mesh, tile_particles=tile)
            o = make_oracle(oracle_mod, mesh, plan, compliance=compliance)
            for _ in range(TICKS):
                o.step(DT, SUBSTEPS)
            done[name, tile] = (mesh, o.x.copy(), o.v.copy(), _largest_tile(mesh, plan))
        return done[name, tile]
    return get


def _run(mesh, tile, compliance=(0.0, 0.0, 0.0), **kw):
    sb = Softbody(mesh, substeps=SUBSTEPS, fixed_delta_time=DT, tile_particles=tile, distance_compliance=compliance[0],
                  volume_compliance=compliance[1], bending_compliance=compliance[2], **kw).Start()
    try:
        for _ in range(TICKS):
            sb.FixedUpdate(readback=False)
        owned = sb.owner() == 0 if kw.get("world", 1) > 1 else slice(None)
        return sb.get_positions()[owned].copy(), sb.get_velocities()[owned].copy(), sb.stats()
    finally:
        sb.OnDestroy()


@pytest.mark.parametrize("lanes", ["", "128", "256"])
def test_spring_tiles_at_512_128_and_256_lanes(reference, monkeypatch, lanes):
    # 10^3 cube in 64-particle tiles: a few dozen small spring-only tiles per launch -> 512 x 1 by launch size, 128 x 4 and 256 x 2 forced
    _set(monkeypatch, "SB_TILE_LANES", lanes)
    mesh, want_x, want_v, largest = reference("cube10", 64)
    x, v, st = _run(mesh, 64)
    assert largest <= 512 and st["n_tiles"][0] <= 768
    assert np.array_equal(_bits(x), _bits(want_x)) and np.array_equal(_bits(v), _bits(want_v))


def test_large_spring_tiles_at_256_lanes_4_particles_per_lane(reference, monkeypatch):
    _set(monkeypatch, "SB_TILE_LANES", "")
    mesh, want_x, want_v, largest = reference("cube12", 1024)
    assert 512 < largest <= 1024      # some tile is a large tile: every launch of its tiling runs 256 x 4
    x, v, st = _run(mesh, 1024)
    assert np.array_equal(_bits(x), _bits(want_x)) and np.array_equal(_bits(v), _bits(want_v))


@pytest.mark.parametrize("quad_lanes", ["256", "512"])
@pytest.mark.parametrize("tile", [256, 1024])
def test_tiles_with_tets_and_hinges_at_256_and_512_lanes_small_and_large(reference, monkeypatch, quad_lanes, tile):
    # 256 x 2 and 256 x 4 with quads (SB_QUAD_LANES=256), 512 x 1 and 512 x 2 (512)
    _set(monkeypatch, "SB_TILE_LANES", "")
    _set(monkeypatch, "SB_QUAD_LANES", quad_lanes)
    mesh, want_x, want_v, largest = reference("tets", tile, TET_COMPLIANCE)
    assert len(mesh.vol_rest) and len(mesh.bend_rest)
    assert largest <= 512 if tile == 256 else 512 < largest <= 1024
    x, v, st = _run(mesh, tile, TET_COMPLIANCE)
    assert np.array_equal(_bits(x), _bits(want_x)) and np.array_equal(_bits(v), _bits(want_v))


@pytest.mark.parametrize("lanes", ["", "128", "256"])
def test_ghost_reading_tiles_at_512_128_and_256_lanes(monkeypatch, lanes):
    # rank 0 of two, every peer the rank itself (loopback: no oracle for that state): the T1 kernels read their ghosts from the receive
    # buffer (fused unpack) -- the same run with the unpack kernel in front of them instead must give the same bits
    _set(monkeypatch, "SB_TILE_LANES", lanes)
    mesh = jelly_cube(10)

    def run(fused):
        _set(monkeypatch, "SB_NO_FUSED_UNPACK", "" if fused else "1")
        return _run(mesh, 64, device=0, rank=0, world=2, unique_id=comm_unique_id(), halo_schedule=native.SB_SCHEDULE_SERIAL_EAGER,
                    debug_flags=native.SB_DEBUG_LOOPBACK)
    xa, va, sa = run(True)
    xb, vb, sb_ = run(False)
    assert sa["halo_unpack_fused"] == 1 and sb_["halo_unpack_fused"] == 0 and sa["halo_particles_t1"] > 0
    assert np.array_equal(_bits(xa), _bits(xb)) and np.array_equal(_bits(va), _bits(vb))
