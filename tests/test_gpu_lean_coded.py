"""The lean coded tile kernels (csrc/tile_kernel.hip.hpp LEAN; launch_shape.hpp use_lean_coded says who runs them): a single-rank spring
lattice with previous-position codes whose every device tile, in both tilings, is lane-packed -- the configuration of the 256^3 headline.
Small cubes are forced onto the narrow launch (SB_NARROW_MIN_TILES=1) as in test_gpu_prev_code.py. Cubes whose edge is a multiple of 8,
the tile's edge, have rim packs of the headline's kinds. Every case is bitwise against the oracle, positions and velocities after every
tick, with the table validator clean, and asserts what the rule reads: lane_packed_tiles == n_tiles in both tilings, coded by launch_bytes.
A launch with one inverse mass runs the uniform-mass kernels (first, mid, last); palettes of several masses, pinned particles among them,
run the palette kernels (first, mid, last, mid-kinematic)."""
import numpy as np
import pytest

from helpers import make_oracle
from softbodyunity_amd import Softbody, jelly_cube
from test_gpu_prev_code import DT, _bits, _coded, _escapes, _handoffs, _narrow

pytestmark = pytest.mark.gpu


def _all_packed(st):
    return all(st["n_tiles"][tl] > 0 and st["lane_packed_tiles"][tl] == st["n_tiles"][tl] for tl in (0, 1))


def _run(oracle_mod, mesh, kw, ticks=4, pos_only=(1,), lean=True, before_tick=None, state=None):
    """`ticks` ticks against the oracle, bit for bit after every tick: positions and velocities, or -- after the ticks in pos_only --
    positions alone, which leaves the tick's last kernel held back (peek), so that the next tick starts with the fused kernel"""
    sb = Softbody(mesh, **kw).Start()
    try:
        st = sb.stats()
        assert _coded(st), st["launch_bytes"]
        assert lean is None or _all_packed(st) == lean, (st["lane_packed_tiles"], st["n_tiles"])
        if state is not None:
            sb.set_state(*state)
            mesh.pos, mesh.vel = state
        okw = {k: v for k, v in kw.items() if k in ("ground_plane", "damping")}
        o = make_oracle(oracle_mod, mesh, sb.plan(), **okw)
        for t in range(ticks):
            if before_tick:
                before_tick(t, sb, o)
            sb.step(); o.step(DT, kw["substeps"])
            if t in pos_only:
                assert np.array_equal(_bits(sb.get_positions()), _bits(o.x)), f"positions after tick {t}"
            else:
                x, v = sb.get_positions(), sb.get_velocities()
                assert np.array_equal(_bits(x), _bits(o.x)) and np.array_equal(_bits(v), _bits(o.v)), f"state after tick {t}"
        x, v = sb.get_positions(), sb.get_velocities()
        assert np.array_equal(_bits(x), _bits(o.x)) and np.array_equal(_bits(v), _bits(o.v))
        rep = sb.validate()
        assert rep["errors"] == [0] * 6 and rep["constraints_checked"] == len(mesh.dist_rest), rep
        return sb.stats()
    finally:
        sb.OnDestroy()


@pytest.mark.parametrize("n", (16, 24))
@pytest.mark.parametrize("substeps", (5, 6))
def test_substep_parity_the_last_kernel_on_either_tiling(monkeypatch, oracle_mod, n, substeps):
    _narrow(monkeypatch)
    st = _run(oracle_mod, jelly_cube(n), dict(substeps=substeps))
    if substeps % 2 == 0:      # (an odd count ends the tick on T1: its held-back last kernel cannot fuse with a first kernel on T0)
        assert st["ticks_fused"] >= 1      # the tick after the positions-only read started on the fused boundary


def test_ground_plane_three_rest_lengths_and_a_mass_palette_with_pins(monkeypatch, oracle_mod):
    _narrow(monkeypatch)
    n = 16
    mesh = jelly_cube(n)
    m = len(mesh.dist_rest) // 3                  # structural springs: x, then y, then z
    mesh.dist_rest = mesh.dist_rest.copy()
    mesh.dist_rest[m:2 * m] *= np.float32(1.03125)      # three rest lengths: every tile's palette has three entries, read through LDS
    mesh.dist_rest[2 * m:] *= np.float32(0.96875)
    assert len(np.unique(mesh.dist_rest)) == 3
    w = mesh.inv_mass.copy().reshape(n, n, n)
    w[:, :, 1::3] = 0.5; w[:, 2::5, :] = 2.0; w[3::7, :, :] = 0.25      # four masses, in every tile
    w[n - 1, n - 1, :] = 0.0; w[5, 9, 3] = 0.0                            # pinned: an edge of the cube and one particle inside (P.w == 0)
    mesh.inv_mass = w.reshape(-1)
    assert len(np.unique(mesh.inv_mass)) == 5
    # one free particle is thrown as in the escape case below (several units per substep, far beyond 2^20 ulps of any coordinate of this
    # cube), so that the palette kernels' escape paths run too: the decode's dependent load and the store's ballot
    vel = np.zeros_like(mesh.pos)
    assert mesh.inv_mass[0] > 0.0
    vel[0] = -1500.0
    _run(oracle_mod, mesh, dict(substeps=6, ground_plane=(0, 1, 0, -3.0), damping=0.05), state=(mesh.pos.copy(), vel))


def test_escapes_and_codes_side_by_side_at_one_boundary_on_both_tilings(monkeypatch, oracle_mod):
    """One corner particle is thrown hard enough for its code to escape, and it drags a few neighbours along; the cube is moved away
    from the origin, where tiny coordinates would make escapes of their own. The hand-offs are computed on the CPU first. A wave owns at
    most 256 particles, so a tiling runs at least n / 256 waves: with fewer escaped particles than that, some wave holds none."""
    _narrow(monkeypatch)
    n, substeps, ticks = 24, 6, 2
    mesh = jelly_cube(n)
    mesh.pos = mesh.pos + np.float32(8.0); mesh.rest_pos = mesh.rest_pos + np.float32(8.0)
    vel = np.zeros_like(mesh.pos)
    vel[0] = -1500.0      # (5 units per substep; the springs pull most of it back before the hand-off)
    state = (mesh.pos.copy(), vel)
    probe = jelly_cube(n)
    probe.pos, probe.rest_pos, probe.vel = state[0].copy(), mesh.rest_pos.copy(), vel.copy()
    counts = [int(_escapes(p, x).sum()) for x, p in _handoffs(oracle_mod, probe, substeps, ticks)]
    print("escaped particles per launch boundary:", counts)
    mixed = [0 < c < mesh.n // 256 for c in counts]
    tiling_of = [it & 1 for _ in range(ticks) for it in range(substeps)]      # the tiling of the kernel that writes the hand-off
    assert any(m for m, tl in zip(mixed, tiling_of) if tl == 0) and any(m for m, tl in zip(mixed, tiling_of) if tl == 1), counts
    _run(oracle_mod, mesh, dict(substeps=substeps), ticks=ticks, pos_only=(0,), state=state)


def test_kinematic_targets_inside_the_fused_boundary(monkeypatch, oracle_mod):
    _narrow(monkeypatch)
    pins = np.nonzero(jelly_cube(16, pin_top=True).inv_mass == 0.0)[0].astype(np.int32)
    rest = jelly_cube(16, pin_top=True).pos[pins].copy()

    def move(t, sb, o):
        target = rest + np.array([0.3 * np.sin(0.4 * t), 0.1 * t, -0.2 * t], np.float32)
        sb.set_kinematic_positions(pins, target)
        o.set_kinematic_positions(pins, target)
    st = _run(oracle_mod, jelly_cube(16, pin_top=True), dict(substeps=6), ticks=5, pos_only=(0, 1, 2, 3), before_tick=move)
    assert st["ticks_fused_kinematic"] >= 3, st      # the moves travelled inside the fused kernel: the lean mid-kinematic kernel ran


def test_cube40_tile128_rim_packs_and_many_runs(monkeypatch, oracle_mod):
    """Measured on the GPU: this lattice comes out all-packed too (lane_packed_tiles == n_tiles == [148, 324]), so by the rule it runs
    the lean kernels, with rim packs of many runs; the negative proper is the next case."""
    _narrow(monkeypatch)
    _run(oracle_mod, jelly_cube(40), dict(substeps=4, tile_particles=128), lean=True)


def test_negative_one_tile_with_a_long_palette_keeps_the_general_coded_kernels(monkeypatch, oracle_mod):
    """64 springs at one corner get rest lengths of their own: the tiles that hold them need a palette of more than kLanePackMaxPalette
    entries and stay unpacked (4-byte slots through the LDS window), every other tile is lane-packed. The solver is coded but not
    all-packed: it keeps the general coded kernels."""
    _narrow(monkeypatch)
    mesh = jelly_cube(16)
    mesh.dist_rest = mesh.dist_rest.copy()
    mesh.dist_rest[:64] *= (np.float32(1.0) + np.arange(1, 65, dtype=np.float32) / np.float32(1024.0))
    assert len(np.unique(mesh.dist_rest)) == 65
    st = _run(oracle_mod, mesh, dict(substeps=6), lean=False)
    assert any(0 < st["lane_packed_tiles"][tl] < st["n_tiles"][tl] for tl in (0, 1)), (st["lane_packed_tiles"], st["n_tiles"])
