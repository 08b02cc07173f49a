"""Content-addressed tile programs (csrc/tables.hip): tiles whose programs are byte-identical -- every interior tile of a lattice, the face,
edge and corner tiles of each kind -- share ONE copy in the uploaded stream. Only the descriptors' s_begin changes, so every mesh, layout
and schedule gives the same bits with sharing on and off (SB_NO_SHARED_PROGRAMS=1), the validator walks every tile as before, and the
compulsory-bytes model (sb_stats.launch_bytes: what the tiles READ) stays what it was; only the device memory of the tables shrinks."""
import numpy as np
import pytest

from softbodyunity_amd import Softbody, bunny_surrogate, jelly_cube

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _share(monkeypatch, on):
    if on:
        monkeypatch.delenv("SB_NO_SHARED_PROGRAMS", raising=False)
    else:
        monkeypatch.setenv("SB_NO_SHARED_PROGRAMS", "1")


def _run_single(monkeypatch, on, mesh, kw, ticks):
    _share(monkeypatch, on)
    sb = Softbody(mesh, **kw).Start()
    try:
        st = sb.stats()
        for _ in range(ticks):
            sb.step()
        x, v = sb.get_positions().copy(), sb.get_velocities().copy()
        rep = sb.validate()
        assert rep["errors"] == [0] * 6 and rep["first_stage"] == -1, rep
        assert rep["constraints_checked"] == len(mesh.dist_rest) + len(mesh.vol_rest) + len(mesh.bend_rest), rep
        return x, v, st, rep
    finally:
        sb.OnDestroy()


def _table_stream_bytes(st, tl):
    """Bytes of tiling tl's programs as the tiles read them: launch_bytes minus the particle state and the descriptors (uniform-mass
    springs-only lattices: 48 B per staged particle, no run overflow)."""
    return st["launch_bytes"][tl] - 48 * st["n_particles_local"] - 128 * st["n_tiles"][tl]


CASES = {
    # 512-lane launches (64^3: 512 / 729 tiles), programs in the 4-byte form
    "cube64": lambda: (jelly_cube(64), dict(substeps=6, ground_plane=(0, 1, 0, -2.0), damping=0.05), True),
    # 256-lane launches with the 8-byte wide-packed programs (80^3: 1 000 T0 tiles)
    "wide_cube80": lambda: (jelly_cube(80), dict(substeps=4), True),
    # per-particle masses and per-spring rest lengths: no two tiles have the same program, the same bits all the same
    "cube40_heterogeneous": lambda: (jelly_cube(40, heterogeneous=True), dict(substeps=4, ground_plane=(0, 1, 0, -2.0)), False),
    # tets and hinges: wave items and four-vertex slots in the programs
    "bunny5k_tets_hinges": lambda: (bunny_surrogate(target_verts=5000, seed=11),
                                    dict(substeps=6, distance_compliance=1e-7, volume_compliance=1e-7, bending_compliance=1e-4), False),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_shared_programs_give_the_same_bits(case, monkeypatch):
    mesh, kw, lattice = CASES[case]()
    monkeypatch.delenv("SB_NARROW_MIN_TILES", raising=False)
    xa, va, sa, ra = _run_single(monkeypatch, True, mesh, kw, 3)
    xb, vb, sb_, rb = _run_single(monkeypatch, False, mesh, kw, 3)
    assert np.array_equal(_bits(xa), _bits(xb)) and np.array_equal(_bits(va), _bits(vb))
    assert ra == rb                                                        # the validator walks every tile either way
    assert sa["launch_bytes"] == sb_["launch_bytes"]                       # the bytes model counts what the tiles read
    assert sa["lane_packed_tiles"] == sb_["lane_packed_tiles"] and sa["n_tiles"] == sb_["n_tiles"]
    assert sa["device_bytes"] <= sb_["device_bytes"]
    if lattice:      # most of the lattice's programs are shared: the uploaded tables shrink by most of their program bytes
        programs = _table_stream_bytes(sb_, 0) + _table_stream_bytes(sb_, 1)
        assert sb_["device_bytes"] - sa["device_bytes"] > 0.8 * programs, (sa["device_bytes"], sb_["device_bytes"], programs)
    if case == "wide_cube80":
        assert sa["lane_packed_tiles"][0] == sa["n_tiles"][0] == 1000


def test_shared_programs_narrow_lane_packed(monkeypatch):
    # the headline's form (16-byte lane-packed words, 128-lane launches), forced onto a small lattice
    monkeypatch.setenv("SB_NARROW_MIN_TILES", "1")
    mesh = jelly_cube(48)
    xa, va, sa, _ = _run_single(monkeypatch, True, mesh, dict(substeps=6), 3)
    xb, vb, sb_, _ = _run_single(monkeypatch, False, mesh, dict(substeps=6), 3)
    assert sa["lane_packed_tiles"][0] > 0
    assert np.array_equal(_bits(xa), _bits(xb)) and np.array_equal(_bits(va), _bits(vb))
    assert sa["launch_bytes"] == sb_["launch_bytes"] and sa["device_bytes"] < sb_["device_bytes"]


@pytest.mark.parametrize("world", [2, 4])
def test_shared_programs_on_hosted_ranks(world, monkeypatch):
    # the ranks of a partitioned lattice: boundary / interior pieces of the T0 and T1 launches, ghost runs, fused unpack
    from hosted import HostedRanks
    monkeypatch.delenv("SB_NARROW_MIN_TILES", raising=False)
    mesh = jelly_cube(96)

    def run(on):
        _share(monkeypatch, on)
        with HostedRanks(mesh, world, 4) as H:
            st = [sb.stats() for sb in H.ranks]
            for _ in range(2):
                H.tick()
            x, v, ghosts = H.merged_state()
            for sb in H.ranks:
                rep = sb.validate()
                assert rep["errors"] == [0] * 6, rep
            return x, v, st
    xa, va, sa = run(True)
    xb, vb, sb_ = run(False)
    assert np.array_equal(_bits(xa), _bits(xb)) and np.array_equal(_bits(va), _bits(vb))
    for a, b in zip(sa, sb_):
        assert a["launch_bytes"] == b["launch_bytes"] and a["device_bytes"] < b["device_bytes"]


def test_shared_programs_with_peek_and_kinematic_targets(monkeypatch):
    # position reads between ticks peek (kKindPeek launches over the tiles' programs), pinned particles move (kKindMidKinematic fused first kernel)
    monkeypatch.setenv("SB_PEEK_MIN_TILES", "0")
    n = 24
    mesh = jelly_cube(n)
    pins = np.nonzero(mesh.pos[:, 1] > mesh.pos[:, 1].max() - 0.5)[0].astype(np.int32)
    mesh.inv_mass[pins] = 0.0
    rest = mesh.pos[pins].copy()

    def run(on):
        _share(monkeypatch, on)
        sb = Softbody(mesh, substeps=8, damping=0.05).Start()
        try:
            reads = []
            for t in range(8):
                target = rest + np.array([0.3 * np.sin(0.4 * t), 0.1 * np.cos(0.7 * t) - 0.1, 0.05 * t], np.float32)
                sb.set_kinematic_positions(pins, target)
                if t & 1:
                    reads.append(sb.get_positions().copy())
                sb.step()
            st = sb.stats()
            assert st["readback_peeks"] > 0 and st["ticks_fused_kinematic"] > 0, st
            rep = sb.validate()
            assert rep["errors"] == [0] * 6, rep
            return reads, sb.get_positions().copy(), sb.get_velocities().copy()
        finally:
            sb.OnDestroy()
    ra, xa, va = run(True)
    rb, xb, vb = run(False)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(ra, rb))
    assert np.array_equal(_bits(xa), _bits(xb)) and np.array_equal(_bits(va), _bits(vb))
