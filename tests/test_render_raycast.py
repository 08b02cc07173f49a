"""The ray casts of SPEC.md 6e on the CPU: the two restatements of tests/raycast_ref.py agree bit for bit on the hostile corpus and on random
scenes, known answers, the ties the GPU test relies on, and what the entry points refuse without a GPU. (tests/test_abi.py checks that the
two entry points are declared, exported and bound consistently.)"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from raycast_ref import (GRID_CAP, HIT, LANES, RAY_BATCH, RAY_COUNTS, RAY_TILE, SEED, TRIANGLE_COUNTS, bits, candidates, hostile_scene, lattice_points,
                         lattice_rays, make_rays, point_of, random_scene, raycast_loop, raycast_ref, same_hits)
from softbodyunity_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

UNIT = (np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.int32([[0, 1, 2]]))


def test_the_two_restatements_agree_on_the_hostile_corpus():
    p, tri, rays, names = hostile_scene()
    a, b = raycast_ref(p, tri, rays), raycast_loop(p, tri, rays)
    assert a.dtype == HIT and same_hits(a, b)
    # ... and on a corpus with the triangles in another order (the ids change, nothing else does)
    perm = np.random.default_rng(1).permutation(len(tri))
    c = raycast_ref(p, tri[perm], rays)
    hit = a["triangle"] >= 0
    assert np.array_equal(hit, c["triangle"] >= 0) and np.array_equal(bits(a["t"]), bits(c["t"]))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_two_restatements_agree_on_random_scenes(seed):
    p, tri, rays = random_scene(60, 257, 9, seed)
    a = raycast_ref(p, tri, rays)
    assert same_hits(a, raycast_loop(p, tri, rays))
    assert (a["triangle"] >= 0).any()


def test_known_answers_on_the_unit_triangle():
    p, tri = UNIT
    rays = make_rays([(0.25, 0.25, 1), (0.25, 0.25, -1), (0.25, 0.25, 1), (2, 2, 1), (0.25, 0.25, 1)], [(0, 0, -1), (0, 0, 1), (0, 0, -4), (0, 0, -1), (0, 0, 1)])
    for f in (raycast_ref, raycast_loop):
        h = f(p, tri, rays)
        assert h[0] == np.array((0, 1.0, 0.25, 0.25), HIT), "from the front"
        assert h[1]["triangle"] == 0 and h[1]["t"] == 1 and h[1]["u"] == 0.25 and h[1]["v"] == 0.25, "from behind: both faces are hit"
        assert h[2]["triangle"] == 0 and h[2]["t"] == 0.25, "t is in units of |d|"
        for k in (3, 4):
            assert h[k] == np.array((-1, 0, 0, 0), HIT) and not h[k].tobytes()[4:].strip(b"\0"), "a miss is -1, +0, +0, +0"
        assert np.allclose(point_of(p, tri, h[0]), [0.25, 0.25, 0])
    assert same_hits(raycast_ref(p, np.zeros((0, 3), np.int32), rays), np.array([(-1, 0, 0, 0)] * 5, HIT))


def test_the_hostile_corpus_reaches_every_planted_case():
    p, tri, rays, n = hostile_scene()
    h = raycast_ref(p, tri, rays)
    A = n["tri_A"]
    ray = lambda name: h[n["ray_" + name]]
    assert ray("front")["triangle"] == A and ray("front")["t"] == 1 and ray("behind")["triangle"] == A and ray("behind")["t"] == 1
    assert ray("parallel")["triangle"] != A
    for name in ("in_plane_down", "in_plane_up", "tmax_zero"):
        assert ray(name)["triangle"] == A and bits(ray(name)["t"]) == 0, f"{name}: a zero distance is +0"
    # from one side the raw quotient is -0: the + 0.0f is what makes it +0
    one = rays[n["ray_in_plane_up"]], rays[n["ray_in_plane_down"]]
    raw = []
    for r in one:
        d = r[4:7]; e1 = p[tri[A][1]] - p[tri[A][0]]; e2 = p[tri[A][2]] - p[tri[A][0]]
        T = r[0:3] - p[tri[A][0]]
        Q = np.cross(T, e1).astype(np.float32); det = np.float32(np.dot(e1, np.cross(d, e2)))
        raw.append(np.float32(np.dot(e2, Q)) * (np.float32(1) / det))
    assert sorted(int(bits(x).item()) for x in raw) == [0, 0x80000000]
    assert ray("one_ulp_behind")["triangle"] != A and ray("one_ulp_behind")["triangle"] == n["tri_huge"]
    assert ray("tmax_equal")["triangle"] == A and ray("tmax_one_ulp_below")["triangle"] == -1
    # (with a direction of length 4 the triangle with the 1e38 corner, whose rounding errors are of the size of the scene, comes out nearer)
    assert raycast_ref(p, tri[[A]], rays[n["ray_long_direction"]])[0]["t"] == 0.25 and ray("long_direction")["t"] <= 0.25
    assert ray("subnormal_det")["triangle"] == n["tri_subnormal_det"] and ray("subnormal_det")["t"] == 1
    assert ray("underflowing_det")["triangle"] != n["tri_underflowing_det"]
    assert ray("barely_normal_det")["triangle"] == n["tri_barely_normal_det"]
    assert ray("tie_of_the_tiny_ones")["triangle"] == n["tri_subnormal_det"] and len(candidates(p, tri, rays[n["ray_tie_of_the_tiny_ones"]])) >= 2
    assert ray("huge_only")["triangle"] == n["tri_huge"] and ray("huge_oblique")["triangle"] == n["tri_huge"] and ray("away")["triangle"] == -1
    # zero-area triangles and those with a NaN or infinite corner are never hit, and remove nothing else
    dead = {n["tri_" + k] for k in ("repeated_corner", "collinear", "point", "nan", "nan_last", "pinf", "ninf")}
    assert not dead & set(h["triangle"].tolist())
    keep = np.array([t not in dead for t in range(len(tri))])
    g = raycast_ref(p, tri[keep], rays)
    assert np.array_equal(bits(g["t"]), bits(h["t"])) and np.array_equal(bits(g["u"]), bits(h["u"]))
    assert not np.isnan(h["t"]).any() and not np.isnan(h["u"]).any() and not np.isnan(h["v"]).any()
    assert (h["triangle"][-24:] >= 0).any(), "no random ray meets the cloud"


def test_ties_go_to_the_lower_index_and_the_lattice_has_them():
    from readback_bench import surface_triangles
    n = 12
    p, tri = lattice_points(n), surface_triangles(n)
    rays, counts = lattice_rays(n)
    h = raycast_ref(p, tri, rays)
    for r, want in enumerate(counts):
        cand = candidates(p, tri, rays[r])
        top = [c for c in cand if c[1] == h[r]["t"]]
        assert len(top) == want and h[r]["t"] == 8 + 1, (r, cand)
        assert h[r]["triangle"] == min(c[0] for c in top)
    # the same triangle twice: the lower index wins wherever the two sit
    p1, t1 = UNIT
    one = make_rays([(0.25, 0.25, 1)], (0, 0, -1))
    far = np.int32([[0, 0, 0]] * 700)
    for lo, hi in ((3, 4), (3, 67), (3, 300), (3, 699), (63, 64), (255, 256)):
        t = far.copy(); t[lo] = t1[0]; t[hi] = t1[0]
        assert raycast_ref(p1, t, one)[0]["triangle"] == lo and raycast_loop(p1, t[:hi + 1], one)[0]["triangle"] == lo


def test_the_shapes_mirror_the_kernels_constants():
    src = open(os.path.join(ROOT, "softbodyunity_amd", "csrc", "readback_kernels.hip.hpp")).read()
    for name, value in (("kRayLanes", LANES), ("kRayMaxGroups", GRID_CAP), ("kRayTile", RAY_TILE), ("kRayBatch", RAY_BATCH)):
        assert f"constexpr int {name} = {value};" in src, name
    assert TRIANGLE_COUNTS[-1] == 3 * GRID_CAP * LANES + 77 and RAY_COUNTS == (1, RAY_TILE - 1, RAY_TILE, RAY_TILE + 1, RAY_BATCH + 1)
    assert 2 <= RAY_TILE <= 8 and SEED >= 0


def test_the_abi_refuses_a_null_handle_without_a_gpu():
    L = native.lib()
    assert C.sizeof(native.SbRayHit) == 16 and HIT.itemsize == 16
    rays = make_rays([(0, 0, 1)], (0, 0, -1))
    hits = np.full(1, 7, np.int32).repeat(4).view(HIT)
    before = hits.tobytes()
    for fn, name in ((L.sb_readback_raycast, b"sb_readback_raycast"), (L.sb_group_readback_raycast, b"sb_group_readback_raycast")):
        rc = fn(None, rays.ctypes.data_as(C.POINTER(C.c_float)), 1, hits.ctypes.data_as(C.POINTER(native.SbRayHit)))
        assert rc == native.SB_ERR_INVALID_ARG and name in L.sb_last_error() and hits.tobytes() == before
