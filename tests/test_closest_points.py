"""The closest-point queries of SPEC.md 6g on the CPU: the two float32 restatements of tests/closest_ref.py agree bit for bit on random scenes
and on the hostile corpus, known answers in every region on small-integer coordinates, the ties the GPU test relies on, the limit, the
float64 restatement as an error yardstick, and what the entry point refuses without a GPU. (tests/test_abi.py checks that the entry point
is declared, exported and bound consistently.)"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from closest_ref import (GRID_CAP, HIT, LANES, QUERY_BATCH, QUERY_COUNTS, QUERY_TILE, REGIONS, SEED, TRIANGLE_COUNTS, bits, candidates, closest_f64,
                         closest_loop, closest_ref, hostile_scene, lattice_queries, make_queries, point_of, random_scene, same_hits)
from raycast_ref import lattice_points
from raycast_ref import random_scene as ray_random_scene
from softbodyunity_amd import CLOSEST_HIT, impulse_hits, make_closest_queries, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# one triangle on small integers: every product and sum below is exact
TRI = (np.float32([[0, 0, 0], [4, 0, 0], [0, 4, 0]]), np.int32([[0, 1, 2]]))
# query, region, u, v, distance
KNOWN = [((-3, -4, 0), 1, 0.0, 0.0, 5.0), ((7, -4, 0), 2, 1.0, 0.0, 5.0), ((1, -2, 0), 3, 0.25, 0.0, 2.0), ((-4, 7, 0), 4, 0.0, 1.0, 5.0),
         ((-2, 1, 0), 5, 0.0, 0.25, 2.0), ((4, 4, 1), 6, 0.5, 0.5, 3.0), ((1, 1, 3), 7, 0.25, 0.25, 3.0)]
MISS = np.array((-1, 0, 0, 0), HIT)


def test_the_two_float32_forms_agree_on_the_hostile_corpus():
    p, tri, q, names = hostile_scene()
    a, b = closest_ref(p, tri, q), closest_loop(p, tri, q)
    assert a.dtype == HIT and same_hits(a, b)
    # ... and on a corpus with the triangles in another order (the ids change, nothing else does)
    perm = np.random.default_rng(1).permutation(len(tri))
    c = closest_ref(p, tri[perm], q)
    assert np.array_equal(a["triangle"] >= 0, c["triangle"] >= 0) and np.array_equal(bits(a["distance"]), bits(c["distance"]))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_two_float32_forms_agree_on_random_scenes(seed):
    p, tri, q = random_scene(60, 257, 9, seed)
    a = closest_ref(p, tri, q)
    assert same_hits(a, closest_loop(p, tri, q))
    assert (a["triangle"] >= 0).any()


def test_known_answers_in_each_of_the_seven_regions():
    p, tri = TRI
    q = make_queries([k[0] for k in KNOWN])
    for f in (closest_ref, closest_loop):
        h = f(p, tri, q)
        for j, (xyz, _, u, v, dist) in enumerate(KNOWN):
            assert h[j] == np.array((0, dist, u, v), HIT), (f.__name__, xyz, h[j])
    h, regions = closest_ref(p, tri, q, with_regions=True)
    assert regions.tolist() == [k[1] for k in KNOWN] == [1, 2, 3, 4, 5, 6, 7] and len(REGIONS) == 7
    assert np.allclose(point_of(p, tri, h[5]), [2, 2, 0]) and np.allclose(point_of(p, tri, h[6]), [1, 1, 0])
    assert same_hits(closest_ref(p, np.zeros((0, 3), np.int32), q), np.array([MISS] * 7))


def test_a_query_on_a_vertex_an_edge_and_the_face_is_at_distance_plus_zero():
    p, tri = TRI
    q = make_queries([(4, 0, 0), (2, 0, 0), (1, 1, 0)])
    for f in (closest_ref, closest_loop):
        h = f(p, tri, q)
        assert (h["triangle"] == 0).all() and (bits(h["distance"]) == 0).all(), h
        assert (h["u"].tolist(), h["v"].tolist()) == ([1.0, 0.5, 0.25], [0.0, 0.0, 0.25])


def test_the_limit_is_compared_squared_and_zero_hits_only_on_the_surface():
    p, tri = TRI
    below = np.nextafter(np.float32(3), np.float32(0))
    q = make_queries([(1, 1, 3)] * 4 + [(1, 1, 0), (1, 1, 2.0 ** -60)], [3.0, below, np.inf, 0.0, 0.0, 0.0])
    for f in (closest_ref, closest_loop):
        h = f(p, tri, q)
        assert h[0] == np.array((0, 3.0, 0.25, 0.25), HIT), "max_distance exactly the distance hits"
        assert h[1] == MISS and not h[1].tobytes()[4:].strip(b"\0"), "one ulp below it misses: -1, +0, +0, +0"
        assert h[2] == h[0] and h[3] == MISS, "+inf is allowed; 0 misses off the surface"
        assert h[4]["triangle"] == 0 and bits(h[4]["distance"]) == 0, "0 hits on the surface"
        # dd = 2^-120 > 0 = R2: a miss, although the distance 2^-60 is far below any limit one would call positive
        assert h[5] == MISS
    # dd against R2, not distance against max_distance: 2^-90 above the face dd underflows to +0, which a limit of 0 admits
    h = closest_ref(p, tri, make_queries([(1, 1, 2.0 ** -90)], 0.0))
    assert h[0]["triangle"] == 0 and bits(h[0]["distance"]) == 0


def test_ties_go_to_the_lowest_index_and_the_lattice_has_them():
    from readback_bench import surface_triangles
    n = 12
    p, tri = lattice_points(n), surface_triangles(n)
    q, counts = lattice_queries(n)
    h = closest_ref(p, tri, q)
    assert same_hits(h, closest_loop(p, tri, q))
    for j, want in enumerate(counts):
        cand = candidates(p, tri, q[j])
        least = min(b for _, b in cand)
        top = [t for t, b in cand if b == least]
        assert len(top) == want and h[j]["distance"] == 2 and h[j]["triangle"] == min(top), (j, top, h[j])
    # the same triangle twice: the lower index wins wherever the two sit
    p1, t1 = TRI
    one = make_queries([(1, 1, 3)])
    far = np.int32([[0, 0, 0]] * 700)                 # (the point p[0] three times: a candidate at its corner, sqrt(11) away -- farther than the planted triangle)
    for lo, hi in ((3, 4), (3, 67), (3, 300), (3, 699), (63, 64), (255, 256)):
        t = far.copy(); t[lo] = t1[0]; t[hi] = t1[0]
        assert closest_ref(p1, t, one)[0]["triangle"] == lo and closest_loop(p1, t[:hi + 1], one)[0]["triangle"] == lo


def test_the_hostile_corpus_reaches_every_planted_case():
    p, tri, q, n = hostile_scene()
    h, regions = closest_ref(p, tri, q, with_regions=True)
    A = n["tri_A"]
    at = lambda name: h[n["q_" + name]]       # noqa: E731
    for k, name in enumerate(("on_vertex_a", "on_vertex_b", "on_edge_ab", "on_vertex_c", "on_edge_ac", "on_edge_bc", "in_face")):
        assert at(name)["triangle"] == A and bits(at(name)["distance"]) == 0, f"{name}: a zero distance is +0"
    for k, name in enumerate(("beyond_a", "beyond_b", "beyond_ab", "beyond_c", "beyond_ac", "beyond_bc", "above_face")):
        assert at(name)["triangle"] == A and regions[n["q_" + name]] == k + 1 and at(name)["distance"] > 0, name
    assert at("on_face_limit_zero")["triangle"] == A and at("off_face_limit_zero")["triangle"] == -1
    assert at("limit_equal")["triangle"] == A and at("limit_equal")["distance"] == 0.25 and at("limit_one_ulp_below")["triangle"] == -1
    # NaN and infinite corners fail every test; a repeated corner and one point three times answer with a corner or divide 0 by 0, and are
    # nearest to no query here
    dead = {n["tri_" + k] for k in ("repeated_corner", "point", "nan", "nan_last", "pinf", "ninf")}
    assert not dead & set(h["triangle"].tolist())
    keep = np.array([t not in dead for t in range(len(tri))])
    g = closest_ref(p, tri[keep], q)
    assert np.array_equal(bits(g["distance"]), bits(h["distance"])) and np.array_equal(bits(g["u"]), bits(h["u"])) and np.array_equal(bits(g["v"]), bits(h["v"]))
    assert not np.isnan(h["distance"]).any() and not np.isnan(h["u"]).any() and not np.isnan(h["v"]).any()
    # these collinear corners have a sound edge region; the sound neighbour of the NaN triangles answers beside them
    assert at("on_collinear")["triangle"] == n["tri_collinear"] and bits(at("on_collinear")["distance"]) == 0
    assert at("at_the_nan")["triangle"] == n["tri_1e38"] and at("near_the_nan")["distance"] == 0.25
    # denormals are kept: edges of 2^-64 resolve a third of an edge, edges of 2^-140 answer with their corner
    assert at("on_subnormal_edges")["triangle"] == n["tri_subnormal_det"] and at("on_subnormal_edges")["u"] == np.float32(1 / 3)
    assert at("on_2^-140")["triangle"] == n["tri_underflowing_det"] and bits(at("on_2^-140")["distance"]) == 0
    # 1e30 away dd overflows: no candidate at all, whatever the limit; 1e18 away it does not
    for name in ("1e30_away_x", "1e30_away_z", "1e30_away_diagonal"):
        assert at(name) == MISS, name
    assert at("1e18_away")["triangle"] >= 0 and np.isfinite(at("1e18_away")["distance"])
    # (the triangle of size 2^40 overflows the products of the chain for every query here: it is never a candidate, a known limitation)
    assert n["tri_huge"] not in set(h["triangle"][:n["q_1e18_away"]].tolist())
    assert (h["triangle"][-24:][np.isinf(q[-24:, 3])] >= 0).all() and (h["triangle"][-24:] < 0).any(), "the cloud answers every unlimited random query"


def test_float32_against_the_float64_restatement_and_every_region_decides_a_winner():
    # The scene and the queries of the issue: raycast_ref.random_scene(1000, 257, 64, SEED), its ray origins times 0.4f.
    # Measured here: the float32 winner's distance differs from the float64 minimum by at most 8.597752e-08 (absolute; seeds 0 .. 5 of the
    # same generator: 6.5e-08 .. 1.43e-07). The bound asserted is 8 x the measured maximum: the error scales with the scene's extent, and
    # other seeds of the same generator must pass.
    measured = 8.597752224059896e-08
    bound = 8 * measured
    p, tri, rays = ray_random_scene(1000, 257, 64, SEED)
    q = make_queries(rays[:, 0:3] * np.float32(0.4))
    h, regions = closest_ref(p, tri, q, with_regions=True)
    d64, _, _ = closest_f64(p, tri, q)
    worst = float(np.abs(h["distance"].astype(np.float64) - d64).max())
    counts = np.bincount(regions, minlength=8)
    print(f"float32 against float64: worst absolute deviation {worst:.6e} (bound {bound:.6e}); winners per region 1 .. 7: {counts[1:].tolist()}")
    assert (h["triangle"] >= 0).all() and np.isfinite(d64).all(), "no winner is a miss at max_distance = +inf"
    assert worst <= bound
    assert counts[0] == 0 and (counts[1:] >= 1).all(), counts
    for seed in (0, 1, 2):
        p, tri, rays = ray_random_scene(1000, 257, 64, seed)
        q = make_queries(rays[:, 0:3] * np.float32(0.4))
        dev = float(np.abs(closest_ref(p, tri, q)["distance"].astype(np.float64) - closest_f64(p, tri, q)[0]).max())
        print(f"seed {seed}: {dev:.6e}")
        assert dev <= bound, seed


def test_the_shapes_mirror_the_kernels_constants():
    csrc = os.path.join(ROOT, "softbodyunity_amd", "csrc")
    src = open(os.path.join(csrc, "readback_kernels.hip.hpp")).read() + open(os.path.join(csrc, "closest_kernels.hip.hpp")).read()
    for name, value in (("kRayLanes", LANES), ("kRayMaxGroups", GRID_CAP), ("kClosestTile", QUERY_TILE), ("kClosestBatch", QUERY_BATCH)):
        assert f"constexpr int {name} = {value};" in src, name
    assert TRIANGLE_COUNTS[-1] == 3 * GRID_CAP * LANES + 77 and QUERY_COUNTS == (1, QUERY_TILE - 1, QUERY_TILE, QUERY_TILE + 1, QUERY_BATCH + 1)
    assert 2 <= QUERY_TILE <= 8 and SEED >= 0


def test_the_python_builders_and_impulse_hits_take_what_a_query_returns():
    assert CLOSEST_HIT == HIT and C.sizeof(native.SbClosestHit) == 16 and HIT.itemsize == 16
    q = make_closest_queries([(1, 2, 3), (4, 5, 6)], [0.5, np.inf])
    assert q.dtype == np.float32 and np.array_equal(q, make_queries([(1, 2, 3), (4, 5, 6)], [0.5, np.inf]))
    assert np.array_equal(make_closest_queries((1, 2, 3)), np.float32([[1, 2, 3, np.inf]]))
    p, tri = TRI
    h = closest_ref(p, tri, make_queries([(1, 1, 3), (1, 1, 3)], [np.inf, 1.0]))
    items = impulse_hits(h, (0, 0, -1))
    assert items["kind"].tolist() == [native.SB_IMPULSE_SURFACE] * 2 and items["index"].tolist() == [0, -1]
    assert items["u"].tolist() == [0.25, 0.0] and items["v"].tolist() == [0.25, 0.0]


def test_the_abi_refuses_a_null_group_without_a_gpu():
    L = native.lib()
    q = make_queries([(0, 0, 1)])
    hits = np.full(1, 7, np.int32).repeat(4).view(HIT)
    before = hits.tobytes()
    rc = L.sb_group_readback_closest_points(None, q.ctypes.data_as(C.POINTER(C.c_float)), 1, hits.ctypes.data_as(C.POINTER(native.SbClosestHit)))
    assert rc == native.SB_ERR_INVALID_ARG and b"sb_group_readback_closest_points" in L.sb_last_error() and hits.tobytes() == before
    # (the other refusals -- a negative count, null arrays, NaN and infinite coordinates, a NaN or negative max_distance -- are checked
    # behind the null-group test, so they need a live group: tests/test_gpu_closest_points.py)
