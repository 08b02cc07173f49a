"""Reference for the closest-point queries of SPEC.md 6g, three times: vectorised numpy float32 with one rounded operation per statement, the
plain sequential loop over the triangles in float32 scalars, and the same chain in float64 (an error yardstick, not a bitwise quantity).
dd is a sum of squares, so (bits(dd) << 32) | triangle is a total order and the nearest point is an exact minimum: the GPU must reproduce
all four fields bit for bit, whatever tree it reduces in. Also the region (1 .. 7) that decided each winner, the hostile corpus, and the
constants that mirror the kernels' shape."""
import numpy as np

from raycast_ref import hostile_scene as _ray_hostile_scene
from raycast_ref import random_scene as _ray_random_scene

F32 = np.float32
HIT = np.dtype([("triangle", np.int32), ("distance", np.float32), ("u", np.float32), ("v", np.float32)])
MISS_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)

# = kRayLanes, kRayMaxGroups (the query shares the ray cast's launch shape and buffers), kClosestTile, kClosestBatch of
# csrc/readback_kernels.hip.hpp and csrc/closest_kernels.hip.hpp: lanes of a workgroup, the grid cap along the triangles (longer lists walk
# the grid-stride loop), queries a workgroup tests each triangle against, queries per pair of launches
LANES = 256
GRID_CAP = 1024
QUERY_TILE = 4
QUERY_BATCH = 256
TRIANGLE_COUNTS = (1, 63, 64, 65, 255, 256, 257, 3 * (GRID_CAP * LANES) + 77)
QUERY_COUNTS = (1, QUERY_TILE - 1, QUERY_TILE, QUERY_TILE + 1, QUERY_BATCH + 1)
SEED = 5
REGIONS = ("vertex a", "vertex b", "edge ab", "vertex c", "edge ac", "edge bc", "face")       # region r is REGIONS[r - 1]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_hits(got, want):
    """bitwise on all four fields"""
    got = np.ascontiguousarray(got); want = np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == HIT and want.dtype == HIT and got.tobytes() == want.tobytes()


def make_queries(points, max_distance=np.inf):
    """(Q, 4) float32 = x, y, z, max_distance"""
    points = np.asarray(points, F32).reshape(-1, 3)
    q = np.zeros((points.shape[0], 4), F32)
    q[:, 0:3] = points; q[:, 3] = max_distance
    return q


def _dot(a, b):
    xx = a[0] * b[0]; yy = a[1] * b[1]; zz = a[2] * b[2]
    return (xx + yy) + zz


def _chain(pa, ab, ac, pb, pc, q, one):
    """SPEC.md 6g for one query q (3 scalars) against arrays of triangles (pa, pb, pc, ab, ac: three arrays each), every statement one
    rounded operation of the arrays' type. -> (region, u, v, dd)"""
    ap = [q[k] - pa[k] for k in range(3)]; bp = [q[k] - pb[k] for k in range(3)]; cp = [q[k] - pc[k] for k in range(3)]
    d1 = _dot(ab, ap); d2 = _dot(ac, ap); d3 = _dot(ab, bp); d4 = _dot(ac, bp); d5 = _dot(ab, cp); d6 = _dot(ac, cp)
    t0 = d1 * d4; t1 = d3 * d2; vc = t0 - t1
    t0 = d5 * d2; t1 = d1 * d6; vb = t0 - t1
    t0 = d3 * d6; t1 = d5 * d4; va = t0 - t1
    e = d4 - d3; f = d5 - d6
    tests = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6), (vb <= 0) & (d2 >= 0) & (d6 <= 0),
             (va <= 0) & (e >= 0) & (f >= 0)]
    region = np.full(d1.shape, 7, np.int32)
    for r in range(6, 0, -1):                   # the first test that holds decides
        region[tests[r - 1]] = r
    zero = one * 0
    t0 = d1 - d3; u3 = d1 / t0
    t0 = d2 - d6; v5 = d2 / t0
    t0 = e + f; w = e / t0; u6 = one - w
    t0 = va + vb; t0 = t0 + vc; den = one / t0; u7 = vb * den; v7 = vc * den
    u = np.select([region == 1, region == 2, region == 3, region == 4, region == 5, region == 6], [zero, one, u3, zero, zero, u6], u7)
    v = np.select([region == 1, region == 2, region == 3, region == 4, region == 5, region == 6], [zero, zero, zero, one, v5, w], v7)
    u = u.astype(d1.dtype); v = v.astype(d1.dtype)
    r = []
    for k in range(3):
        t0 = u * ab[k]; t1 = v * ac[k]; t0 = t0 + t1; c = pa[k] + t0
        r.append(q[k] - c)
    return region, u, v, _dot(r, r)


def closest_ref(p, tri, queries, with_regions=False):
    """hits (Q,) of queries (Q, 4) against triangles tri (m, 3) over vertices p (rows, 3): vectorised over the triangles, every statement of
    SPEC.md 6g one float32 numpy operation. with_regions: -> (hits, the region 1 .. 7 that decided each winner, 0 for a miss)"""
    p = np.ascontiguousarray(p, F32).reshape(-1, 3)
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    queries = np.ascontiguousarray(queries, F32).reshape(-1, 4)
    hits = np.zeros(queries.shape[0], HIT)
    hits["triangle"] = -1
    regions = np.zeros(queries.shape[0], np.int32)
    if tri.shape[0]:
        ids = np.arange(tri.shape[0], dtype=np.uint64)
        with np.errstate(all="ignore"):
            pa = [p[tri[:, 0], k] for k in range(3)]; pb = [p[tri[:, 1], k] for k in range(3)]; pc = [p[tri[:, 2], k] for k in range(3)]
            ab = [pb[k] - pa[k] for k in range(3)]; ac = [pc[k] - pa[k] for k in range(3)]
            for j, qr in enumerate(queries):
                R2 = qr[3] * qr[3]
                region, u, v, dd = _chain(pa, ab, ac, pb, pc, qr[0:3], F32(1))
                assert dd.dtype == F32 and u.dtype == F32 and v.dtype == F32
                ok = (dd <= R2) & (dd < np.inf)
                key = np.where(ok, (bits(dd).astype(np.uint64) << np.uint64(32)) | ids, MISS_KEY)
                k = int(np.argmin(key))
                if key[k] != MISS_KEY:
                    hits[j] = (k, np.sqrt(dd[k]), u[k], v[k])
                    regions[j] = region[k]
    return (hits, regions) if with_regions else hits


def closest_loop(p, tri, queries):
    """The statements of SPEC.md 6g, one triangle after the other, in float32 scalars: the chain as the first test that holds."""
    p = np.ascontiguousarray(p, F32).reshape(-1, 3)
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    queries = np.ascontiguousarray(queries, F32).reshape(-1, 4)
    hits = np.zeros(queries.shape[0], HIT)
    z, one = F32(0), F32(1)
    with np.errstate(all="ignore"):
        for j, qr in enumerate(queries):
            q = qr[0:3]
            R2 = qr[3] * qr[3]
            best = (-1, z, z, z)
            for t_id, (a, b, c) in enumerate(tri):
                ab = p[b] - p[a]; ac = p[c] - p[a]; ap = q - p[a]; bp = q - p[b]; cp = q - p[c]
                d1 = _dot(ab, ap); d2 = _dot(ac, ap); d3 = _dot(ab, bp); d4 = _dot(ac, bp); d5 = _dot(ab, cp); d6 = _dot(ac, cp)
                vc = (d1 * d4) - (d3 * d2); vb = (d5 * d2) - (d1 * d6); va = (d3 * d6) - (d5 * d4); e = d4 - d3; f = d5 - d6
                if d1 <= 0 and d2 <= 0:
                    u, v = z, z
                elif d3 >= 0 and d4 <= d3:
                    u, v = one, z
                elif vc <= 0 and d1 >= 0 and d3 <= 0:
                    u, v = d1 / (d1 - d3), z
                elif d6 >= 0 and d5 <= d6:
                    u, v = z, one
                elif vb <= 0 and d2 >= 0 and d6 <= 0:
                    u, v = z, d2 / (d2 - d6)
                elif va <= 0 and e >= 0 and f >= 0:
                    w = e / (e + f)
                    u, v = one - w, w
                else:
                    den = one / ((va + vb) + vc)
                    u, v = vb * den, vc * den
                cc = p[a] + ((u * ab) + (v * ac))
                r = q - cc
                dd = _dot(r, r)
                if not (dd <= R2 and dd < np.inf):
                    continue
                if best[0] < 0 or dd < best[1]:          # (triangles ascending: among equal dd the first one stays)
                    best = (t_id, dd, u, v)
            hits[j] = (best[0], np.sqrt(best[1]), best[2], best[3])
    return hits


def closest_f64(p, tri, queries):
    """The same chain in float64 on the float32 inputs. -> (distance (Q,) float64, +inf for a miss; triangle; region)"""
    p = np.ascontiguousarray(p, F32).reshape(-1, 3).astype(np.float64)
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    queries = np.ascontiguousarray(queries, F32).reshape(-1, 4).astype(np.float64)
    dist = np.full(queries.shape[0], np.inf); who = np.full(queries.shape[0], -1); regions = np.zeros(queries.shape[0], np.int32)
    with np.errstate(all="ignore"):
        pa = [p[tri[:, 0], k] for k in range(3)]; pb = [p[tri[:, 1], k] for k in range(3)]; pc = [p[tri[:, 2], k] for k in range(3)]
        ab = [pb[k] - pa[k] for k in range(3)]; ac = [pc[k] - pa[k] for k in range(3)]
        for j, qr in enumerate(queries):
            region, _, _, dd = _chain(pa, ab, ac, pb, pc, qr[0:3], np.float64(1))
            dd = np.where((dd <= qr[3] * qr[3]) & (dd < np.inf), dd, np.inf)
            k = int(np.argmin(dd))
            if dd[k] < np.inf:
                dist[j], who[j], regions[j] = np.sqrt(dd[k]), k, region[k]
    return dist, who, regions


def candidates(p, tri, query):
    """(triangle id, bits of dd) of every candidate of one query, for tests that count ties"""
    p = np.ascontiguousarray(p, F32).reshape(-1, 3)
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    q = np.asarray(query, F32).reshape(4)
    with np.errstate(all="ignore"):
        pa = [p[tri[:, 0], k] for k in range(3)]; pb = [p[tri[:, 1], k] for k in range(3)]; pc = [p[tri[:, 2], k] for k in range(3)]
        ab = [pb[k] - pa[k] for k in range(3)]; ac = [pc[k] - pa[k] for k in range(3)]
        _, _, _, dd = _chain(pa, ab, ac, pb, pc, q[0:3], F32(1))
        ok = (dd <= q[3] * q[3]) & (dd < np.inf)
    return [(int(t), int(bits(dd[t:t + 1])[0])) for t in np.nonzero(ok)[0]]


def point_of(p, tri, hit):
    """(1 - u - v) p[a] + u p[b] + v p[c] in float64: where the hit lies (for known answers, not a bitwise quantity)"""
    a, b, c = (np.asarray(p, np.float64)[i] for i in tri[hit["triangle"]])
    u, v = float(hit["u"]), float(hit["v"])
    return (1 - u - v) * a + u * b + v * c


def random_scene(n_vertices, n_triangles, n_queries, seed):
    """raycast_ref.random_scene's vertices and triangles; the queries are its ray origins times 0.4f -- points at radius 1.2 around a cloud
    in [-1, 1]^3 --, every third cut short by a finite max_distance, every other one of those by a minute one, so that hits and misses both
    occur at every triangle count"""
    p, tri, rays = _ray_random_scene(n_vertices, n_triangles, n_queries, seed)
    pts = rays[:, 0:3] * F32(0.4)
    rng = np.random.default_rng([seed, n_queries, 11])
    lim = np.where(np.arange(n_queries) % 3 == 1, rng.uniform(0.02, 0.6, size=n_queries), np.inf)
    lim[4::6] *= 2.0 ** -24            # (a list of many triangles is near every query: some limits lie below any distance there)
    return p, tri, make_queries(pts, lim)


def hostile_scene(seed=SEED):
    """-> (p, tri, queries, names): the vertices and triangles of raycast_ref.hostile_scene -- a random cloud around (-10, 0, 0); the unit
    triangle A at z = 5 (x offset 10); a repeated corner, three collinear corners, one point three times; NaN, +inf, -inf and 1e38 corners
    beside sound triangles; edges of 2^-64 and 2^-140; a triangle of size 2^40 -- and the queries of SPEC.md 6g that go wrong first: on a
    vertex, an edge and the face of A (distance +0), in each region around A, with max_distance exactly the distance, one ulp below it and
    zero, beside the tiny and the degenerate triangles, and 1e30 away, where dd overflows."""
    p, tri, _, ray_names = _ray_hostile_scene(seed)
    names = {k: v for k, v in ray_names.items() if k.startswith("tri_")}
    qs = []

    def Q(name, xyz, lim=np.inf):
        qs.append((xyz[0], xyz[1], xyz[2], lim)); names["q_" + name] = len(qs) - 1

    Q("on_vertex_a", (10, 0, 5)); Q("on_vertex_b", (11, 0, 5)); Q("on_vertex_c", (10, 1, 5))
    Q("on_edge_ab", (10.5, 0, 5)); Q("on_edge_ac", (10, 0.5, 5)); Q("on_edge_bc", (10.5, 0.5, 5)); Q("in_face", (10.25, 0.25, 5))
    Q("on_face_limit_zero", (10.25, 0.25, 5), 0.0); Q("off_face_limit_zero", (10.25, 0.25, 5.125), 0.0)
    Q("above_face", (10.25, 0.25, 5.25)); Q("limit_equal", (10.25, 0.25, 5.25), 0.25)
    Q("limit_one_ulp_below", (10.25, 0.25, 5.25), np.nextafter(F32(0.25), F32(0)))
    Q("beyond_a", (9.5, -0.5, 5.125)); Q("beyond_b", (12, -0.25, 5.125)); Q("beyond_c", (9.75, 2, 5.125))
    Q("beyond_ab", (10.5, -0.5, 5.125)); Q("beyond_ac", (9.5, 0.5, 5.125)); Q("beyond_bc", (11, 1, 5.125))
    Q("beside_collinear", (10.25, 0.125, 4.5)); Q("on_collinear", (10.75, 0, 4.5))
    Q("at_the_nan", (10.5, 0.5, 7.5)); Q("near_the_nan", (10.5, 0.5, 7.25), 0.5)
    e = 2.0 ** -64
    Q("on_subnormal_edges", (0.5 * e, 0.25 * e, 0)); Q("over_subnormal_edges", (0.5 * e, 0.25 * e, 2.0 ** -70))
    Q("on_2^-140", (0, 0, -1)); Q("beside_2^-140", (2.0 ** -141, 2.0 ** -141, -1), 2.0 ** -100)
    Q("under_huge", (300, 300, -51)); Q("on_huge", (2.0 ** 30, 2.0 ** 20, -50)); Q("far_from_huge", (0, 0, 1e6))
    Q("1e30_away_x", (1e30, 0, 0)); Q("1e30_away_z", (0, 0, -1e30)); Q("1e30_away_diagonal", (-1e30, 1e30, 1e30))
    Q("1e18_away", (0, 1e18, 0))
    _, _, cloud = random_scene(8, 1, 24, seed)
    cloud[:, 0:3] *= F32(0.5); cloud[:, 0] += F32(-10)
    return p, tri, np.concatenate([np.array(qs, F32), cloud]), names


def lattice_queries(n):
    """Queries two above the top face of the undeformed n^3 lattice (tools/readback_bench.py surface_triangles: every quad cut along the same
    diagonal) over an interior lattice vertex, the middle of an edge and the middle of a quad's diagonal: 6, 2 and 2 triangles are equally
    near there. -> (queries, the candidate counts of equal dd)"""
    c = n // 2
    return make_queries([(c, c, n + 1), (c + 0.5, c, n + 1), (c + 0.5, c + 0.5, n + 1)]), (6, 2, 2)
