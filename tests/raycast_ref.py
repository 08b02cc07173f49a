"""Reference for the ray casts of SPEC.md 6e, twice: vectorised numpy float32 with one rounded operation per statement, and the plain
sequential loop over the triangles. A candidate's t is a non-negative float after its + 0.0f, so (bits(t) << 32) | triangle is a total order
and the nearest hit is an exact minimum: the GPU must reproduce all four fields bit for bit, whatever tree it reduces in. Also the hostile
corpus, and the constants that mirror the kernels' shape."""
import numpy as np

F32 = np.float32
HIT = np.dtype([("triangle", np.int32), ("t", np.float32), ("u", np.float32), ("v", np.float32)])
MISS_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)

# = kRayLanes, kRayMaxGroups, kRayTile, kRayBatch of csrc/readback_kernels.hip.hpp: lanes of a workgroup, the grid cap along the triangles
# (longer lists walk the grid-stride loop), rays a workgroup tests each triangle against, rays per pair of launches
LANES = 256
GRID_CAP = 1024
RAY_TILE = 4
RAY_BATCH = 256
# the shapes the GPU test runs: around a wave and a workgroup, and three walks of the capped grid with a ragged tail
TRIANGLE_COUNTS = (1, 63, 64, 65, 255, 256, 257, 3 * (GRID_CAP * LANES) + 77)
RAY_COUNTS = (1, RAY_TILE - 1, RAY_TILE, RAY_TILE + 1, RAY_BATCH + 1)
SEED = 5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_hits(got, want):
    """bitwise on all four fields"""
    got = np.ascontiguousarray(got); want = np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == HIT and want.dtype == HIT and got.tobytes() == want.tobytes()


def make_rays(origin, direction, tmax=np.inf):
    """(R, 8) float32 = origin xyz, t_max, direction xyz, 0"""
    origin = np.asarray(origin, F32).reshape(-1, 3)
    direction = np.broadcast_to(np.asarray(direction, F32).reshape(-1, 3), origin.shape)
    rays = np.zeros((origin.shape[0], 8), F32)
    rays[:, 0:3] = origin; rays[:, 3] = tmax; rays[:, 4:7] = direction
    return rays


def _cross(a, b):
    t0 = a[1] * b[2]; t1 = a[2] * b[1]; t2 = a[2] * b[0]; t3 = a[0] * b[2]; t4 = a[0] * b[1]; t5 = a[1] * b[0]
    return (t0 - t1, t2 - t3, t4 - t5)


def _dot(a, b):
    xx = a[0] * b[0]; yy = a[1] * b[1]; zz = a[2] * b[2]
    return (xx + yy) + zz


def raycast_ref(p, tri, rays):
    """hits (R,) of rays (R, 8) against triangles tri (m, 3) over vertices p (rows, 3): vectorised over the triangles, every statement of
    SPEC.md 6e one float32 numpy operation."""
    p = np.ascontiguousarray(p, F32).reshape(-1, 3)
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    rays = np.ascontiguousarray(rays, F32).reshape(-1, 8)
    hits = np.zeros(rays.shape[0], HIT)
    hits["triangle"] = -1
    if tri.shape[0] == 0:
        return hits
    ids = np.arange(tri.shape[0], dtype=np.uint64)
    with np.errstate(all="ignore"):
        pa = [p[tri[:, 0], c] for c in range(3)]
        e1 = [p[tri[:, 1], c] - pa[c] for c in range(3)]
        e2 = [p[tri[:, 2], c] - pa[c] for c in range(3)]
        for r, ray in enumerate(rays):
            o, tmax, d = ray[0:3], ray[3], ray[4:7]
            P = _cross(d, e2)
            det = _dot(e1, P)
            ok = det != 0
            inv = F32(1) / det
            T = [o[c] - pa[c] for c in range(3)]
            u = _dot(T, P) * inv
            ok &= (u >= 0) & (u <= 1)
            Q = _cross(T, e1)
            v = _dot(d, Q) * inv
            ok &= (v >= 0) & ((u + v) <= 1)
            t = _dot(e2, Q) * inv
            ok &= (t >= 0) & (t <= tmax)
            t = t + F32(0)
            assert t.dtype == F32 and u.dtype == F32 and v.dtype == F32
            key = np.where(ok, (bits(t).astype(np.uint64) << np.uint64(32)) | ids, MISS_KEY)
            k = int(np.argmin(key))
            if key[k] != MISS_KEY:
                hits[r] = (k, t[k], u[k], v[k])
    return hits


def raycast_loop(p, tri, rays):
    """The statements of SPEC.md 6e, one triangle after the other, in float32 scalars."""
    p = np.ascontiguousarray(p, F32).reshape(-1, 3)
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    rays = np.ascontiguousarray(rays, F32).reshape(-1, 8)
    hits = np.zeros(rays.shape[0], HIT)
    z = F32(0)
    with np.errstate(all="ignore"):
        for r, ray in enumerate(rays):
            o, tmax, d = ray[0:3], ray[3], ray[4:7]
            best = (-1, z, z, z)
            for t_id, (a, b, c) in enumerate(tri):
                e1 = p[b] - p[a]; e2 = p[c] - p[a]
                P = _cross(d, e2)
                det = _dot(e1, P)
                if not (det != 0):
                    continue
                inv = F32(1) / det
                T = o - p[a]
                u = _dot(T, P) * inv
                if not (u >= 0 and u <= 1):
                    continue
                Q = _cross(T, e1)
                v = _dot(d, Q) * inv
                if not (v >= 0 and (u + v) <= 1):
                    continue
                t = _dot(e2, Q) * inv
                if not (t >= 0 and t <= tmax):
                    continue
                t = t + z
                if best[0] < 0 or t < best[1]:           # (triangles ascending: among equal t the first one stays)
                    best = (t_id, t, u, v)
            hits[r] = best
    return hits


def candidates(p, tri, ray):
    """(triangle ids, t) of every candidate of one ray, for tests that count ties"""
    one = np.asarray(ray, F32).reshape(1, 8)
    out = []
    for t_id in range(len(tri)):
        h = raycast_ref(p, tri[t_id:t_id + 1], one)[0]
        if h["triangle"] == 0:
            out.append((t_id, h["t"]))
    return out


def point_of(p, tri, hit):
    """(1 - u - v) p[a] + u p[b] + v p[c] in float64: where the hit lies (for known answers, not a bitwise quantity)"""
    a, b, c = (np.asarray(p, np.float64)[i] for i in tri[hit["triangle"]])
    u, v = float(hit["u"]), float(hit["v"])
    return (1 - u - v) * a + u * b + v * c


def random_scene(n_vertices, n_triangles, n_rays, seed):
    """random triangles over vertices in [-1, 1]^3 (thin ones, so that a ray meets a few of them, not all), rays from a sphere of radius 3
    aimed into the cloud, a third of them cut short by a finite t_max"""
    rng = np.random.default_rng([seed, n_vertices, n_triangles, n_rays])
    p = rng.uniform(-1.0, 1.0, size=(n_vertices, 3)).astype(F32)
    tri = rng.integers(0, n_vertices, size=(n_triangles, 3)).astype(np.int32)
    o = rng.normal(size=(n_rays, 3)); o = 3.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
    target = rng.uniform(-0.7, 0.7, size=(n_rays, 3))
    d = (target - o) * rng.uniform(0.25, 4.0, size=(n_rays, 1))           # not unit length
    tmax = np.where(rng.uniform(size=n_rays) < 0.33, rng.uniform(0.1, 1.5, size=n_rays), np.inf)
    return p, tri, make_rays(o, d, tmax)


SUB = F32(2.0 ** -140)


def hostile_scene(seed=SEED):
    """-> (p, tri, rays, names): a cloud of random triangles around (-10, 0, 0) and, away from it, the cases of SPEC.md 6e that go wrong first:
      the unit triangle A at z = 5 (x offset 10) with rays from the front, from behind, parallel to it, with the origin in its plane
      (t = +0 from either side), starting one ulp behind it, with t_max exactly t and one ulp below, with a direction of length 4;
      zero-area triangles (a repeated corner, three collinear corners, one point three times); triangles with a NaN, a +inf, a -inf and
      a 1e38 corner beside sound ones; triangles whose determinant is subnormal (edges of 2^-64), underflows to zero (edges of 2^-140) or is
      barely normal (2^-63); one of size 2^40 below everything.
    names: ray and triangle indices by name."""
    rng = np.random.default_rng([seed, 77])
    cloud = (rng.uniform(-1.0, 1.0, size=(200, 3)) + [-10, 0, 0]).astype(F32)
    verts = [tuple(v) for v in cloud]
    tris = [tuple(t) for t in rng.integers(0, 200, size=(300, 3))]
    names = {}

    def V(*xyz):
        verts.append(tuple(F32(c) for c in xyz)); return len(verts) - 1

    def T(name, a, b, c):
        tris.append((a, b, c)); names["tri_" + name] = len(tris) - 1

    a0, a1, a2 = V(10, 0, 5), V(11, 0, 5), V(10, 1, 5)
    T("A", a0, a1, a2)
    T("repeated_corner", a0, a0, a1)
    c0, c1, c2 = V(10, 0, 4.5), V(10.5, 0, 4.5), V(11, 0, 4.5)
    T("collinear", c0, c1, c2)
    T("point", a2, a2, a2)
    nan, pinf, ninf, big = V(np.nan, 0.5, 7.5), V(np.inf, 0, 7.5), V(10, -np.inf, 7.5), V(1e38, -1e38, 7.5)
    g0, g1 = V(10, 0, 7.5), V(11, 1, 7.5)
    T("nan", nan, g0, g1); T("nan_last", g0, g1, nan)
    T("pinf", g0, pinf, g1); T("ninf", g0, g1, ninf); T("1e38", g0, big, g1)
    e = 2.0 ** -64
    s0, s1, s2 = V(0, 0, 0), V(1.5 * e, 0, 0), V(0, e, 0)
    T("subnormal_det", s0, s1, s2)
    u0, u1, u2 = V(0, 0, -1), V(SUB, 0, -1), V(0, SUB, -1)
    T("underflowing_det", u0, u1, u2)
    n1, n2 = V(2.0 ** -63, 0, 0), V(0, 2.0 ** -63, 0)
    T("barely_normal_det", s0, n1, n2)
    h = 2.0 ** 40
    T("huge", V(-h, -h, -50), V(h, -h, -50), V(0, h, -50))

    rays = []

    def R(name, o, d, tmax=np.inf):
        rays.append((o[0], o[1], o[2], tmax, d[0], d[1], d[2], 0.0)); names["ray_" + name] = len(rays) - 1

    down, up = (0, 0, -1), (0, 0, 1)
    R("front", (10.25, 0.25, 6), down)
    R("behind", (10.25, 0.25, 4), up)
    R("parallel", (9.5, 0.25, 5), (1, 0, 0))
    R("in_plane_down", (10.25, 0.5, 5), down)
    R("in_plane_up", (10.25, 0.5, 5), up)
    R("one_ulp_behind", (10.25, 0.25, np.nextafter(F32(5), F32(0))), down)
    R("tmax_equal", (10.25, 0.25, 6), down, 1.0)
    R("tmax_one_ulp_below", (10.25, 0.25, 6), down, np.nextafter(F32(1), F32(0)))
    R("long_direction", (10.25, 0.25, 6), (0, 0, -4))
    R("tmax_zero", (10.25, 0.5, 5), down, 0.0)
    R("through_corner", (10, 0, 6), down)
    R("along_edge_line", (10.5, 0, 6), down)
    R("subnormal_det", (0.5 * e, 0.25 * e, 1), down)
    R("underflowing_det", (0.25 * float(SUB), 0.25 * float(SUB), 1), down)
    R("barely_normal_det", (1.625 * e, 0.25 * e, 1), down)
    R("tie_of_the_tiny_ones", (2.0 ** -65, 2.0 ** -65, 1), down)
    R("at_the_nan", (10.5, 0.5, 8), down)
    R("huge_only", (300, 300, 10), down)
    R("huge_oblique", (0, 0, 1e6), (0.5, 0.25, -1))
    R("away", (10.25, 0.25, 8), up)
    p = np.array(verts, F32)
    tri = np.array(tris, np.int32)
    _, _, cloud_rays = random_scene(8, 1, 24, seed)
    cloud_rays[:, 0:3] += F32([-10, 0, 0])
    return p, tri, np.concatenate([np.array(rays, F32), cloud_rays]), names


def lattice_rays(n):
    """Rays down -z onto the top face of the undeformed n^3 lattice (tools/readback_bench.py surface_triangles: every quad cut along the
    same diagonal) through an interior lattice vertex, the middle of an edge and the middle of a quad's diagonal: 6, 2 and 2 triangles meet
    there, all at the same t. -> (rays, the candidate counts)"""
    c = n // 2
    return make_rays([(c, c, n + 8), (c + 0.5, c, n + 8), (c + 0.5, c + 0.5, n + 8)], (0, 0, -1)), (6, 2, 2)


def lattice_points(n):
    ax = np.arange(n, dtype=F32)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(F32)
