"""The inputs of tests/test_gpu_distance_field.py (SPEC.md 2i), built without a GPU so that tests/test_distance_field.py can check on the CPU
that they reach every branch of tests/distance_field_ref.py: the tables (grids, cells from 2^-40 to 2^30, samples of +-3e38 and subnormal
ones), the poses (identity and turned frames, at rest and moving), the hostile state of tests/test_gpu_colliders.py with particles planted
on the places a random cloud has measure zero at, and the prop of the ticking bodies."""
import numpy as np

import distance_field_ref
import placement_ref
from test_gpu_colliders import SIZES, hostile_state       # noqa: F401  (the particle counts and the state are that module's, as they are)

F = np.float32
GRIDS = {"2x2x2": (2, 2, 2), "2x3x2": (2, 3, 2), "3x2x4": (3, 2, 4), "9x5x17": (9, 5, 17), "1024x2x2": (1024, 2, 2)}      # (nx, ny, nz): non-cubic ones catch a swapped pair
TILT = placement_ref.rotation((0.3, -0.5, 0.2, 0.7))
OFFSET, THICKNESS = 0.25, 0.75       # dyadic, so gap == 0 and gap == thickness can be planted
MOVING = dict(lin=(0.5, -0.25, 0.125), ang=(0.25, 1.0, -0.5))
T_HIT = 0.4375                       # where along axis 1 of the exact cell the first planted particle sits: gap = h / 16


def const_cell(nx, ny, nz):
    """the corner of the cell whose eight samples are equal (len == 0), apart from the exact cell; None on grids too small for one"""
    return (nx - 2, 0, 0) if nx >= 4 else (0, 0, nz - 2) if nz >= 4 else None


def samples_of(nx, ny, nz):
    """(nz, ny, nx): a wavy floor over a nominal span of 6 x 6 x 6 -- phi grows along axis 1 --, whatever the table's cell will be. Cell
    (0, 0, 0) is EXACT: phi = OFFSET + h (t1 - 1/2) with h = 6 / (ny - 1), constant along axes 0 and 2, so that with dyadic t1 every
    lerp of SPEC.md 2i is exact there. const_cell's samples are all 0: under the contact surface, with no direction to push along."""
    u = [6.0 * np.arange(n) / (n - 1) for n in (nx, ny, nz)]
    s = ((u[1] - 2.5)[None, :, None] + 0.4 * np.sin(1.3 * u[0])[None, None, :] + 0.3 * np.cos(0.9 * u[2])[:, None, None]).astype(np.float32)
    h = 6.0 / (ny - 1)
    s[0:2, 0, 0:2] = OFFSET - h / 2
    s[0:2, 1, 0:2] = OFFSET + h / 2
    cc = const_cell(nx, ny, nz)
    if cc is not None:
        s[cc[2]:cc[2] + 2, cc[1]:cc[1] + 2, cc[0]:cc[0] + 2] = 0.0
    return s


def to_world(ps, q):
    """frame coordinates (q0, q1, q2 along the rows of rot) -> simulation space, in binary64 and rounded once: exact in the identity frame
    when the numbers are dyadic"""
    R = ps["rot"].astype(np.float64).reshape(3, 3)
    return (ps["a"].astype(np.float64) + np.asarray(q, np.float64) @ R).astype(np.float32)


def _walk(df, ps, x, axis, sign, want_inside):
    """from x, the first binary32 position along world axis `axis` (direction sign) that SPEC.md 2i finds inside / outside the footprint"""
    x = np.array(x, np.float32)
    for _ in range(64):
        if distance_field_ref.surface(df, ps, x[None, :])["inside"][0] == want_inside:
            return x
        x = x.copy()
        x[axis] = np.nextafter(x[axis], F(sign * np.inf))
    raise AssertionError("no such position within 64 steps")


def planted(df, ps, identity):
    """positions (P, 3) on the places SPEC.md 2i branches at; the first one is a hit in the exact cell. In the identity frame with dyadic
    a and cell they sit there exactly; elsewhere they are near them. Rows: 0 a hit; 1 gap == 0; 2 gap == thickness; 3..5 on a grid plane
    of each axis; 6..11 on the six faces of the footprint (low 0, high 0, low 1, ...: the high ones are in the last cell, where the index
    is clamped); 12..17 outside each face (the first float there in the identity frame); 18 in the constant cell, where there is one."""
    c, dims = df["cell"].astype(np.float64), (df["nx"], df["ny"], df["nz"])
    at = lambda f0, f1, f2: to_world(ps, (f0 * c[0], f1 * c[1], f2 * c[2]))      # noqa: E731
    h = 6.0 / (dims[1] - 1)
    mid = [0.5, T_HIT, 0.5]
    P = [at(0.25, T_HIT, 0.5), at(0.25, 0.5, 0.25), at(0.25, 0.5 - THICKNESS / h, 0.75),
         at(1.0, T_HIT, 0.5), at(0.5, 1.0, 0.5), at(0.5, T_HIT, 1.0)]
    faces = []
    for k in range(3):
        for f in (0.0, float(dims[k] - 1)):
            q = list(mid); q[k] = f
            faces.append((k, -1 if f == 0.0 else +1, at(*q)))
    if identity:        # (world axis k is frame axis k: walk to the last float inside, then to the first one outside)
        on = [_walk(df, ps, x, k, -sign, True) for k, sign, x in faces]
        P += on + [_walk(df, ps, x, k, sign, False) for (k, sign, _), x in zip(faces, on)]
    else:
        P += [x for _, _, x in faces]
        for k in range(3):
            for f in (-1e-3, dims[k] - 1 + 1e-3):
                q = list(mid); q[k] = f
                P.append(at(*q))
    cc = const_cell(*dims)
    if cc is not None:
        P.append(at(cc[0] + 0.5, cc[1] + 0.5, cc[2] + 0.5))
    return np.array(P, np.float32)


def _centred(ps, df):
    """the pose with the footprint's middle -- nominally 6 x 6 x 6 -- at (0.5, -0.25, 0.25)"""
    c, dims = df["cell"].astype(np.float64), (df["nx"], df["ny"], df["nz"])
    half = np.array([(dims[k] - 1) * c[k] / 2 for k in range(3)])
    ps["a"] = (np.array([0.5, -0.25, 0.25]) - half @ ps["rot"].astype(np.float64).reshape(3, 3)).astype(np.float32)
    return ps


def field_cases():
    """-> list of (name, table, pose, planted positions)"""
    out = []
    response = [(0.0, 0.0), (0.4, 0.5), (50.0, 0.0), (0.0, 1.0), (0.4, 0.25)]
    ref = distance_field_ref
    for k, (name, (nx, ny, nz)) in enumerate(GRIDS.items()):
        cell = (6.0 / (nx - 1), 6.0 / (ny - 1), 6.0 / (nz - 1))
        df = ref.make(samples_of(nx, ny, nz), cell, OFFSET, THICKNESS)
        mu, e = response[k]
        ps = ref.pose((-3.0, -3.0, -3.0), friction=mu, restitution=e)
        out.append((name, df, ps, planted(df, ps, True)))
        mu, e = response[(k + 1) % 5]
        ps = _centred(ref.pose((0, 0, 0), rot=TILT, friction=mu, restitution=e, **MOVING), df)
        out.append((name + " turned moving", df, ps, planted(df, ps, False)))
    nx, ny, nz = GRIDS["9x5x17"]
    cell = (6.0 / (nx - 1), 6.0 / (ny - 1), 6.0 / (nz - 1))
    df = ref.make(samples_of(nx, ny, nz), cell, OFFSET, THICKNESS)
    ps = ref.pose((-3.0, -3.0, -3.0), friction=0.4, restitution=0.5, **MOVING)
    out.append(("9x5x17 moving", df, ps, planted(df, ps, True)))
    ps = _centred(ref.pose((0, 0, 0), rot=TILT, friction=0.0, restitution=0.25), df)
    out.append(("9x5x17 turned", df, ps, planted(df, ps, False)))
    # samples of +-3e38 (a difference of two overflows: phi is NaN or infinite and such a cell never hits) and subnormal samples (a cell of
    # nothing else never hits either: the squares of its gradient underflow and len == 0)
    s = samples_of(nx, ny, nz)
    s[8:10, 2:4, 4:8] = np.float32([[[3e38, -3e38, 3e38, 3e38], [-3e38, 3e38, 3e38, -3e38]], [[-3e38, -3e38, 3e38, -3e38], [3e38, 3e38, -3e38, 3e38]]])
    s[12:15, 0, 2:6].view(np.uint32)[...] = np.uint32([[0x000002ca, 0x800002ca, 0x00000001, 0x00000000], [0x80000001, 0x000002ca, 0x00400000, 0x80000000],
                                                       [0x000002ca, 0x00000000, 0x807fffff, 0x00000001]])
    s[12:15, 1, 2:6] = 0.5               # (over the subnormal floor: phi = t1 / 2 but for subnormal terms, which reach G0 and G2, n and the response)
    df = ref.make(s, cell, OFFSET, THICKNESS)
    ps = ref.pose((-3.0, -3.0, -3.0), friction=0.4, restitution=0.5, **MOVING)
    c = [float(t) for t in df["cell"]]
    extra = [to_world(ps, (f0 * c[0], f1 * c[1], f2 * c[2])) for f0, f1, f2 in ((4.5, 2.25, 8.5), (5.25, 2.5, 8.25), (6.5, 2.75, 8.75), (3.5, 2.5, 8.5), (7.25, 2.5, 9.5),
                                                                                 (2.25, 0.25, 12.25), (3.5, 0.5, 12.75), (4.25, 0.75, 13.5), (4.5, 0.25, 13.25), (2.75, 0.5, 13.75))]
    out.append(("9x5x17 extreme samples", df, ps, np.concatenate([planted(df, ps, True), np.array(extra, np.float32)])))
    # the smallest and the largest cell: dyadic a, so the planted particles are exact here too
    df = ref.make(samples_of(3, 2, 4), (2.0 ** -40, 2.0 ** -39, 2.0 ** -40), OFFSET, THICKNESS)
    ps = ref.pose((0.0, 0.0, 0.0), friction=0.4, restitution=0.5)
    out.append(("3x2x4 cell 2^-40", df, ps, planted(df, ps, True)))
    df = ref.make(samples_of(2, 3, 2), (2.0 ** 30, 2.0 ** 29, 2.0 ** 30), OFFSET, THICKNESS)
    ps = ref.pose((-2.0 ** 29, -2.0 ** 29, -2.0 ** 29), friction=0.0, restitution=0.25, **MOVING)
    out.append(("2x3x2 cell 2^30", df, ps, planted(df, ps, True)))
    return out


def state(n, P):
    """the hostile state of n particles with the positions P planted into its first free rows (as many as fit)"""
    x, v, w, special = hostile_state(n, n)
    rows = np.nonzero(w > 0)[0][:len(P)]
    x[rows] = P[:len(rows)]
    return x, v, w, rows


# ---- the prop of the ticking bodies: a sphere sampled on a grid, rising and turning about its centre -------------------------------------------

def sampled_sphere(radius, n=17, pad=0.5, offset=0.0, thickness=None):
    """|p - centre| - radius on n^3 samples over a cube of side 2 radius (1 + pad), the centre in its middle -> (table, side)"""
    side = 2.0 * radius * (1.0 + pad)
    p = np.arange(n) * (side / (n - 1)) - side / 2
    r = np.sqrt(p[:, None, None] ** 2 + p[None, :, None] ** 2 + p[None, None, :] ** 2)
    return distance_field_ref.make(r - radius, side / (n - 1), offset, radius if thickness is None else thickness), side


def pose_about(centre, side, quat, lin=(0, 0, 0), ang=(0, 0, 0), friction=0.0, restitution=0.0):
    """the pose of a cubic table of side `side` whose MIDDLE is at `centre`, turned by `quat`, its middle moving with `lin` while it turns
    with `ang` about the middle: a is the corner, so lin there is lin + ang x (a - centre)"""
    rot = placement_ref.rotation(quat)
    centre, lin, ang = (np.asarray(t, np.float64) for t in (centre, lin, ang))
    a = centre - np.full(3, side / 2) @ rot.astype(np.float64)
    return distance_field_ref.pose(a, rot=rot, lin=lin + np.cross(ang, a - centre), ang=ang, friction=friction, restitution=restitution)


DT = 0.02
TICKS = 6


def ticking_case(case):
    """-> mesh, pins, group keywords, oracle keywords, table, poses (one per tick): a body without a ground plane, held by a few pinned
    particles (they are what the kinematic moves move) and otherwise falling at 0.6 body heights per second, over a sphere that starts
    with its top in the body's underside, rises through it at 0.8 body heights per second and turns about its own middle"""
    from softbodyunity_amd import bunny_surrogate, jelly_cube
    S = 6
    if case == "cube":
        mesh = jelly_cube(8)
        top = mesh.pos[:, 1] > mesh.pos[:, 1].max() - 0.5
        pins = np.nonzero(top & (mesh.pos[:, 0] > mesh.pos[:, 0].max() - 0.5))[0].astype(np.int32)       # one upper edge
        kw = dict(substeps=S, damping=0.05)
        okw = dict(damping=0.05)
    else:
        mesh = bunny_surrogate(target_verts=5000, seed=11)
        pins = np.argsort(mesh.pos[:, 1])[-20:].astype(np.int32)
        kw = dict(substeps=S, distance_compliance=1e-7, volume_compliance=1e-7, bending_compliance=1e-4)
        okw = dict(compliance=(1e-7, 1e-7, 1e-4))
        assert len(mesh.dist_rest) and len(mesh.vol_rest) and len(mesh.bend_rest)
    mesh.inv_mass[pins] = 0.0
    lo, hi = mesh.pos.min(axis=0).astype(np.float64), mesh.pos.max(axis=0).astype(np.float64)
    ext, mid = hi - lo, (lo + hi) / 2
    mesh.vel[:, 1] = -0.6 * float(ext[1])
    mesh.vel[pins] = 0.0
    radius = 0.45 * float(max(ext[0], ext[2]))
    df, side = sampled_sphere(radius, thickness=0.5 * radius)
    rise, ang = np.array([0.0, 0.8 * ext[1], 0.0]), np.array([0.3, 0.8, -0.2])
    poses = []
    for t in range(TICKS):
        centre = np.array([mid[0], lo[1] - radius + 0.08 * ext[1], mid[2]]) + rise * (t * DT)
        half = 0.5 * np.linalg.norm(ang) * t * DT + 0.2
        quat = np.concatenate([ang / np.linalg.norm(ang) * np.sin(half), [np.cos(half)]])
        poses.append(pose_about(centre, side, quat, lin=rise, ang=ang, friction=0.5, restitution=0.1))
    return mesh, pins, kw, okw, df, poses
