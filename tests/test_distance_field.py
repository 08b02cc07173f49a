"""Contacts with signed-distance volumes between two ticks (SPEC.md 2i), without a GPU: the structs' layout, what
sb_group_set_distance_field and sb_group_collide_distance_field refuse before they touch a group, known answers and properties of the
reference the GPU tests compare against (tests/distance_field_ref.py), the branches the GPU module's inputs reach
(tests/distance_field_cases.py), and the baker (softbodyunity_amd.signed_distance_grid)."""
import ctypes as C
import os
import subprocess

import numpy as np

import distance_field_cases
import distance_field_ref
from distance_field_ref import bits
from softbodyunity_amd import native, signed_distance_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _good(nx=3, ny=2, nz=4):
    return native.distance_field(np.arange(nx * ny * nz, dtype=np.float32).reshape(nz, ny, nx), (0.5, 0.25, 2.0), offset=0.125, thickness=0.75)


def _good_pose():
    return native.distance_field_pose((1, 2, 3), rot=distance_field_cases.TILT, lin=(0.5, 0, -1), ang=(0, 2, 0), friction=0.5, restitution=0.25)


def _fp(s):
    return s.ctypes.data_as(C.POINTER(C.c_float))


def bad_distance_fields():
    """(descriptor, samples, the word sb_last_error must hold) for everything SPEC.md 2i refuses in a table itself"""
    rows = []
    for k in range(3):
        for val in (np.nan, np.inf, -np.inf):
            d, s = _good(); d.cell[k] = val
            rows.append((d, s, "NaN or infinite value in the descriptor"))
        for val in (0.0, -0.0, -1e-30):
            d, s = _good(); d.cell[k] = val
            rows.append((d, s, "cell must be > 0"))
    for name in ("offset", "thickness"):
        for val in (np.nan, np.inf, -np.inf):
            d, s = _good(); setattr(d, name, val)
            rows.append((d, s, "NaN or infinite value in the descriptor"))
    for val in (-0.5, -1e-30):
        d, s = _good(); d.offset = val
        rows.append((d, s, "offset must be >= 0"))
    for val in (0.0, -0.5):
        d, s = _good(); d.thickness = val
        rows.append((d, s, "thickness must be > 0"))
    for name in ("nx", "ny", "nz"):
        for val in (1, 0, -3, native.SB_DISTANCE_FIELD_MAX_DIM + 1, 2 ** 31 - 1):
            d, s = _good(); setattr(d, name, val)
            rows.append((d, s, name + " outside"))
    d, s = _good(); d.nx, d.ny, d.nz = 1024, 1024, 129          # every dimension in range, the product over the limit: refused before a sample is read
    rows.append((d, s, "nx * ny * nz over"))
    for flags in (1, 0x80000000):
        d, s = _good(); d.flags = flags
        rows.append((d, s, "flags"))
    for k in range(3):
        d, s = _good(); d.reserved[k] = -1 if k else 1
        rows.append((d, s, "reserved"))
    for at, val in ((0, np.nan), (23, np.inf), (7, -np.inf)):
        d, s = _good(); s = s.copy(); s.reshape(-1)[at] = val
        rows.append((d, s, f"sample at index {at}"))
    d, s = _good(); s = s.copy(); s.reshape(-1)[2] = np.inf; s.reshape(-1)[4] = np.nan
    rows.append((d, s, "sample at index 2"))                 # the FIRST bad sample is named
    return rows


def bad_poses():
    """(pose, the word sb_last_error must hold) for everything SPEC.md 2i refuses in a pose"""
    rows = []
    for name, count in (("a", 3), ("rot", 9), ("lin", 3), ("ang", 3)):
        for k in sorted({0, count - 1}):
            for val in (np.nan, np.inf, -np.inf):
                p = _good_pose(); getattr(p, name)[k] = val
                rows.append((p, "NaN or infinite value in the pose"))
    for name in ("friction", "restitution"):
        for val in (np.nan, np.inf, -np.inf):
            p = _good_pose(); setattr(p, name, val)
            rows.append((p, "NaN or infinite value in the pose"))
    p = _good_pose(); p.friction = -0.125
    rows.append((p, "negative friction"))
    for val in (-0.125, 1.0 + 2.0 ** -23):
        p = _good_pose(); p.restitution = val
        rows.append((p, "restitution outside"))
    for k in range(2):
        p = _good_pose(); p.reserved[k] = 1 - 2 * k
        rows.append((p, "reserved"))
    return rows


def test_the_structs_are_48_and_88_bytes_in_the_header_and_in_ctypes(tmp_path):
    fields = {"sb_distance_field": ["nx", "ny", "nz", "cell", "offset", "thickness", "flags", "reserved"],
              "sb_distance_field_pose": ["a", "rot", "lin", "ang", "friction", "restitution", "reserved"]}
    body = "".join(f'printf("%zu", sizeof({t}));\n' + "".join(f'printf(" %zu", offsetof({t}, {n}));\n' for n in names) + 'printf("\\n");\n' for t, names in fields.items())
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "softbody_group.h"\nint main(void){' + body
                   + 'printf("%d %d %d\\n", SB_DISTANCE_FIELD_SLOTS, SB_DISTANCE_FIELD_MAX_DIM, SB_DISTANCE_FIELD_MAX_SAMPLES); return 0;}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [[int(x) for x in line.split()] for line in subprocess.check_output([str(exe)], text=True).splitlines()]
    for line, (K, names) in zip(got, ((native.SbDistanceField, fields["sb_distance_field"]), (native.SbDistanceFieldPose, fields["sb_distance_field_pose"]))):
        assert line == [C.sizeof(K)] + [getattr(K, n).offset for n in names]
    assert got[0] == [48, 0, 4, 8, 12, 24, 28, 32, 36] and got[1] == [88, 0, 12, 48, 60, 72, 76, 80]
    assert got[2] == [native.SB_DISTANCE_FIELD_SLOTS, native.SB_DISTANCE_FIELD_MAX_DIM, native.SB_DISTANCE_FIELD_MAX_SAMPLES] == [4, 1024, 1 << 27]
    assert (distance_field_ref.SLOTS, distance_field_ref.MAX_DIM, distance_field_ref.MAX_SAMPLES) == (4, 1024, 1 << 27)


def test_null_arguments_bad_slots_tables_and_poses_are_refused_before_the_group_is_touched():
    L = native.lib()
    d, s = _good()
    p = _good_pose()
    assert L.sb_group_set_distance_field(None, 0, C.byref(d), _fp(s)) == native.SB_ERR_INVALID_ARG and b"null group" in L.sb_last_error()
    assert L.sb_group_set_distance_field(None, 0, None, None) == native.SB_ERR_INVALID_ARG
    assert L.sb_group_collide_distance_field(None, 0, C.byref(p)) == native.SB_ERR_INVALID_ARG and b"null group" in L.sb_last_error()
    # the checks come before the group is looked at: a handle that is no group at all is never read
    no_group = C.create_string_buffer(64)
    g = C.cast(no_group, C.c_void_p)
    assert L.sb_group_set_distance_field(g, 0, C.byref(d), None) == native.SB_ERR_INVALID_ARG and b"null samples" in L.sb_last_error()
    assert L.sb_group_collide_distance_field(g, 0, None) == native.SB_ERR_INVALID_ARG and b"null pose" in L.sb_last_error()
    for slot in (-1, native.SB_DISTANCE_FIELD_SLOTS, 2 ** 31 - 1, -2 ** 31):
        assert L.sb_group_set_distance_field(g, slot, C.byref(d), _fp(s)) == native.SB_ERR_INVALID_ARG and b"slot outside" in L.sb_last_error()
        assert L.sb_group_set_distance_field(g, slot, None, None) == native.SB_ERR_INVALID_ARG and b"slot outside" in L.sb_last_error(), "a clear checks its slot too"
        assert L.sb_group_collide_distance_field(g, slot, C.byref(p)) == native.SB_ERR_INVALID_ARG and b"slot outside" in L.sb_last_error()
    rows = bad_distance_fields()
    assert len(rows) == 18 + 6 + 2 + 2 + 15 + 1 + 2 + 3 + 3 + 1
    for slot, (bad, samples, word) in enumerate(rows):
        assert L.sb_group_set_distance_field(g, slot % 4, C.byref(bad), _fp(samples)) == native.SB_ERR_INVALID_ARG
        err = L.sb_last_error().decode()
        assert word in err and "sb_group_set_distance_field" in err, (word, err)
    poses = bad_poses()
    assert len(poses) == 4 * 2 * 3 + 6 + 1 + 2 + 2
    for slot, (bad, word) in enumerate(poses):
        assert L.sb_group_collide_distance_field(g, slot % 4, C.byref(bad)) == native.SB_ERR_INVALID_ARG
        err = L.sb_last_error().decode()
        assert word in err and "sb_group_collide_distance_field" in err, (word, err)
    assert no_group.raw == bytes(64)


def test_the_makers_fill_the_structs():
    d, s = native.distance_field(np.arange(24).reshape(4, 2, 3), (0.5, 0.25, 2.0), offset=0.125, thickness=0.75)
    assert (d.nx, d.ny, d.nz, d.flags, list(d.reserved), d.offset, d.thickness) == (3, 2, 4, 0, [0, 0, 0], 0.125, 0.75) and list(d.cell) == [0.5, 0.25, 2.0]
    assert s.dtype == np.float32 and s.shape == (4, 2, 3) and list(s.reshape(-1)) == list(range(24))
    d, s = native.distance_field(np.zeros((2, 2, 2)), 2.0)
    assert list(d.cell) == [2, 2, 2] and d.offset == 0 and d.thickness == 1
    p = native.distance_field_pose((1, 2, 3))
    assert list(p.a) == [1, 2, 3] and list(p.rot) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(p.lin) + list(p.ang) == [0] * 6 and (p.friction, p.restitution, list(p.reserved)) == (0, 0, [0, 0])
    p = native.distance_field_pose((0, 0, 0), rot=np.arange(9).reshape(3, 3), lin=(1, 2, 3), ang=(4, 5, 6), friction=0.5, restitution=0.25)
    assert list(p.rot) == list(range(9)) and list(p.lin) == [1, 2, 3] and list(p.ang) == [4, 5, 6] and (p.friction, p.restitution) == (0.5, 0.25)
    df = distance_field_ref.make(np.arange(24).reshape(4, 2, 3), (0.5, 0.25, 2.0), 0.125, 0.75)
    n, samples = distance_field_ref.to_native(df)
    assert (n.nx, n.ny, n.nz) == (3, 2, 4) and samples is df["s"] and list(n.cell) == [0.5, 0.25, 2.0]
    ps = distance_field_ref.pose((1, 2, 3), rot=distance_field_cases.TILT, **distance_field_cases.MOVING)
    pn = distance_field_ref.pose_to_native(ps)
    assert np.array_equal(bits(np.array(pn.rot[:], np.float32)), bits(ps["rot"])) and list(pn.lin) == [0.5, -0.25, 0.125]


# ---- known answers ---------------------------------------------------------------------------------------------------------------------------

def _one(x, v, df, ps, w=1.0):
    x, v = np.array([x], np.float32), np.array([v], np.float32)
    hit = distance_field_ref.apply(x, v, np.array([w], np.float32), df, ps)
    return x[0], v[0], bool(hit[0])


def _plane_field(c, offset, thickness, a1=-1.0):
    """phi = y - c sampled exactly on a 3 x 5 x 4 grid with cell (0.5, 0.25, 2) that stands at a = (-0.5, a1, -1): every sample dyadic"""
    y = a1 + 0.25 * np.arange(5)
    return distance_field_ref.make(np.broadcast_to((y - c)[None, :, None], (4, 5, 3)), (0.5, 0.25, 2.0), offset, thickness), (-0.5, a1, -1.0)


def test_a_plane_field_lifts_a_particle_onto_its_contact_surface_along_y_bit_for_bit():
    c, offset = F(-0.375), F(0.125)
    df, a = _plane_field(c, offset, 0.5)
    x0 = np.float32([0.3, -0.4375, 1.7])                       # phi = -0.0625: 0.1875 under the contact surface y = c + offset = -0.25
    for lin, want in (((0, 0, 0), 0.0), ((0, 0.5, 0), 0.5)):    # the prop at rest, and rising: the particle takes the prop's normal velocity
        ps = distance_field_ref.pose(a, lin=lin)
        x, v, hit = _one(x0, (0.25, -1.0, 0.5), df, ps)
        assert hit and np.array_equal(bits(x), bits(np.float32([0.3, c + offset, 1.7]))), x      # n = (0, 1, 0) exactly
        assert np.array_equal(bits(v), bits(np.float32([0.25, want, 0.5]))), v                    # frictionless: the normal part is the prop's
    ps = distance_field_ref.pose(a, friction=50.0)
    x, v, hit = _one(x0, (0.25, -1.0, 0.5), df, ps)
    assert hit and np.array_equal(bits(v), bits(np.float32([0.0, 0.0, 0.0]))), "stick gives +0"
    ps = distance_field_ref.pose(a, restitution=1.0)
    x, v, hit = _one(x0, (0.25, -1.0, 0.5), df, ps)
    assert hit and np.array_equal(bits(v), bits(np.float32([0.25, 1.0, 0.5])))
    # a prop turning about a's y axis carries a stuck particle along: vc = ang x (x' - a)
    ps = distance_field_ref.pose(a, ang=(0, 2, 0), friction=50.0)
    x, v, hit = _one(x0, (0.0, -1.0, 0.0), df, ps)
    r = x - np.float32(a)
    assert hit and np.array_equal(bits(v), bits(np.float32([F(2) * r[2] - F(0) * r[1], F(0) * r[0] - F(0) * r[2], F(0) * r[1] - F(2) * r[0]])))
    # on the contact surface, above it, and thickness under it: not touched
    ps = distance_field_ref.pose(a)
    for y in (-0.25, -0.125, -0.75, -0.875):
        x, v, hit = _one((0.3, y, 1.7), (0.25, -1.0, 0.5), df, ps)
        assert not hit and np.array_equal(bits(x), bits(np.float32([0.3, y, 1.7]))), y
    assert _one((0.3, -0.7421875, 1.7), (0, 0, 0), df, ps)[2], "just less than thickness under it: hit"
    assert not _one(x0, (0.25, -1.0, 0.5), df, ps, w=0.0)[2], "pinned"


def test_a_separating_particle_keeps_its_velocity_but_not_its_position_and_the_rest_keeps_every_bit():
    df, a = _plane_field(0.0, 0.0, 0.5, a1=-0.75)
    ps = distance_field_ref.pose(a, friction=0.5, restitution=0.5)
    v0 = np.array([0.3, 0.9, -0.1], np.float32)
    v0.view(np.uint32)[2] = 0x80000001        # a subnormal: any arithmetic on it would show
    x, v, hit = _one((0.1, -0.25, 0.5), v0, df, ps)
    assert hit and np.array_equal(bits(v), bits(v0)) and x[1] == 0.0
    pool = np.array([0x80000000, 0x00000001, 0x7fc12345, 0xffc00001, 0x7f800001, 0x7f800000, 0xff800000, 0x3f000000], np.uint32)
    x = np.zeros((8, 3), np.float32); v = np.zeros((8, 3), np.float32)
    for c in range(3):
        x.view(np.uint32)[:, c] = np.roll(pool, c); v.view(np.uint32)[:, c] = np.roll(pool, c + 3)
    x[7] = (0.1, -0.25, 0.5)                                # under the surface, pinned
    x[6] = (0.1, -0.625, 0.5)                               # too deep
    x[5] = (0.1, 0.0, 0.5)                                  # on the surface: gap == 0
    x[4] = (0.75, -0.25, 0.5)                               # beside the volume
    w = np.float32([1, 1, 1, 1, 1, 1, 1, 0])
    x0, v0 = x.copy(), v.copy()
    hit = distance_field_ref.apply(x, v, w, df, ps)
    assert not hit[4:].any() and np.array_equal(bits(x[~hit]), bits(x0[~hit])) and np.array_equal(bits(v[~hit]), bits(v0[~hit]))
    assert not hit[np.isnan(x0).any(axis=1) | np.isinf(x0).any(axis=1)].any(), "NaN and infinite positions are never hit"


def test_a_constant_cell_never_hits_and_axes_are_not_swapped():
    df = distance_field_ref.make(np.full((2, 2, 2), -0.25), 1.0, 0.0, 1.0)
    assert not _one((0.5, 0.5, 0.5), (0, -1, 0), df, distance_field_ref.pose((0, 0, 0)))[2]
    # phi grows along axis 0, 1 or 2 alone on a 3 x 4 x 5 grid: the push goes along that row of rot
    R = distance_field_cases.TILT
    for k in range(3):
        idx = np.arange((3, 4, 5)[k], dtype=np.float64)
        shape = [1, 1, 1]; shape[2 - k] = -1
        s = np.broadcast_to((0.5 * idx - 0.625).reshape(shape), (5, 4, 3))
        df = distance_field_ref.make(s, (0.5, 0.5, 0.5), 0.0, 1.0)
        ps = distance_field_ref.pose((0, 0, 0), rot=R)
        q = np.full(3, 0.625); q[k] = 0.5                      # phi = 0.5 - 0.625 = -0.125 there
        x0 = distance_field_cases.to_world(ps, q)
        g = distance_field_ref.surface(df, ps, x0[None, :])
        assert g["hit"][0] and abs(float(g["gap"][0]) - 0.125) < 1e-6
        assert np.allclose([float(g["n"][c][0]) for c in range(3)], R[k], atol=1e-6), k


# ---- properties of the reference on random contacts ------------------------------------------------------------------------------------------

N_CLOUD = 200_000


def _phi64(df, ps, x):
    """the trilinear interpolation of SPEC.md 2i in binary64 from the binary32 inputs: (inside, phi)"""
    a, R, cell = ps["a"].astype(np.float64), ps["rot"].astype(np.float64).reshape(3, 3), df["cell"].astype(np.float64)
    dims = (df["nx"], df["ny"], df["nz"])
    s = df["s"].astype(np.float64).reshape(dims[2], dims[1], dims[0])
    f = ((x.astype(np.float64) - a) @ R.T) / cell
    inside = np.ones(len(x), bool)
    for k in range(3):
        inside &= (f[:, k] >= 0) & (f[:, k] <= dims[k] - 1)
    i = [np.clip(np.where(inside, f[:, k], 0).astype(np.int64), 0, dims[k] - 2) for k in range(3)]
    t = [f[:, k] - i[k] for k in range(3)]
    phi = 0.0
    for c in (0, 1):
        for b in (0, 1):
            for aa in (0, 1):
                wgt = (t[0] if aa else 1 - t[0]) * (t[1] if b else 1 - t[1]) * (t[2] if c else 1 - t[2])
                phi = phi + wgt * s[i[2] + c, i[1] + b, i[0] + aa]
    return inside, phi


def test_on_a_sampled_sphere_non_hits_keep_every_bit_and_hits_end_no_further_from_the_contact_surface():
    """The bound, derived. psi = |p - c| - R is the true distance: |grad psi| = 1, and its Hessian has the eigenvalues 0 and 1/r twice, so
    every second derivative is at most 1/r in magnitude, r >= r_min over the cells a hit can touch. I is the trilinear interpolant with
    spacing h.
    VALUE. Multilinear interpolation errs by at most sum_k h^2 / 8 max|d_kk psi|: E = 3 h^2 / (8 r_min).
    DIRECTION. A component of grad I is a convex combination of difference quotients of psi along cell edges, each equal to that
    derivative of psi somewhere on the edge, no further than the cell's diagonal h sqrt 3 from x: it errs by at most sqrt 3 h / r_min,
    the vector by 3 h / r_min, and the unit vector n against the radial unit vector u by at most twice that: D = 6 h / r_min.
    AFTER THE PUSH x' = x + gap n with gap = offset - I(x): psi is 1-Lipschitz and grows by exactly gap along u, so
    psi(x') = psi(x) + gap + d with |d| <= gap D, hence psi(x') - offset = -(I - psi)(x) + d and
    |I(x') - offset| <= 2 E + gap D, plus the roundings of binary32 on values below 8 (thirty of them: 30 * 2^-24 * 8 < 2^-16).
    That is no larger than the gap before wherever gap (1 - D) >= 2 E + 2^-16. Neither figure is tuned: both follow from h, R, offset,
    thickness."""
    R_, n, offset, thickness = 2.0, 65, 0.125, 0.5
    df, side = distance_field_cases.sampled_sphere(R_, n=n, pad=0.5, offset=offset, thickness=thickness)
    h = side / (n - 1)
    r_min = R_ + offset - thickness - h * np.sqrt(3)
    E, D, ROUND = 3 * h * h / (8 * r_min), 6 * h / r_min, 2.0 ** -16
    assert D < 0.5 and E < 0.01
    rng = np.random.default_rng(23)
    x0 = rng.uniform(-3.5, 3.5, size=(N_CLOUD, 3)).astype(np.float32)
    v0 = rng.uniform(-2, 2, size=(N_CLOUD, 3)).astype(np.float32)
    w = rng.choice(np.float32([0.5, 1, 2]), size=N_CLOUD).astype(np.float32)
    w[::7] = 0
    for quat, motion in (((0, 0, 0, 1), {}), ((0.3, -0.5, 0.2, 0.7), distance_field_cases.MOVING)):
        ps = distance_field_cases.pose_about((0.25, -0.125, 0.5), side, quat, friction=0.3, restitution=0.5, **motion)
        x, v = x0.copy(), v0.copy()
        hit = distance_field_ref.apply(x, v, w, df, ps)
        assert hit.sum() > 10_000 and not hit[w == 0].any()
        assert np.array_equal(bits(x[~hit]), bits(x0[~hit])) and np.array_equal(bits(v[~hit]), bits(v0[~hit])), "non-hits keep every bit"
        in0, phi0 = _phi64(df, ps, x0)
        in1, phi1 = _phi64(df, ps, x)
        assert in0[hit].all() and in1[hit].all()
        gap0, off1 = offset - phi0[hit], np.abs(phi1[hit] - offset)
        assert (gap0 > -ROUND).all() and (gap0 < thickness + ROUND).all()
        bound = 2 * E + gap0 * D + ROUND
        print("hits %d, worst |phi(x') - offset| %.3e against a bound of %.3e there" % (hit.sum(), off1.max(), bound[np.argmax(off1)]))
        assert (off1 <= bound).all()
        improves = gap0 * (1 - D) >= 2 * E + ROUND
        assert improves.sum() > 0.9 * hit.sum() and (off1[improves] <= gap0[improves]).all(), "a hit ends no further from the contact surface than it was"
        # no hit particle approaches the moving prop afterwards (restitution 0.5 > 0: it leaves), to the same count of roundings
        g = distance_field_ref.surface(df, ps, x0)
        nrm = np.stack([g["n"][c] for c in range(3)], axis=1).astype(np.float64)
        vc = ps["lin"].astype(np.float64) + np.cross(ps["ang"].astype(np.float64), x.astype(np.float64) - ps["a"].astype(np.float64))
        un = ((v.astype(np.float64) - vc) * nrm).sum(axis=1)
        assert (un[hit] >= -2.0 ** -16 * 8).all()


def test_the_inputs_of_the_gpu_module_reach_every_branch():
    cases = distance_field_cases.field_cases()
    names = [name for name, *_ in cases]
    assert len(cases) == 15 and all(g in names and g + " turned moving" in names for g in distance_field_cases.GRIDS)
    cells = [float(c) for _, df, *_ in cases for c in df["cell"]]
    assert min(cells) == 2.0 ** -40 and max(cells) == 2.0 ** 30
    assert any(np.abs(df["s"]).max() > 2.9e38 for _, df, *_ in cases) and any(((df["s"] != 0) & (np.abs(df["s"]) < 1e-38)).any() for _, df, *_ in cases)
    per_size = {}
    for n in distance_field_cases.SIZES:
        trace = distance_field_ref.new_trace()
        for name, df, ps, P in cases:
            x, v, w, rows = distance_field_cases.state(n, P)
            hit = distance_field_ref.apply(x, v, w, df, ps, trace)
            assert hit[rows[0]], (n, name, "the first planted particle is a hit")
        per_size[n] = trace
    print(per_size[4099])
    for n in (1023, 1024, 1025, 4099):
        assert all(per_size[n][k] > 0 for k in distance_field_ref.TRACE_KEYS), (n, per_size[n])      # no key may be zero
    total = {k: sum(t[k] for t in per_size.values()) for k in distance_field_ref.TRACE_KEYS}
    assert all(total[k] > 0 for k in distance_field_ref.TRACE_KEYS), total
    # the planted places, exactly, in every identity-frame case with dyadic cells
    for name, df, ps, P in cases:
        if "turned" in name:
            continue
        dims = (df["nx"], df["ny"], df["nz"])
        g = distance_field_ref.surface(df, ps, P)
        assert g["hit"][0] and g["gap"][0] == F(6.0 / (dims[1] - 1) / 16), name
        assert g["gap"][1] == 0 and g["inside"][1] and not g["hit"][1], (name, g["gap"][:3])
        assert g["gap"][2] == df["thickness"] and g["inside"][2] and not g["hit"][2], (name, g["gap"][:3])
        if "1024" not in name:                                 # (cell 6 / 1023 is not dyadic: near the plane there)
            assert g["f"][0][3] == 1, name
        assert g["f"][1][4] == 1 and g["f"][2][5] == 1, name
        assert g["inside"][6:12].all() and not g["inside"][12:18].any(), name
        for k in range(3):
            assert g["f"][k][6 + 2 * k] == 0 and g["f"][k][7 + 2 * k] == dims[k] - 1 and g["i0"][k][7 + 2 * k] == dims[k] - 1 and g["i"][k][7 + 2 * k] == dims[k] - 2, (name, k)
        if distance_field_cases.const_cell(*dims) is not None:
            assert g["inside"][18] and g["length"][18] == 0 and g["gap"][18] == F(0.25) and not g["hit"][18], name
    # the overflowing cells never hit, whatever is in them; the ones over a subnormal floor do, with subnormal parts in the normal
    name, df, ps, P = cases[12]
    assert name == "9x5x17 extreme samples"
    g = distance_field_ref.surface(df, ps, P[19:24])
    assert g["inside"].all() and (~np.isfinite(g["phi"])).sum() >= 3 and not g["hit"][~np.isfinite(g["phi"])].any()
    g = distance_field_ref.surface(df, ps, P[24:])
    tiny = lambda a: (a != 0) & (np.abs(a) < 1e-37)       # noqa: E731
    assert g["inside"].all() and g["hit"].sum() >= 2 and (tiny(g["G"][0]) | tiny(g["G"][2])).any() and any(tiny(g["n"][c]).any() for c in range(3))


# ---- the baker -------------------------------------------------------------------------------------------------------------------------------

def _box_mesh(lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    V = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])      # vertex 4 i + 2 j + k
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]      # outward
    T = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))])
    return V, T


def test_the_baker_gives_a_cubes_analytic_distance_inside_and_outside():
    lo, hi = np.array([-0.5, 0.25, 1.0]), np.array([1.0, 1.5, 2.0])
    V, T = _box_mesh(lo, hi)
    assert len(T) == 12
    cell, padding = (0.17, 0.13, 0.11), 0.4
    s, origin = signed_distance_grid(V, T, cell, padding)
    nz, ny, nx = s.shape
    assert s.dtype == np.float32 and np.allclose(origin, lo - padding) and all(origin[k] + ((nx, ny, nz)[k] - 1) * cell[k] >= hi[k] + padding - 1e-9 for k in range(3))
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    P = origin + np.stack([ix, iy, iz], axis=-1) * np.asarray(cell)
    q = np.abs(P - (lo + hi) / 2) - (hi - lo) / 2
    want = np.linalg.norm(np.maximum(q, 0), axis=-1) + np.minimum(q.max(axis=-1), 0)
    diagonal = np.linalg.norm((np.array([nx, ny, nz]) - 1) * np.asarray(cell))
    tol = 4 * float(np.spacing(F(diagonal)))                  # 4 float32 ulps of the grid's diagonal; float64 brute force errs far below one
    assert (want < 0).sum() > 100 and (want > 0).sum() > 1000
    assert np.abs(s.astype(np.float64) - want).max() <= tol, (np.abs(s - want).max(), tol)
    assert np.array_equal(s < 0, want.astype(np.float32) < 0)


def test_the_baker_signs_a_concave_l_shaped_prism():
    poly = np.array([(0, 0), (2, 0), (2, 1), (1, 1), (1, 2), (0, 2)], np.float64)       # counter-clockwise, star-shaped about vertex 0
    m = len(poly)
    V = np.concatenate([np.c_[poly, np.zeros(m)], np.c_[poly, np.ones(m)]])
    T = [(0, k + 1, k) for k in range(1, m - 1)] + [(m, m + k, m + k + 1) for k in range(1, m - 1)]       # bottom (facing -z), top
    for k in range(m):
        a, b = k, (k + 1) % m
        T += [(a, b, m + b), (a, m + b, m + a)]
    s, origin = signed_distance_grid(V, np.array(T), 0.21, 0.3)
    nz, ny, nx = s.shape
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    P = origin + np.stack([ix, iy, iz], axis=-1) * 0.21
    x, y, z = P[..., 0], P[..., 1], P[..., 2]
    inside = (((x > 0) & (x < 2) & (y > 0) & (y < 1)) | ((x > 0) & (x < 1) & (y > 0) & (y < 2))) & (z > 0) & (z < 1)
    clear = np.abs(s) > 1e-9
    assert clear.sum() > 0.99 * clear.size and inside.sum() > 50 and (~inside).sum() > 500
    assert np.array_equal(s[clear] < 0, inside[clear])
    # in the notch, outside the prism but inside its convex hull, the distance is to the nearer of the two inner walls
    notch = (x > 1) & (y > 1) & (x < 2) & (y < 2) & (z > 0) & (z < 1)
    assert notch.sum() > 10 and np.allclose(s[notch], np.minimum(x - 1, y - 1)[notch], atol=1e-6)
