"""Surface forces between two ticks (SPEC.md 2e), without a GPU: known answers of the reference the GPU tests compare against
(tests/surface_force_ref.py), chosen so that nothing rounds; its properties; the record's layout in the header, the ctypes twin and the C#
binding; and what the entry point refuses before it touches a group."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import surface_force_ref
from softbodyunity_amd import make_surface_force, native
from surface_force_ref import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TRI = np.array([[0, 1, 2]])
CUBE = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], np.float32)
# the unit cube's skin, every triangle wound so that its right-hand normal points outwards
CUBE_TRI = np.array([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [3, 6, 2], [3, 7, 6], [0, 4, 7], [0, 7, 3], [1, 2, 6], [1, 6, 5]])


def _right_triangle():
    x = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    return x, np.zeros((3, 3), np.float32), np.ones(3, np.float32)


# ---- known answers, exact ---------------------------------------------------------------------------------------------------------------------

def test_wind_along_the_normal_of_a_unit_right_triangle():
    # f = (0, 0, 1), L2 = L = 1, hn = (0.5 * 12) / 6 = 1, u = (0, 0, 2), q = 2, un = (0, 0, 2), J = 1 * (1 * 2) = 2 per corner
    x, v, w = _right_triangle()
    surface_force_ref.apply(x, v, w, TRI, wind=(0, 0, 2), normal=12.0, dt=0.5)
    assert v.tolist() == [[0, 0, 2]] * 3


def test_wind_across_the_same_triangle():
    x, v, w = _right_triangle()
    surface_force_ref.apply(x, v, w, TRI, wind=(2, 0, 0), tangential=12.0, normal=0.0, dt=0.5)
    assert v.tolist() == [[2, 0, 0]] * 3
    # ... and the normal coefficient alone does nothing to a wind in the plane, the tangential one nothing to a wind along the normal
    x, v, w = _right_triangle()
    surface_force_ref.apply(x, v, w, TRI, wind=(2, 0, 0), normal=12.0, dt=0.5)
    surface_force_ref.apply(x, v, w, TRI, wind=(0, 0, 2), tangential=12.0, dt=0.5)
    assert not v.any()


def test_pressure_inflates_the_unit_cube_and_the_velocities_sum_to_zero():
    # every triangle: |f| = 1 along the outward axis, hp = 1, J = f; a corner sums the J of its incident triangles: every component
    # comes out +-1 or +-2 (one or two triangles of that face meet the corner), and the faces cancel in the total
    v = np.zeros((8, 3), np.float32)
    surface_force_ref.apply(CUBE, v, np.ones(8, np.float32), CUBE_TRI, pressure=12.0, dt=0.5)
    assert set(np.abs(v).ravel().tolist()) == {1.0, 2.0}
    assert (np.sign(v) == np.sign(CUBE - 0.5)).all(), "outwards"
    assert v.sum(axis=0).tolist() == [0, 0, 0]
    v2 = np.zeros((8, 3), np.float32)
    surface_force_ref.apply(CUBE, v2, np.ones(8, np.float32), CUBE_TRI, pressure=-12.0, dt=0.5)
    assert np.array_equal(v2, -v), "a negative pressure deflates"


# ---- properties -------------------------------------------------------------------------------------------------------------------------------

def test_a_body_that_moves_with_the_wind_feels_nothing():
    rng = np.random.default_rng(1)
    x = (CUBE * np.float32(1.5) + rng.uniform(-0.2, 0.2, size=(8, 3))).astype(np.float32)
    v = np.tile(np.float32([0.75, -1.5, 0.25]), (8, 1))        # (a + a) + a and / 3 are exact for these
    before = v.copy()
    surface_force_ref.apply(x, v, np.ones(8, np.float32), CUBE_TRI, wind=(0.75, -1.5, 0.25), normal=3.0, tangential=1.0, dt=0.02)
    assert np.array_equal(v, before)


def test_who_keeps_the_bits_of_its_velocity():
    # 0 pinned; 1, 2 free; 3 in no triangle; 4 in skipped triangles only (a zero-area one, a subnormal-area one, an overflowing one)
    x = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [2, 0, 0], [1e-20, 0, 0], [0, 1e-20, 0], [3e30, 0, 0], [0, 3e30, 0]], np.float32)
    tri = np.array([[0, 1, 2], [4, 1, 1], [4, 4, 4], [0, 5, 6], [0, 7, 8], [4, 0, 0]])
    w = np.ones(9, np.float32); w[0] = 0
    v = np.zeros((9, 3), np.float32)
    odd = np.array([0x80000000, 0x7fc0beef, 0xffc00001], np.uint32)      # -0, two NaN payloads
    for p in (0, 3, 4):
        v.view(np.uint32)[p] = odd
    before = v.copy()
    one = np.float32(1)
    for t in (1, 2, 3, 4, 5):
        assert surface_force_ref.triangle_impulse(x, v, tri[t], np.zeros(3, np.float32), one, one, one) is None, t
    assert surface_force_ref.triangle_impulse(x, v, tri[0], np.zeros(3, np.float32), one, one, one) is not None
    e1, e2 = x[5] - x[0], x[6] - x[0]
    assert 0 < e1[0] * e2[1] < np.finfo(np.float32).tiny, "triangle 3 has a subnormal doubled area"
    surface_force_ref.apply(x, v, w, tri, wind=(1, 2, 3), normal=2.0, tangential=1.0, pressure=0.5, dt=0.5)
    assert np.array_equal(bits(v[[0, 3, 4, 5, 6, 7, 8]]), bits(before[[0, 3, 4, 5, 6, 7, 8]]))
    # (the pinned corner's NaN velocity components reach its triangle's other corners through vt: canonical NaN there)
    assert (bits(v[1]) != 0).any() and np.array_equal(bits(v[1]), bits(v[2]))


def test_the_area_thresholds():
    # f = (0, 0, s * s): L2 = s^4. 2^-24: L2 = 2^-96, the smallest that counts; just below it, skipped; s = 2^32: L2 = +inf, skipped
    wind, v = np.float32([0, 0, 1]), np.zeros((3, 3), np.float32)

    def J(s):
        x = np.array([[0, 0, 0], [s, 0, 0], [0, s, 0]], np.float32)
        return surface_force_ref.triangle_impulse(x, v, (0, 1, 2), wind, np.float32(1), np.float32(0), np.float32(0))
    assert J(2.0 ** -24) is not None and J(np.nextafter(np.float32(2.0 ** -24), np.float32(0))) is None
    assert J(2.0 ** 31) is not None and J(2.0 ** 32) is None
    x = np.array([[0, 0, 0], [np.nan, 0, 0], [0, 1, 0]], np.float32)
    assert surface_force_ref.triangle_impulse(x, v, (0, 1, 2), wind, np.float32(1), np.float32(0), np.float32(0)) is None, "a NaN area"


def test_a_nan_result_is_stored_as_the_canonical_quiet_nan():
    x, v, w = _right_triangle()
    v[0] = (np.inf, 0, 0); v[1] = (0, 0, -np.inf)
    v.view(np.uint32)[2, 1] = 0xffc12345
    surface_force_ref.apply(x, v, w, TRI, wind=(0, 0, 1), normal=6.0, tangential=6.0, dt=1.0)
    assert np.isnan(v).any() and (bits(v)[np.isnan(v)] == 0x7fc00000).all()


def test_a_shared_vertex_adds_in_ascending_triangle_order():
    # vertex 0 is the corner of three triangles whose J along z are 2^24, 1 and -2^24 (pressure; areas 2^24, 1, 2^24 with opposite winding):
    # (2^24 + 1) + -2^24 = 0 in float32, while any other order gives 1
    big = np.float32(2.0 ** 24)
    x = np.array([[0, 0, 0], [big, 0, 0], [0, 1, 0], [1, 0, 0], [0, big, 0]], np.float32)
    tri = np.array([[0, 1, 2], [0, 3, 2], [0, 4, 3]])
    v = np.zeros((5, 3), np.float32)
    surface_force_ref.apply(x, v, np.ones(5, np.float32), tri, pressure=6.0, dt=1.0)
    assert v[0].tolist() == [0, 0, 0] and v[1].tolist() == [0, 0, float(big)] and v[4].tolist() == [0, 0, -float(big)]
    v = np.zeros((5, 3), np.float32)
    surface_force_ref.apply(x, v, np.ones(5, np.float32), tri[[0, 2, 1]], pressure=6.0, dt=1.0)
    assert v[0].tolist() == [0, 0, 1]
    # a triangle that is listed twice counts twice
    v = np.zeros((5, 3), np.float32)
    surface_force_ref.apply(x, v, np.ones(5, np.float32), tri[[1, 1]], pressure=6.0, dt=1.0)
    assert v[0].tolist() == [0, 0, 2]


# ---- interface --------------------------------------------------------------------------------------------------------------------------------

def test_the_record_is_44_bytes_in_the_header_in_ctypes_and_in_csharp(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "softbody_group.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(sb_surface_force), offsetof(sb_surface_force, normal), '
                   'offsetof(sb_surface_force, tangential), offsetof(sb_surface_force, pressure), offsetof(sb_surface_force, dt), '
                   'offsetof(sb_surface_force, flags), offsetof(sb_surface_force, reserved)); return 0;}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    S = native.SbSurfaceForce
    assert got == [C.sizeof(S), S.normal.offset, S.tangential.offset, S.pressure.offset, S.dt.offset, S.flags.offset, S.reserved.offset] == [44, 12, 16, 20, 24, 28, 32]
    cs = open(os.path.join(ROOT, "csharp", "SoftbodyNative.cs")).read()
    body = re.search(r"public struct SbSurfaceForce\s*\{(.*?)\}", cs, re.S).group(1)
    fields = re.findall(r"public (int|uint|float) ([^;]+);", body)
    assert sum(len(names.split(",")) for _, names in fields) == 11           # eleven 4-byte fields
    assert "sb_group_apply_surface_forces(IntPtr g, ref SbSurfaceForce" in cs
    hdr = open(os.path.join(ROOT, "include", "softbody.h")).read()
    assert int(re.search(r"#define\s+SB_ABI_VERSION\s+(\d+)", hdr).group(1)) == 8, "the change is additive"


def bad_records():
    """(record, the word sb_last_error must hold) for everything SPEC.md 2e refuses in the record itself"""
    rows = []
    for name in ("normal", "tangential", "pressure", "dt"):
        for val in (np.nan, np.inf, -np.inf):
            f = make_surface_force(normal=1.0, dt=0.02)
            setattr(f, name, val)
            rows.append((f, name))
    for k in range(3):
        for val in (np.nan, np.inf, -np.inf):
            f = make_surface_force(normal=1.0, dt=0.02)
            f.wind[k] = val
            rows.append((f, "wind"))
    for name, val in (("normal", -1.0), ("normal", -1e-45), ("tangential", -0.5), ("tangential", -1e-45), ("dt", 0.0), ("dt", -0.0), ("dt", -0.02)):
        f = make_surface_force(normal=1.0, dt=0.02)
        setattr(f, name, val)
        rows.append((f, name))
    for flags in (1, 0x80000000):
        f = make_surface_force(normal=1.0, dt=0.02); f.flags = flags
        rows.append((f, "flag"))
    for k in range(3):
        f = make_surface_force(normal=1.0, dt=0.02); f.reserved[k] = -1 if k else 1
        rows.append((f, "reserved"))
    return rows


def test_null_arguments_and_bad_records_are_refused_before_anything_is_touched():
    L = native.lib()
    good = make_surface_force(wind=(1, 2, 3), normal=1.0, tangential=0.5, pressure=-2.0, dt=0.02)
    assert (C.sizeof(good), list(good.wind), good.flags, list(good.reserved)) == (44, [1, 2, 3], 0, [0, 0, 0])
    rows = bad_records()
    assert len(rows) == 4 * 3 + 3 * 3 + 7 + 2 + 3
    for fn, name in ((L.sb_group_apply_surface_forces, "sb_group_apply_surface_forces"),):
        assert fn(None, C.byref(good)) == native.SB_ERR_INVALID_ARG and b"null" in L.sb_last_error()
        assert fn(None, None) == native.SB_ERR_INVALID_ARG
        # the record's checks come before the handle is looked at: a handle that is no group at all is never read
        nobody = C.create_string_buffer(64)
        assert fn(C.cast(nobody, C.c_void_p), None) == native.SB_ERR_INVALID_ARG and b"null" in L.sb_last_error()
        for f, word in rows:
            assert fn(C.cast(nobody, C.c_void_p), C.byref(f)) == native.SB_ERR_INVALID_ARG
            err = L.sb_last_error().decode()
            assert word in err and err.startswith(name + ":"), (word, err)
        assert nobody.raw == bytes(64)
