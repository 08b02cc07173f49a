"""Render tangents (SPEC.md 6c), the parts that need no GPU: the entry points exist and reject null handles, and the numpy reference the GPU
tests compare against is itself right -- against its float64 twin on the fixed 12^3 case, and exactly on hand-made triangles."""
import ctypes as C
import os
import sys

import numpy as np

from tangent_ref import bits, lattice_uvs, tangent_coefficients, tangents_ref, tangents_ref64
from softbodyunity_amd import jelly_cube, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_entry_points_are_bound_and_reject_null_handles():
    L = native.lib()
    for name in ("sb_set_render_uvs", "sb_readback_get_tangents", "sb_group_set_render_uvs", "sb_group_readback_get_tangents"):
        assert name in native.SIGNATURES, name
    uv = np.zeros((1, 2), np.float32)
    fp = C.POINTER(C.c_float)
    q = fp()
    assert L.sb_set_render_uvs(None, uv.ctypes.data_as(fp), 1) == native.SB_ERR_INVALID_ARG and b"sb_set_render_uvs" in L.sb_last_error()
    assert L.sb_group_set_render_uvs(None, uv.ctypes.data_as(fp), 1) == native.SB_ERR_INVALID_ARG and b"sb_group_set_render_uvs" in L.sb_last_error()
    assert L.sb_readback_get_tangents(None, C.byref(q)) == native.SB_ERR_INVALID_ARG and b"sb_readback_get_tangents" in L.sb_last_error()
    assert L.sb_group_readback_get_tangents(None, C.byref(q)) == native.SB_ERR_INVALID_ARG and b"sb_group_readback_get_tangents" in L.sb_last_error()


def test_the_float32_reference_agrees_with_float64_on_the_lattice_case(oracle_mod):
    from readback_bench import surface_triangles
    n = 12
    mesh = jelly_cube(n, heterogeneous=True)
    tri = surface_triangles(n)
    uv = lattice_uvs(n)
    used = np.unique(tri)
    assert used.size == 728 and tri.shape[0] == 1452
    nrm = oracle_mod.vertex_normals(mesh.pos, tri)
    t32 = tangents_ref(mesh.pos, nrm, tri, uv)
    t64, n64 = tangents_ref64(mesh.pos, tri, uv)
    assert t32.dtype == np.float32 and t32.shape == (mesh.n, 4)
    a, b = t32[used].astype(np.float64), t64[used]
    length = np.linalg.norm(a[:, :3], axis=1)
    figures = dict(degenerate=int((length == 0).sum()), plus=int((a[:, 3] == 1).sum()), minus=int((a[:, 3] == -1).sum()),
                   unit=float(np.abs(length - 1).max()), ortho=float(np.abs(np.einsum("ij,ij->i", a[:, :3], nrm[used].astype(np.float64))).max()),
                   f32_f64=float(np.abs(a[:, :3] - b[:, :3]).max()))
    print(figures)
    assert figures["degenerate"] == 0
    assert figures["plus"] == 364 and figures["minus"] == 364
    assert np.array_equal(a[:, 3], b[:, 3])
    assert figures["unit"] <= 3e-6
    assert figures["ortho"] <= 1e-5
    assert figures["f32_f64"] <= 1e-5
    # a particle in no surface triangle
    inner = np.setdiff1d(np.arange(mesh.n), used)
    assert inner.size == 10 ** 3 and np.array_equal(bits(t32[inner]), bits(np.tile(np.float32([0, 0, 0, 1]), (inner.size, 1))))


def test_uv_degenerate_triangles_contribute_nothing():
    rng = np.random.default_rng(2)
    p = rng.uniform(-1, 1, size=(7, 3)).astype(np.float32)
    uv = rng.uniform(0, 1, size=(7, 2)).astype(np.float32)
    uv[4] = uv[0]                                           # triangle (0, 4, 1): two corners with equal UVs
    uv[5] = (0.0, 0.0); uv[6] = (1e-30, 0.0)                # triangle (5, 6, 3) after uv[3] below: UV differences of 1e-30
    good = np.array([[0, 1, 2], [0, 2, 1]], np.int32)
    k = tangent_coefficients(uv, np.array([[0, 1, 2], [0, 4, 1]], np.int32))
    assert k.dtype == np.float32 and k.shape == (2, 4) and np.isfinite(k).all()
    assert k[0].any() and not k[1].any(), "two corners with equal UVs give k = 0"
    uv3 = uv.copy(); uv3[3] = (0.0, 1e-30)
    with np.errstate(all="ignore"):
        det = np.float32(1e-30) * np.float32(1e-30)
        assert not np.isfinite(np.float32(1e-30) / det)                                   # what the rule is for
    assert not tangent_coefficients(uv3, np.array([[5, 6, 3]], np.int32)).any(), "a quotient that overflows gives k = 0"
    # the sums with the degenerate triangles present are those without them
    tri_all = np.array([[0, 1, 2], [0, 4, 1], [0, 2, 1], [5, 6, 3]], np.int32)
    n = np.zeros((7, 3), np.float32); n[:, 2] = 1
    with_deg = tangents_ref(p, n, tri_all, uv3)
    without = tangents_ref(p, n, good, uv3)
    assert np.array_equal(bits(with_deg), bits(without))
    # vertex 4 (only in a degenerate triangle), vertices 3, 5 and 6 (only in the overflowing one): (0, 0, 0, 1)
    assert np.array_equal(bits(with_deg[[3, 4, 5, 6]]), bits(np.tile(np.float32([0, 0, 0, 1]), (4, 1))))
    assert np.linalg.norm(with_deg[2, :3]) > 0.5


def test_a_right_triangle_with_axis_aligned_uvs_is_exact():
    p = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]])       # (vertex 3 is in no triangle)
    tri = np.int32([[0, 1, 2]])
    n = np.float32([[0, 0, 1]] * 3 + [[0, 0, 0]])
    uv = np.float32([[0, 0], [1, 0], [0, 1], [0.5, 0.5]])
    t = tangents_ref(p, n, tri, uv)
    assert np.array_equal(t[:3], np.tile(np.float32([1, 0, 0, 1]), (3, 1)))
    assert np.array_equal(bits(t[3]), bits(np.float32([0, 0, 0, 1])))
    uv[:, 0] = -uv[:, 0]
    t = tangents_ref(p, n, tri, uv)
    assert np.array_equal(t[:3], np.tile(np.float32([-1, 0, 0, -1]), (3, 1)))
    t64, n64 = tangents_ref64(p, tri, uv)
    assert np.array_equal(t64[:3], np.tile([-1.0, 0, 0, -1], (3, 1))) and np.array_equal(n64[:3], np.tile([0.0, 0, 1], (3, 1)))
