"""Embedded render vertices (SPEC.md 6b), the parts that need no GPU: the entry points exist and reject bad arguments, mesh.embed_vertices
binds a visual mesh to a tet cage, and the numpy reference the GPU tests compare against is itself right."""
import ctypes as C
import os
import sys

import numpy as np

from embedding_ref import embedded_ref, embedded_ref64
from softbodyunity_amd import bunny_surrogate, embed_vertices, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_bound_and_reject_null_handles():
    L = native.lib()
    assert "sb_set_render_embedding" in native.SIGNATURES and "sb_group_set_render_embedding" in native.SIGNATURES
    assert L.sb_set_render_embedding(None, None, None, 0, None, 0) == native.SB_ERR_INVALID_ARG
    assert b"sb_set_render_embedding" in L.sb_last_error()
    assert L.sb_group_set_render_embedding(None, None, None, 0, None, 0) == native.SB_ERR_INVALID_ARG
    assert b"sb_group_set_render_embedding" in L.sb_last_error()
    cage = np.zeros((1, 4), np.int32); w = np.zeros((1, 4), np.float32)
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    assert L.sb_set_render_embedding(None, cage.ctypes.data_as(ip), w.ctypes.data_as(fp), 1, None, 0) == native.SB_ERR_INVALID_ARG
    assert L.sb_group_set_render_embedding(None, cage.ctypes.data_as(ip), w.ctypes.data_as(fp), 1, None, 0) == native.SB_ERR_INVALID_ARG


def _cases(mesh):
    """(name, vertices float64) of the issue's three vertex sets on a tet mesh"""
    rng = np.random.default_rng(11)
    rest = mesh.rest_pos.astype(np.float64)
    tets = mesh.vol_ijkl.reshape(-1, 4)
    t = tets[rng.integers(0, tets.shape[0], 500)]
    lam = rng.dirichlet(np.ones(4), size=500)                     # a random convex combination of the tet's corners
    inside = np.einsum("rj,rjc->rc", lam, rest[t])
    # 50 surface points pushed outwards by 5 % of the bounding-box diagonal
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from embedding_bench import tet_boundary_faces
    faces = tet_boundary_faces(tets)
    f = faces[rng.integers(0, faces.shape[0], 50)]
    a, b, c = rest[f[:, 0]], rest[f[:, 1]], rest[f[:, 2]]
    nrm = np.cross(b - a, c - a)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    diag = float(np.linalg.norm(rest.max(0) - rest.min(0)))
    outside = (a + b + c) / 3.0 + 0.05 * diag * nrm
    return [("inside", inside), ("nodes", rest), ("outside", outside)], diag


def test_embed_vertices_on_the_tet_surrogate():
    mesh = bunny_surrogate(target_verts=2000, seed=7)
    cases, diag = _cases(mesh)
    rest = mesh.rest_pos
    tets = mesh.vol_ijkl.reshape(-1, 4)
    tet_rows = {tuple(sorted(r)) for r in tets.tolist()}
    for name, verts in cases:
        cage, w = embed_vertices(rest, tets, verts)
        m = verts.shape[0]
        assert cage.dtype == np.int32 and cage.shape == (m, 4) and w.dtype == np.float32 and w.shape == (m, 4), name
        assert cage.min() >= 0 and cage.max() < mesh.n and np.isfinite(w).all(), name
        assert all(tuple(sorted(r)) in tet_rows for r in cage[:64].tolist()), name          # a cage is a tet of the mesh
        assert np.abs(w.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-6, name
        err = np.abs(embedded_ref(rest, cage, w).astype(np.float64) - verts).max()
        assert err <= 1e-5 * diag, (name, err, diag)
        if name == "outside":
            assert (w.min(axis=1) < 0).all(), name
        else:
            assert w.min() >= -1e-6, (name, float(w.min()))


def test_the_float32_reference_agrees_with_float64():
    rng = np.random.default_rng(5)
    x = rng.uniform(-3, 3, size=(4000, 3)).astype(np.float32)
    cage = rng.integers(0, 4000, size=(3000, 4)).astype(np.int32)
    w = rng.uniform(-0.5, 1.5, size=(3000, 4)).astype(np.float32)
    w[:4] = [[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0], [0.25, 0.25, 0.25, 0.25]]
    got = embedded_ref(x, cage, w)
    assert got.dtype == np.float32 and got.shape == (3000, 3)
    want = embedded_ref64(x, cage, w)
    # relative to the size of the terms summed (a sum may cancel): 4 roundings of products + 3 of sums, each <= 2^-24 of a partial sum
    scale = np.einsum("rj,rjc->rc", np.abs(w.astype(np.float64)), np.abs(x[cage].astype(np.float64)))
    assert (np.abs(got - want) <= 1e-6 * np.maximum(scale, 1e-30)).all()
    assert np.array_equal(got[0], x[cage[0, 0]]) and np.array_equal(got[1], x[cage[1, 3]]) and not got[2].any()
