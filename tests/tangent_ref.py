"""Reference for render tangents (SPEC.md 6c): plain numpy float32, elementwise, in the spec's bracketing, sums accumulated one triangle
corner at a time in (t, j) order (np.add.at is unbuffered and sequential). numpy neither contracts a product and a sum into an FMA nor
flushes denormals, and its float32 division and square root are correctly rounded, so the GPU must reproduce this bit for bit from the same
vertex array and the same normals. A float64 twin of the whole chain (normals included) is what the float32 one is checked against."""
import numpy as np


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _coefficients(uv, tri, dtype):
    uv = np.ascontiguousarray(uv, dtype).reshape(-1, 2)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    du1 = uv[b, 0] - uv[a, 0]; dv1 = uv[b, 1] - uv[a, 1]
    du2 = uv[c, 0] - uv[a, 0]; dv2 = uv[c, 1] - uv[a, 1]
    with np.errstate(all="ignore"):
        p0 = du1 * dv2; p1 = du2 * dv1
        det = p0 - p1
        k = np.stack([dv2 / det, dv1 / det, du1 / det, du2 / det], axis=1)
    bad = (det == 0) | ~np.isfinite(k).all(axis=1)
    k[bad] = 0
    assert k.dtype == dtype
    return k


def tangent_coefficients(uv, tri):
    """(m,4) float32: (dv2, dv1, du1, du2) / det per triangle, zeros for a UV-degenerate one (det == 0 or a quotient not finite)."""
    return _coefficients(uv, tri, np.float32)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _frame_sums(p, tri, k):
    """S, T per vertex: s = k0*e1 - k1*e2 and q = k2*e2 - k3*e1 of every triangle added to its three corners, t ascending, j = 0, 1, 2"""
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    e1 = p[b] - p[a]; e2 = p[c] - p[a]
    s = k[:, 0:1] * e1 - k[:, 1:2] * e2
    q = k[:, 2:3] * e2 - k[:, 3:4] * e1
    S = np.zeros_like(p); T = np.zeros_like(p)
    flat = tri.reshape(-1)
    np.add.at(S, flat, np.repeat(s, 3, axis=0))
    np.add.at(T, flat, np.repeat(q, 3, axis=0))
    return S, T


def _per_vertex(n, S, T, guard):
    with np.errstate(all="ignore"):
        d = _dot(n, S)
        o = S - d[:, None] * n
        L2 = _dot(o, o)
        ok = L2 >= guard
        L = np.sqrt(np.where(ok, L2, 1).astype(S.dtype))
        o = np.where(ok[:, None], o / L[:, None], 0).astype(S.dtype)
        h = _dot(_cross(n, S), T)
    w = np.where(h < 0, -1, 1).astype(S.dtype)          # (a NaN gives +1)
    return np.concatenate([o, w[:, None]], axis=1)


def tangents_ref(p, normals, tri, uv):
    """(rows,4) float32 tangents (xyz, handedness) of SPEC.md 6c on the vertex array p with the normals of SPEC.md 6a on the same array."""
    p = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
    n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        S, T = _frame_sums(p, tri, tangent_coefficients(uv, tri))
    out = _per_vertex(n, S, T, np.float32(2.0 ** -96))
    assert out.dtype == np.float32 and S.dtype == np.float32
    return out


def tangents_ref64(p, tri, uv):
    """The same chain in float64, normals included -> (tangents (rows,4), normals (rows,3))"""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    f = _cross(p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]])
    n = np.zeros_like(p)
    np.add.at(n, tri.reshape(-1), np.repeat(f, 3, axis=0))
    L2 = _dot(n, n)
    ok = L2 >= 2.0 ** -96
    n = np.where(ok[:, None], n / np.sqrt(np.where(ok, L2, 1))[:, None], 0.0)
    with np.errstate(all="ignore"):
        S, T = _frame_sums(p, tri, _coefficients(uv, tri, np.float64))
    return _per_vertex(n, S, T, 2.0 ** -96), n


def lattice_uvs(n):
    """The fixed UVs of the n^3 lattice the tests use: v runs with iy, u with ix on one half and mirrored on the other (both handednesses)."""
    i = np.arange(n ** 3)
    ix, iy, iz = (i % n).astype(np.float64), ((i // n) % n).astype(np.float64), (i // (n * n)).astype(np.float64)
    v = (iy + 0.21 * iz + 0.13 * ix) / n
    u = np.where(ix < n // 2, (ix + 0.37 * iz) / n, (n - 1 - ix + 0.37 * iz) / n + 0.5)
    return np.stack([u, v], axis=1).astype(np.float32)
