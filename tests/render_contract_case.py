"""The render API's contract as a user meets it, walked through ctypes: every refusal of sb_readback_* / sb_set_render_* /
sb_set_readback_* (and their sb_group_* twins) with its status code and the whole sb_last_error text, and -- for a solver --
sb_stats.device_bytes after each step of a fixed sequence of render modes, as a delta from its value right after Start().
tests/golden/make_render_contract.py records what this walk gives into tests/golden/render_contract.json;
tests/test_gpu_render_contract.py walks it again and compares. Nothing here provokes a fault: every call is a clean refusal or a
normal readback.

A group runs in a process of its own (two ranks of one process on one device need a hardware queue per rank, which is set before
the process starts, as tests/test_gpu_group.py does).

usage: render_contract_case.py <solver|threads|walk>      prints `RENDER CONTRACT <json>` on one line
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from embedding_ref import lattice_cell_cages                                   # noqa: E402
from softbodyunity_amd import Softbody, SoftbodyGroup, bunny_surrogate, embed_vertices, jelly_cube, native       # noqa: E402

MARK = "RENDER CONTRACT "
_ip, _fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)


def ip(a):
    return None if a is None else a.ctypes.data_as(_ip)


def fp(a):
    return None if a is None else a.ctypes.data_as(_fp)


class Calls:
    """the walk's record: [label, status code, sb_last_error text ("" for SB_OK)] per call, in order"""

    def __init__(self, L, prefix, handle):
        self.L, self.prefix, self.h, self.rows = L, prefix, handle, []

    def __call__(self, label, name, *args, handle="own"):
        rc = getattr(self.L, self.prefix + name)(self.h if isinstance(handle, str) else handle, *args)
        self.rows.append([f"{name}: {label}", int(rc), self.L.sb_last_error().decode("utf-8", "replace") if rc else ""])
        return rc


def cube_case():
    """jelly_cube(8): surface triangles for the particle mode, cages from lattice cells for the embedding"""
    from readback_bench import surface_triangles
    n = 8
    mesh = jelly_cube(n)
    rng = np.random.default_rng(21)
    m = 60
    cage = lattice_cell_cages(n, rng.integers(0, n - 1, size=(m, 3)), rng)
    w = rng.uniform(-0.5, 1.5, size=(m, 4)).astype(np.float32)
    etri = rng.integers(0, m, size=(100, 3)).astype(np.int32)
    return mesh, np.ascontiguousarray(surface_triangles(n), dtype=np.int32), np.ascontiguousarray(cage, dtype=np.int32), w, etri


def tet_case():
    """the small tet body of tests/test_gpu_render_embedding.py: its boundary faces for the particle mode, the subdivided surface embedded"""
    from embedding_bench import subdivided_surface, tet_boundary_faces
    mesh = bunny_surrogate(target_verts=6000, seed=7)
    faces = tet_boundary_faces(mesh.vol_ijkl)
    verts, etri = subdivided_surface(mesh.rest_pos, faces)
    cage, w = embed_vertices(mesh.rest_pos, mesh.vol_ijkl, verts)
    return (mesh, np.ascontiguousarray(faces, dtype=np.int32), np.ascontiguousarray(cage, dtype=np.int32).reshape(-1, 4),
            np.ascontiguousarray(w, dtype=np.float32).reshape(-1, 4), np.ascontiguousarray(etri, dtype=np.int32))


def getters(call, label):
    q = _fp(); t = _fp(); ids = _ip(); cnt = C.c_int32()
    lo = (C.c_float * 3)(); hi = (C.c_float * 3)()
    call(label, "readback_get_normals", C.byref(q))
    call(label, "readback_get_tangents", C.byref(t))
    call(label, "readback_get_bounds", lo, hi)
    call(label, "readback_get_render_set", C.byref(ids), C.byref(cnt))


def walk_unauthored(L, prefix, handle):
    """a handle that was created and nothing more"""
    call = Calls(L, prefix, handle)
    tri = np.zeros((1, 3), np.int32); cage = np.zeros((1, 4), np.int32); w = np.full((1, 4), 0.25, np.float32); uv = np.zeros((1, 2), np.float32)
    p = _fp(); lo = (C.c_float * 3)(); hi = (C.c_float * 3)()
    call("before set_particles", "set_render_triangles", ip(tri), 1)
    call("before set_particles", "set_render_embedding", ip(cage), fp(w), 1, None, 0)
    call("no render mode, nothing authored", "set_render_uvs", fp(uv), 1)
    call("nothing authored", "set_readback_render_set_only", 1)
    call("before finalize", "readback_begin")
    call("without a begin, nothing authored", "readback_end", C.byref(p))
    call("before finalize", "get_bounds", lo, hi)
    getters(call, "nothing authored")
    return call.rows


def walk_null_arguments(call):
    tri = np.zeros((1, 3), np.int32); cage = np.zeros((1, 4), np.int32); w = np.full((1, 4), 0.25, np.float32); uv = np.zeros((1, 2), np.float32)
    p = _fp(); ids = _ip(); cnt = C.c_int32(); lo = (C.c_float * 3)(); hi = (C.c_float * 3)()
    call("null handle", "set_render_triangles", ip(tri), 1, handle=None)
    call("null handle", "set_render_embedding", ip(cage), fp(w), 1, None, 0, handle=None)
    call("null handle", "set_render_uvs", fp(uv), 1, handle=None)
    call("null handle", "set_readback_render_set_only", 1, handle=None)
    call("null handle", "set_readback_bounds", 1, handle=None)
    call("null handle", "readback_begin", handle=None)
    call("null handle", "readback_end", C.byref(p), handle=None)
    call("null out", "readback_end", None)
    call("null handle", "readback_get_normals", C.byref(p), handle=None)
    call("null out", "readback_get_normals", None)
    call("null handle", "readback_get_tangents", C.byref(p), handle=None)
    call("null out", "readback_get_tangents", None)
    call("null handle", "readback_get_bounds", lo, hi, handle=None)
    call("null lo", "readback_get_bounds", None, hi)
    call("null hi", "readback_get_bounds", lo, None)
    call("null handle", "readback_get_render_set", C.byref(ids), C.byref(cnt), handle=None)
    call("null ids", "readback_get_render_set", None, C.byref(cnt))
    call("null count", "readback_get_render_set", C.byref(ids), None)
    call("null handle", "get_bounds", lo, hi, handle=None)
    call("null lo", "get_bounds", None, hi)
    call("null hi", "get_bounds", lo, None)


def walk(L, prefix, handle, n, tri, cage, w, etri, step, device_bytes=None):
    """the fixed sequence on a finalized handle that has not stepped yet -> (calls, device_bytes deltas)"""
    call = Calls(L, prefix, handle)
    m = cage.shape[0]
    base = device_bytes() if device_bytes else 0
    deltas = []

    def mark(what):
        if device_bytes:
            deltas.append([what, int(device_bytes() - base)])

    def readback(label):
        p = _fp()
        call(label, "readback_begin")
        call(label, "readback_end", C.byref(p))

    def pending(label, with_uv_rows):
        uv = np.zeros((with_uv_rows, 2), np.float32)
        p = _fp()
        call(label, "readback_begin")
        call("while a readback is pending, " + label, "set_render_triangles", ip(tri), tri.shape[0])
        call("while a readback is pending, " + label, "set_render_embedding", ip(cage), fp(w), m, None, 0)
        call("while a readback is pending, " + label, "set_render_uvs", fp(uv), with_uv_rows)
        call("while a readback is pending, " + label, "set_render_uvs", None, 0)
        call("while a readback is pending, " + label, "set_readback_bounds", 1)
        call("while a readback is pending, " + label, "set_readback_render_set_only", 1)
        call("second, " + label, "readback_begin")
        call("two pending already, " + label, "readback_begin")
        call("first, " + label, "readback_end", C.byref(p))
        call("second, " + label, "readback_end", C.byref(p))
        call("without a begin, " + label, "readback_end", C.byref(p))

    step()
    walk_null_arguments(call)
    p = _fp()
    getters(call, "nothing finished")
    call("without a begin", "readback_end", C.byref(p))
    call("without triangles", "set_readback_render_set_only", 1)
    call("no render mode", "set_render_uvs", fp(np.zeros((n, 2), np.float32)), n)
    call("count 0, no render mode", "set_render_uvs", None, 0)
    # bad arguments of the two mode setters: refused, nothing changes
    call("null triangles, m = 1", "set_render_triangles", None, 1)
    call("m = -1", "set_render_triangles", ip(tri), -1)
    for bad in (n, -1):
        t2 = tri.copy(); t2[tri.shape[0] // 2, 1] = bad
        call(f"particle index {'n' if bad == n else bad}", "set_render_triangles", ip(t2), t2.shape[0])
    call("m_vertices = -1", "set_render_embedding", ip(cage), fp(w), -1, None, 0)
    call("m_tri = -1", "set_render_embedding", ip(cage), fp(w), m, ip(etri), -1)
    call("null cage", "set_render_embedding", None, fp(w), m, None, 0)
    call("null weights", "set_render_embedding", ip(cage), None, m, None, 0)
    call("null triangles, m_tri = 5", "set_render_embedding", ip(cage), fp(w), m, None, 5)
    for bad in (n, -1):
        c2 = cage.copy(); c2[m // 3, 3] = bad
        call(f"cage index {'n' if bad == n else bad}", "set_render_embedding", ip(c2), fp(w), m, None, 0)
    for bad in (np.nan, np.inf, -np.inf):
        w2 = w.copy(); w2[m // 2, 2] = bad
        call(f"weight {bad}", "set_render_embedding", ip(cage), fp(w2), m, None, 0)
    for bad in (m, -1):
        t2 = etri.copy(); t2[etri.shape[0] // 2, 1] = bad
        call(f"triangle index {'m' if bad == m else bad}", "set_render_embedding", ip(cage), fp(w), m, ip(t2), t2.shape[0])
    # 1. first full readback
    readback("1 first full readback")
    mark("1 first full readback")
    getters(call, "after a readback without a render mode")
    # 2. triangles
    call("2 on", "set_render_triangles", ip(tri), tri.shape[0])
    readback("2 with triangles")
    mark("2 set triangles, readback")
    getters(call, "after a readback with triangles")
    call("render triangles are set", "set_render_embedding", ip(cage), fp(w), m, None, 0)
    uv = np.linspace(0.0, 1.0, 2 * n, dtype=np.float32).reshape(n, 2)
    call("count mismatch (n - 1)", "set_render_uvs", fp(uv), n - 1)
    call("count -1", "set_render_uvs", fp(uv), -1)
    call("null with count n", "set_render_uvs", None, n)
    for bad in (np.nan, np.inf):
        u2 = uv.copy(); u2[n // 2, 1] = bad
        call(f"UV {bad}", "set_render_uvs", fp(u2), n)
    pending("particle mode", n)
    # 3. render set only
    call("3 on", "set_readback_render_set_only", 1)
    readback("3 render set only")
    mark("3 render set only, readback")
    getters(call, "after a render-set-only readback")
    # 4. UVs
    call("4 on", "set_render_uvs", fp(uv), n)
    readback("4 with UVs")
    mark("4 set UVs, readback")
    getters(call, "after a readback with UVs")
    # 5. bounds
    call("5 on", "set_readback_bounds", 1)
    readback("5 with bounds")
    mark("5 bounds on, readback")
    getters(call, "after a readback with bounds")
    # 6. triangles off
    call("6 off", "set_render_triangles", None, 0)
    mark("6 triangles off")
    getters(call, "after the triangles were switched off")
    call("no render mode any more", "set_render_uvs", fp(uv), n)
    call("without triangles any more", "set_readback_render_set_only", 1)
    # 7. embedding with triangles
    call("7 on, with triangles", "set_render_embedding", ip(cage), fp(w), m, ip(etri), etri.shape[0])
    readback("7 embedded")
    mark("7 embedding with triangles, readback")
    getters(call, "after an embedded readback")
    call("a render embedding is set", "set_render_triangles", ip(tri), tri.shape[0])
    call("a render embedding is set", "set_readback_render_set_only", 1)
    euv = np.linspace(0.0, 1.0, 2 * m, dtype=np.float32).reshape(m, 2)
    call("count mismatch (m + 1 given)", "set_render_uvs", fp(np.zeros((m + 1, 2), np.float32)), m + 1)
    e2 = euv.copy(); e2[m - 1, 0] = np.nan
    call("UV nan, last vertex", "set_render_uvs", fp(e2), m)
    pending("embedding", m)
    # 8. UVs over the render vertices
    call("8 on", "set_render_uvs", fp(euv), m)
    readback("8 embedded with UVs")
    mark("8 UVs, readback")
    getters(call, "after an embedded readback with UVs")
    # 9. embedding off
    call("9 off", "set_render_embedding", None, None, 0, None, 0)
    mark("9 embedding off")
    getters(call, "after the embedding was switched off")
    call("off already", "set_render_embedding", None, None, 0, None, 0)
    # an embedding without triangles carries no normals and takes no UVs; bounds off again
    call("on, no triangles", "set_render_embedding", ip(cage), fp(w), m, None, 0)
    readback("embedded, no triangles")
    getters(call, "after an embedded readback without triangles")
    call("embedding without triangles", "set_render_uvs", fp(euv), m)
    call("off", "set_render_embedding", None, None, 0, None, 0)
    call("off", "set_readback_bounds", 0)
    readback("last, full")
    mark("after the last full readback")
    getters(call, "after the last full readback")
    return call.rows, deltas


def _device_bytes(L, h):
    def read():
        st = native.SbStats()
        native.check(L.sb_get_stats(h, C.byref(st)))
        return st.device_bytes
    return read


def solver_contract():
    L = native.lib()
    out = {}
    d = native.SbDesc(); L.sb_desc_default(C.byref(d))
    h = C.c_void_p()
    native.check(L.sb_create(C.byref(d), C.byref(h)))
    try:
        out["unauthored"] = walk_unauthored(L, "sb_", h)
    finally:
        L.sb_destroy(h)
    for name, case, kw in (("cube8", cube_case, dict(substeps=4)),
                           ("tets", tet_case, dict(substeps=4, distance_compliance=1e-7, volume_compliance=1e-7, bending_compliance=1e-4))):
        mesh, tri, cage, w, etri = case()
        sb = Softbody(mesh, **kw).Start()
        try:
            calls, deltas = walk(L, "sb_", sb._h, mesh.n, tri, cage, w, etri, sb.step, _device_bytes(L, sb._h))
        finally:
            sb.OnDestroy()
        out[name] = {"calls": calls, "device_bytes": deltas}
    return out


def group_contract(host):
    L = native.lib()
    out = {}
    d = native.SbDesc(); L.sb_desc_default(C.byref(d))
    g = C.c_void_p()
    native.check(L.sb_group_create(C.byref(d), None, 1, 0, C.byref(g)))
    try:
        out["unauthored"] = walk_unauthored(L, "sb_group_", g)
    finally:
        L.sb_group_destroy(g)
    mesh, tri, cage, w, etri = cube_case()
    grp = SoftbodyGroup(mesh, [0, 0], substeps=4, tile_particles=64, halo_transport=native.SB_TRANSPORT_PEER, walk=host == "walk").Start()
    try:
        calls, _ = walk(L, "sb_group_", grp._g, mesh.n, tri, cage, w, etri, grp.step)
        out["cube8"] = {"calls": calls}
        # a rank of the partitioned solver refuses what needs its neighbours' particles
        ranks = []
        for r in range(2):
            call = Calls(L, "sb_", grp._rank_handle(r))
            q = _fp()
            call(f"rank {r}", "set_render_embedding", ip(cage), fp(w), cage.shape[0], None, 0)
            call(f"rank {r}", "readback_get_normals", C.byref(q))
            call(f"rank {r}", "set_render_uvs", fp(np.zeros((mesh.n, 2), np.float32)), mesh.n)
            call(f"rank {r}", "readback_get_tangents", C.byref(q))
            ranks += call.rows
        out["ranks"] = ranks
    finally:
        grp.OnDestroy()
    return out


def run_group(host):
    """group_contract(host) in a process of its own: a hardware queue per rank for the peer transport's waiting kernels"""
    import subprocess
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), host], env=env, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith(MARK)]
    assert out.returncode == 0 and len(lines) == 1, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads(lines[0][len(MARK):])


if __name__ == "__main__":
    what = sys.argv[1]
    res = solver_contract() if what == "solver" else group_contract(what)
    print(MARK + json.dumps(res), flush=True)
