"""Host-side mirror of the Unity `Softbody : MonoBehaviour` component (csharp/Softbody.cs).

Same member names and call order as the C# component the north star asks for (BASELINE.json:5):
Start() -> sb_create + sb_set_* + sb_finalize, FixedUpdate() -> sb_step + sb_get_positions,
OnDestroy() -> sb_destroy. No reference component exists to copy (/root/reference/README.md:1 is
the whole reference tree). All compute happens in the HIP plugin; there is no CPU path here.
"""
import ctypes as C
import os

import numpy as np

from . import native
from .native import check, f32, i32, ptr


class Softbody:
    # [SerializeField] block of csharp/Softbody.cs
    def __init__(self, mesh, substeps=20, fixed_delta_time=0.02, gravity=(0.0, -9.81, 0.0), damping=0.0,
                 distance_compliance=0.0, volume_compliance=0.0, bending_compliance=0.0, device=0, rank=0, world=1,
                 part_dims=(0, 0, 0), tile_particles=0, use_graph=True, unique_id=None, ground_plane=None, use_gpu=True,
                 partition=native.SB_PARTITION_AUTO, plan_flags=None, halo_transport=None, halo_schedule=None, debug_flags=None, tuning=None):
        self.mesh = mesh
        self.substeps = int(substeps)
        self.fixed_delta_time = float(fixed_delta_time)
        self.gravity = tuple(float(g) for g in gravity)
        self.damping = float(damping)
        self.compliance = (float(distance_compliance), float(volume_compliance), float(bending_compliance))
        self.device, self.rank, self.world = int(device), int(rank), int(world)
        self.part_dims = tuple(int(d) for d in part_dims)
        self.tile_particles = int(tile_particles)
        self.use_graph = bool(use_graph)
        # sb_desc fields a host sets explicitly; None = taken from the harness' environment switches (native.*_from_env:
        # the plugin itself reads no environment variable that changes the plan, the transport or the schedule)
        self.partition = int(partition)
        self.plan_flags = native.plan_flags_from_env() if plan_flags is None else int(plan_flags)
        self.halo_transport = native.halo_transport_from_env() if halo_transport is None else int(halo_transport)
        self.halo_schedule = native.halo_schedule_from_env() if halo_schedule is None else int(halo_schedule)
        self.debug_flags = native.debug_flags_from_env() if debug_flags is None else int(debug_flags)
        self.unique_id = unique_id
        self.tuning = tuning               # native.SbTuning or None = from the harness' SB_* environment switches (A/B runs)
        self.ground_plane = ground_plane   # None or (nx, ny, nz, d): n.x >= d
        # use_gpu=False mirrors the C# component's CPU branch (csharp/Softbody.cs): no solver handle, no device; Start()
        # only fetches the schedule from the host-only planner. The CPU tick itself is C# (SoftbodyCpuSolver.cs); this
        # package has no CPU execution path, so FixedUpdate() refuses -- tests drive the oracle with cpu_schedule().
        self.use_gpu = bool(use_gpu)
        self._cpu_plan = None
        self._h = None
        self._render_set_only = False
        self._embedded = 0    # render vertices of the embedding in force (set_render_embedding), 0 = none
        self.vertices = None  # what the C# component assigns to mesh.vertices after each FixedUpdate

    # ---- MonoBehaviour surface ------------------------------------------------------------------
    def Start(self):
        L = native.lib()
        if not self.use_gpu:
            m = self.mesh
            rest = m.rest_pos if m.rest_pos is not None else m.pos
            self._cpu_plan = native.Plan.build(rest, m.dist_ij, m.vol_ijkl, m.bend_ijkl, rank=0, world=1,
                                               tile_particles=self.tile_particles, plan_flags=self.plan_flags)     # sb_plan_build: host only
            self.n = f32(m.pos, (-1, 3)).shape[0]
            self.vertices = f32(m.pos, (-1, 3)).copy()
            return self
        d = native.SbDesc()
        L.sb_desc_default(C.byref(d))
        d.device, d.rank, d.world = self.device, self.rank, self.world
        d.part_dims[:] = self.part_dims
        d.gravity[:] = self.gravity
        d.damping = self.damping
        d.tile_particles = self.tile_particles
        d.use_graph = 1 if self.use_graph else 0
        d.partition, d.plan_flags = self.partition, self.plan_flags
        d.halo_transport, d.halo_schedule, d.debug_flags = self.halo_transport, self.halo_schedule, self.debug_flags
        h = C.c_void_p()
        check(L.sb_create(C.byref(d), C.byref(h)))
        self._h = h
        try:
            tune = native.tuning_from_env() if self.tuning is None else self.tuning
            if tune is not None:      # A/B measurement switches (include/softbody_debug.h); a product host never calls this
                check(L.sb_set_tuning(h, C.byref(tune)))
            self._author(L, h)
        except Exception:
            self.OnDestroy()      # do not leak the handle when authoring / finalize fails
            raise
        return self

    def _author(self, L, h):
        m = self.mesh
        pos = f32(m.pos, (-1, 3)); vel = f32(m.vel, (-1, 3)); w = f32(m.inv_mass, (-1,))
        self.n = pos.shape[0]
        check(L.sb_set_particles(h, ptr(pos), ptr(vel), ptr(w), self.n))
        if m.rest_pos is not None:
            rest = f32(m.rest_pos, (-1, 3))
            check(L.sb_set_rest_positions(h, ptr(rest), self.n))
        if len(m.dist_rest):
            ij = i32(m.dist_ij, (-1, 2)); r = f32(m.dist_rest, (-1,))
            check(L.sb_set_distance_constraints(h, ptr(ij), ptr(r), r.shape[0], self.compliance[0]))
        if len(m.vol_rest):
            q = i32(m.vol_ijkl, (-1, 4)); r = f32(m.vol_rest, (-1,))
            check(L.sb_set_volume_constraints(h, ptr(q), ptr(r), r.shape[0], self.compliance[1]))
        if len(m.bend_rest):
            q = i32(m.bend_ijkl, (-1, 4)); r = f32(m.bend_rest, (-1, 2))
            check(L.sb_set_bending_constraints(h, ptr(q), ptr(r), r.shape[0], self.compliance[2]))
        peer_only = self.halo_transport == native.SB_TRANSPORT_PEER and self.unique_id is None    # the host connects the mailboxes itself
        if self.world > 1 and not (self.debug_flags & native.SB_DEBUG_NO_COMM) and not peer_only:
            assert self.unique_id is not None and len(self.unique_id) == native.SB_UNIQUE_ID_BYTES
            buf = (C.c_uint8 * native.SB_UNIQUE_ID_BYTES)(*self.unique_id)
            check(L.sb_comm_init(h, buf))
        if self.ground_plane is not None:
            check(L.sb_set_ground_plane(h, *[float(c) for c in self.ground_plane], 1))
        if getattr(m, "domain", None) is not None:      # sharded authoring: `m` is this rank's window of a larger mesh
            gid = i32(m.global_id, (-1,))
            check(L.sb_set_domain(h, C.byref(m.domain), ptr(gid), self.n))
        check(L.sb_finalize(h))
        self.vertices = pos.copy()

    def cpu_schedule(self):
        """use_gpu=False: the published order per substep parity, [(types, ids), (types, ids)] -- what the C# component
        hands to SoftbodyCpuSolver (sb_plan_get_order)."""
        if self._cpu_plan is None:
            raise RuntimeError("cpu_schedule() needs use_gpu=False and Start()")
        return [self._cpu_plan.order(parity) for parity in (0, 1)]

    def FixedUpdate(self, readback=True):
        if not self.use_gpu:
            raise RuntimeError("softbodyunity_amd has no CPU execution path: the CPU tick is csharp/SoftbodyCpuSolver.cs "
                               "(tests drive the oracle with cpu_schedule())")
        check(native.lib().sb_step(self._h, self.fixed_delta_time, self.substeps))
        if readback:
            self.get_positions(self.vertices)
        return self.vertices

    def OnDestroy(self):
        if self._cpu_plan is not None:
            self._cpu_plan.close()      # sb_plan_destroy
            self._cpu_plan = None
        if self._h is not None:
            native.lib().sb_destroy(self._h)
            self._h = None

    # ---- plumbing ---------------------------------------------------------------------------------
    def __enter__(self):
        return self.Start()

    def __exit__(self, *a):
        self.OnDestroy()

    def step(self, dt=None, substeps=None):
        check(native.lib().sb_step(self._h, self.fixed_delta_time if dt is None else dt,
                                   self.substeps if substeps is None else substeps))

    def synchronize(self):
        check(native.lib().sb_synchronize(self._h))

    # peer-store halo transport (SB_HALO_TRANSPORT=peer): the host carries the 64-byte mailbox handles between
    # the ranks with whatever channel it has (bench.py: a gloo all_gather) and connects every other rank's mailbox before the first tick
    def peer_mailbox_handle(self):
        out = np.zeros(native.SB_IPC_HANDLE_BYTES, np.uint8)
        check(native.lib().sb_peer_mailbox_handle(self._h, ptr(out)))
        return out

    def peer_connect(self, rank, handle):
        h = np.ascontiguousarray(handle, np.uint8)
        assert h.shape == (native.SB_IPC_HANDLE_BYTES,)
        check(native.lib().sb_peer_connect(self._h, int(rank), ptr(h), None))

    def get_positions(self, out=None):
        out = np.zeros((self.n, 3), np.float32) if out is None else out
        check(native.lib().sb_get_positions(self._h, ptr(out), self.n))
        return out

    def get_velocities(self, out=None):
        out = np.zeros((self.n, 3), np.float32) if out is None else out
        check(native.lib().sb_get_velocities(self._h, ptr(out), self.n))
        return out

    def readback_begin(self):
        check(native.lib().sb_readback_begin(self._h))

    def readback_end(self, normals=False, tangents=False, bounds=False):
        """-> (N,3) float32 view of the plugin's pinned snapshot (valid until the second readback_begin after it);
        with normals=True -> (positions, vertex normals) -- needs set_render_triangles (SPEC.md 6a). In render-set-only
        mode both arrays are compact, (count,3), entry k belonging to particle render_set()[k]. With an embedding set
        (set_render_embedding) both arrays are (m,3): the skinned render vertices and their normals, in the caller's vertex order.
        With tangents=True -> (positions, normals, tangents), tangents (rows,4) = xyz + handedness -- needs set_render_uvs (SPEC.md 6c).
        With bounds=True the tuple ends with (lo, hi), two float32 (3,) copies: the box of the delivered array -- needs set_readback_bounds
        before the readback_begin (SPEC.md 6d)."""
        p = C.POINTER(C.c_float)()
        check(native.lib().sb_readback_end(self._h, C.byref(p)))
        rows = self.n
        if self._embedded:
            rows = self._embedded
        elif self._render_set_only:
            rows = len(self.render_set())
        out = [np.ctypeslib.as_array(p, shape=(rows, 3))]
        if normals or tangents:
            q = C.POINTER(C.c_float)()
            check(native.lib().sb_readback_get_normals(self._h, C.byref(q)))
            out.append(np.ctypeslib.as_array(q, shape=(rows, 3)))
        if tangents:
            t = C.POINTER(C.c_float)()
            check(native.lib().sb_readback_get_tangents(self._h, C.byref(t)))
            out.append(np.ctypeslib.as_array(t, shape=(rows, 4)))
        if bounds:
            out.append(_box(native.lib().sb_readback_get_bounds, self._h))
        return out[0] if len(out) == 1 else tuple(out)

    def set_readback_bounds(self, on=True):
        """Readbacks begun from now on also bring the bounding box of what they deliver (readback_end(bounds=True), SPEC.md 6d)."""
        check(native.lib().sb_set_readback_bounds(self._h, 1 if on else 0))

    def get_bounds(self):
        """-> (lo, hi), float32 (3,): the box of the particles this rank owns, on what get_positions() would return now (SPEC.md 6d)."""
        return _box(native.lib().sb_get_bounds, self._h)

    def raycast(self, rays):
        """Rays against the deformed render mesh of the snapshot readback_end returned last (SPEC.md 6e). rays: (R, 8) float32 = origin xyz,
        t_max, direction xyz, 0 -- or (R, 7) without the last column. -> structured array (R,) with fields triangle (int32, -1 = no hit),
        t, u, v (float32): the nearest hit, t in units of the direction's length, (u, v) barycentric in the triangle's corners b and c."""
        return _raycast(native.lib().sb_readback_raycast, self._h, rays)

    def set_readback_render_set_only(self, on=True):
        """Readbacks bring only the particles the render triangles use (compact arrays)."""
        check(native.lib().sb_set_readback_render_set_only(self._h, 1 if on else 0))
        self._render_set_only = bool(on)

    def render_set(self):
        """Particle ids (ascending) of the compact readback entries; valid after a finished readback."""
        ids = C.POINTER(C.c_int32)(); cnt = C.c_int32()
        check(native.lib().sb_readback_get_render_set(self._h, C.byref(ids), C.byref(cnt)))
        return np.ctypeslib.as_array(ids, shape=(cnt.value,)) if cnt.value else np.zeros(0, np.int32)

    def set_render_triangles(self, tri):
        """Render triangles (M,3) particle indices: every later readback also brings area-weighted vertex normals."""
        tri = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
        check(native.lib().sb_set_render_triangles(self._h, tri.ctypes.data_as(C.POINTER(C.c_int32)), tri.shape[0]))

    def set_render_embedding(self, cage, weights, tri=None):
        """Embedded render vertices (SPEC.md 6b): vertex r = sum_j weights[r, j] * x[cage[r, j]] (mesh.embed_vertices makes both from a
        visual mesh). Every later readback brings the (m,3) skinned vertices instead of the particles, and -- with tri, (M,3) indices of
        RENDER VERTICES -- their normals. cage=None (or m = 0) switches the embedding off."""
        cage, weights, tri, m = _embedding_args(cage, weights, tri)
        check(native.lib().sb_set_render_embedding(self._h, _ip(cage), _fp(weights), m, _ip(tri), 0 if tri is None else tri.shape[0]))
        self._embedded = m

    def set_render_uvs(self, uv):
        """Render tangents (SPEC.md 6c): one (u, v) pair per vertex of the render mode in force -- per particle with set_render_triangles,
        per render vertex with set_render_embedding(..., tri). Every later readback also brings tangents (readback_end(tangents=True)).
        uv=None switches them off, as does every set_render_triangles / set_render_embedding."""
        uv, count = _uv_args(uv)
        check(native.lib().sb_set_render_uvs(self._h, _fp(uv), count))

    def set_kinematic_positions(self, ids, pos):
        """Move pinned particles (inverse mass 0) to new positions between two ticks (SPEC.md 2, attachments)."""
        ids = i32(ids); pos = f32(pos, (-1, 3))
        assert pos.shape[0] == ids.shape[0]
        check(native.lib().sb_set_kinematic_positions(self._h, ptr(ids), ptr(pos), int(ids.shape[0])))

    def set_state(self, pos, vel):
        pos = f32(pos, (-1, 3)); vel = f32(vel, (-1, 3))
        check(native.lib().sb_set_state(self._h, ptr(pos), ptr(vel), self.n))

    def apply_impulses(self, items):
        """Impulses between two ticks (SPEC.md 2c): items = an IMPULSE structured array, or a list of such arrays (impulse_particles,
        impulse_hits, impulse_explosion), applied in order. Velocities change, positions do not; the next step starts unfused."""
        _apply_impulses(native.lib().sb_apply_impulses, self._h, items)

    def owner(self):
        out = np.zeros(self.n, np.int32)
        check(native.lib().sb_get_owner(self._h, ptr(out), self.n))
        return out

    def validate(self, inject_fault=0):
        """Table validator (sb_debug_validate): a GPU kernel re-reads every table the tile kernels read -> report dict."""
        rep = native.SbValidateReport()
        check(native.lib().sb_debug_validate(self._h, int(inject_fault), C.byref(rep)))
        return {"tiles_checked": rep.tiles_checked, "groups_checked": rep.groups_checked, "constraints_checked": rep.constraints_checked,
                "errors": list(rep.errors), "first_stage": rep.first_stage, "first_tile": rep.first_tile, "first_group": rep.first_group,
                "first_kind": rep.first_kind}

    def stats(self):
        st = native.SbStats()
        check(native.lib().sb_get_stats(self._h, C.byref(st)))
        return st.as_dict()

    def plan(self):
        h = C.c_void_p()
        check(native.lib().sb_get_plan(self._h, C.byref(h)))
        p = native.Plan(h.value, False)
        p.n = self.n
        p.world = self.world
        return p

    def step_profiled(self, dt=None, substeps=None):
        """One eager tick with HIP events around every launch -> (ms per slot, launches per slot)."""
        k = self.stats()["n_global_colours"] + 5
        ms = np.zeros(k, np.float32); cnt = np.zeros(k, np.int32)
        check(native.lib().sb_step_profiled(self._h, self.fixed_delta_time if dt is None else dt,
                                            self.substeps if substeps is None else substeps, ptr(ms), ptr(cnt), k))
        return ms, cnt

    def profile_begin(self):
        check(native.lib().sb_profile_begin(self._h))

    def exchange_timing(self, enabled):
        """HIP events around every ghost exchange of the eager schedules (sb_debug_exchange_timing); read with exchange_timing_read()."""
        check(native.lib().sb_debug_exchange_timing(self._h, 1 if enabled else 0))

    def exchange_timing_read(self):
        t = native.SbExchangeTiming()
        check(native.lib().sb_debug_exchange_timing_read(self._h, C.byref(t)))
        return {"exchanges": t.exchanges, "pack_ms": t.pack_ms, "transport_ms": t.transport_ms, "total_ms": t.total_ms, "exposed_wait_ms": t.exposed_wait_ms}

    def profile_end(self):
        ms = C.c_float()
        check(native.lib().sb_profile_end(self._h, C.byref(ms)))
        return ms.value


def _embedding_args(cage, weights, tri):
    """-> (cage (m,4) int32, weights (m,4) float32, tri (M,3) int32 or None, m) as the C entry points take them"""
    if cage is None:
        return None, None, None, 0
    cage = np.ascontiguousarray(cage, dtype=np.int32).reshape(-1, 4)
    weights = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1, 4)
    assert cage.shape == weights.shape, "one row of four weights per row of four cage particles"
    if tri is not None:
        tri = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
    return cage, weights, tri, cage.shape[0]


def _box(fn, handle):
    """(lo, hi) of one of the *_get_bounds entry points"""
    lo = np.zeros(3, np.float32); hi = np.zeros(3, np.float32)
    check(fn(handle, _fp(lo), _fp(hi)))
    return lo, hi


RAY_HIT = np.dtype([("triangle", np.int32), ("t", np.float32), ("u", np.float32), ("v", np.float32)])


def _raycast(fn, handle, rays):
    """hits of one of the *_readback_raycast entry points"""
    rays = np.asarray(rays, dtype=np.float32)
    assert rays.ndim == 2 and rays.shape[1] in (7, 8), "rays: (R, 8) = origin xyz, t_max, direction xyz, 0 -- or (R, 7)"
    if rays.shape[1] == 7:
        rays = np.concatenate([rays, np.zeros((rays.shape[0], 1), np.float32)], axis=1)
    rays = np.ascontiguousarray(rays)
    hits = np.zeros(rays.shape[0], RAY_HIT)
    check(fn(handle, _fp(rays), rays.shape[0], hits.ctypes.data_as(C.POINTER(native.SbRayHit))))
    return hits


CLOSEST_HIT = np.dtype([("triangle", np.int32), ("distance", np.float32), ("u", np.float32), ("v", np.float32)])


def make_closest_queries(points, max_distance=np.inf):
    """-> (Q, 4) float32 = x, y, z, max_distance, as sb_group_readback_closest_points takes them (SPEC.md 6g): points (Q, 3) or (3,),
    max_distance a scalar or one per point, rounded to binary32 once."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    q = np.zeros((points.shape[0], 4), np.float32)
    q[:, 0:3] = points
    q[:, 3] = np.asarray(max_distance, np.float32)
    return q


# sb_impulse as a numpy record (48 bytes, the layout of native.SbImpulse)
IMPULSE = np.dtype([("kind", np.int32), ("flags", np.uint32), ("index", np.int32), ("u", np.float32), ("v", np.float32),
                    ("vec", np.float32, (3,)), ("radius", np.float32), ("strength", np.float32), ("reserved", np.int32, (2,))])


def impulse_particles(ids, vec, velocity_change=False):
    """PARTICLE items: impulse (or, with velocity_change, velocity change) vec -- (3,) for all, or (K, 3) -- on particles ids."""
    ids = np.atleast_1d(np.asarray(ids, np.int32))
    out = np.zeros(ids.shape[0], IMPULSE)
    out["kind"] = native.SB_IMPULSE_PARTICLE
    out["flags"] = native.SB_IMPULSE_VELOCITY_CHANGE if velocity_change else 0
    out["index"] = ids
    out["vec"] = np.asarray(vec, np.float32)
    return out


def impulse_hits(hits, vec, velocity_change=False):
    """SURFACE items from the structured array raycast() or closest_points() returns, misses included (they are skipped): vec -- (3,) or
    (R, 3) -- at every hit."""
    hits = np.atleast_1d(hits)
    out = np.zeros(hits.shape[0], IMPULSE)
    out["kind"] = native.SB_IMPULSE_SURFACE
    out["flags"] = native.SB_IMPULSE_VELOCITY_CHANGE if velocity_change else 0
    out["index"] = hits["triangle"]; out["u"] = hits["u"]; out["v"] = hits["v"]
    out["vec"] = np.asarray(vec, np.float32)
    return out


def impulse_explosion(centre, radius, strength, linear_falloff=False, velocity_change=False):
    """One RADIAL item (Unity's AddExplosionForce as an impulse); negative strength pulls inwards, radius may be inf."""
    out = np.zeros(1, IMPULSE)
    out["kind"] = native.SB_IMPULSE_RADIAL
    out["flags"] = (native.SB_IMPULSE_LINEAR_FALLOFF if linear_falloff else 0) | (native.SB_IMPULSE_VELOCITY_CHANGE if velocity_change else 0)
    out["vec"] = np.asarray(centre, np.float32)
    out["radius"] = radius; out["strength"] = strength
    return out


def _apply_impulses(fn, handle, items):
    """one of the *_apply_impulses entry points on an IMPULSE array or a list of them"""
    if isinstance(items, (list, tuple)):
        items = np.concatenate([np.atleast_1d(np.asarray(a, IMPULSE)) for a in items]) if len(items) else np.zeros(0, IMPULSE)
    items = np.ascontiguousarray(items, dtype=IMPULSE)
    check(fn(handle, items.ctypes.data_as(C.POINTER(native.SbImpulse)), int(items.shape[0])))


def make_surface_force(wind=(0, 0, 0), normal=0.0, tangential=0.0, pressure=0.0, dt=0.02):
    """-> native.SbSurfaceForce (SPEC.md 2e): the record of one apply_surface_forces call, every value rounded to binary32 once"""
    f = native.SbSurfaceForce()
    f.wind[:] = np.asarray(wind, np.float32).reshape(3).tolist()
    f.normal, f.tangential, f.pressure, f.dt = normal, tangential, pressure, dt
    return f


def placement_from_rotation(quat_xyzw, scale=1.0):
    """-> the (3, 3) float32 matrix SoftbodyGroup.place takes as m: the rotation of a quaternion (x, y, z, w) -- normalised here, computed in
    binary64 and rounded once -- times a uniform scale (rest lengths do not scale: a scaled body is squashed and recovers)."""
    q = np.asarray(quat_xyzw, np.float64).reshape(4)
    x, y, z, w = q / np.sqrt(np.dot(q, q))
    m = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float64)
    return (float(scale) * m).astype(np.float32)


def make_placement(m=None, frm=(0, 0, 0), to=(0, 0, 0), lin=None, ang=None, from_reference=False, keep_pinned=False):
    """-> native.SbPlacement (SPEC.md 2d): x' = m (src - frm) + to. lin / ang given: SB_PLACE_SET_VELOCITY (v' = lin + ang x (x' - to))."""
    p = native.SbPlacement()
    p.flags = ((native.SB_PLACE_FROM_REFERENCE if from_reference else 0) | (native.SB_PLACE_KEEP_PINNED if keep_pinned else 0)
               | (native.SB_PLACE_SET_VELOCITY if (lin is not None or ang is not None) else 0))
    p.m[:] = np.asarray(np.eye(3) if m is None else m, np.float32).reshape(9).tolist()
    p.frm[:] = np.asarray(frm, np.float32).reshape(3).tolist()
    p.to[:] = np.asarray(to, np.float32).reshape(3).tolist()
    p.lin[:] = np.asarray((0, 0, 0) if lin is None else lin, np.float32).reshape(3).tolist()
    p.ang[:] = np.asarray((0, 0, 0) if ang is None else ang, np.float32).reshape(3).tolist()
    return p


def _collider(shape, a, lin, ang, friction, restitution):
    c = native.SbCollider()
    c.shape = shape
    c.a[:] = np.asarray(a, np.float32).reshape(3).tolist()
    c.rot[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    c.lin[:] = np.asarray(lin, np.float32).reshape(3).tolist()
    c.ang[:] = np.asarray(ang, np.float32).reshape(3).tolist()
    c.friction, c.restitution = friction, restitution
    return c


def sphere_collider(centre, radius, lin=(0, 0, 0), ang=(0, 0, 0), friction=0.0, restitution=0.0):
    """-> native.SbCollider (SPEC.md 2f): a sphere about `centre` moving with `lin` and spinning with `ang` (radians per second) about it"""
    c = _collider(native.SB_COLLIDER_SPHERE, centre, lin, ang, friction, restitution)
    c.radius = radius
    return c


def capsule_collider(a, b, radius, lin=(0, 0, 0), ang=(0, 0, 0), friction=0.0, restitution=0.0):
    """-> native.SbCollider (SPEC.md 2f): every point within `radius` of the segment a b; `lin` is the velocity at a, `ang` turns about a"""
    c = _collider(native.SB_COLLIDER_CAPSULE, a, lin, ang, friction, restitution)
    c.b[:] = np.asarray(b, np.float32).reshape(3).tolist()
    c.radius = radius
    return c


def box_collider(centre, half, rot=None, lin=(0, 0, 0), ang=(0, 0, 0), friction=0.0, restitution=0.0):
    """-> native.SbCollider (SPEC.md 2f): a box about `centre` with half extents `half` along the ROWS of `rot` ((3, 3), orthonormal, not
    checked; None = the world axes). The rotation matrix R of a transform has the axes as columns: pass R.T."""
    c = _collider(native.SB_COLLIDER_BOX, centre, lin, ang, friction, restitution)
    c.half[:] = np.asarray(half, np.float32).reshape(3).tolist()
    if rot is not None:
        c.rot[:] = np.asarray(rot, np.float32).reshape(9).tolist()
    return c


def _uv_args(uv):
    """-> (uv (count,2) float32 or None, count) as sb_set_render_uvs takes them"""
    if uv is None:
        return None, 0
    uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
    return uv, uv.shape[0]


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def comm_unique_id():
    buf = (C.c_uint8 * native.SB_UNIQUE_ID_BYTES)()
    check(native.lib().sb_comm_unique_id(buf))
    return bytes(buf)


class SoftbodyGroup:
    """ONE process driving several devices behind one component (include/softbody_group.h; csharp/Softbody.cs with deviceCount > 1):
    the whole mesh authored once, one call per tick, state gathered in the caller's numbering. Same member names as Softbody."""

    def __init__(self, mesh, devices, substeps=20, fixed_delta_time=0.02, gravity=(0.0, -9.81, 0.0), damping=0.0,
                 distance_compliance=0.0, volume_compliance=0.0, bending_compliance=0.0, part_dims=(0, 0, 0), tile_particles=0,
                 use_graph=True, ground_plane=None, partition=native.SB_PARTITION_AUTO, plan_flags=None,
                 halo_transport=native.SB_TRANSPORT_RCCL, halo_schedule=native.SB_SCHEDULE_AUTO, debug_flags=0, walk=False, tuning=None, whole_mesh=False):
        self.mesh = mesh
        self.whole_mesh = bool(whole_mesh)
        self.devices = [int(d) for d in devices]
        self.substeps, self.fixed_delta_time = int(substeps), float(fixed_delta_time)
        self.gravity, self.damping = tuple(float(g) for g in gravity), float(damping)
        self.compliance = (float(distance_compliance), float(volume_compliance), float(bending_compliance))
        self.part_dims, self.tile_particles, self.use_graph = tuple(int(d) for d in part_dims), int(tile_particles), bool(use_graph)
        self.ground_plane = ground_plane
        self.partition = int(partition)
        self.plan_flags = native.plan_flags_from_env() if plan_flags is None else int(plan_flags)
        self.halo_transport, self.halo_schedule, self.debug_flags = int(halo_transport), int(halo_schedule), int(debug_flags)
        self.walk = bool(walk)
        self.tuning = tuning
        self._g = None
        self._render_set_only = False
        self._embedded = 0
        self.vertices = None

    def Start(self):
        L = native.lib()
        d = native.SbDesc()
        L.sb_desc_default(C.byref(d))
        d.part_dims[:] = self.part_dims
        d.gravity[:] = self.gravity
        d.damping, d.tile_particles, d.use_graph = self.damping, self.tile_particles, 1 if self.use_graph else 0
        d.partition, d.plan_flags = self.partition, self.plan_flags
        d.halo_transport, d.halo_schedule, d.debug_flags = self.halo_transport, self.halo_schedule, self.debug_flags
        devs = (C.c_int32 * len(self.devices))(*self.devices)
        g = C.c_void_p()
        check(L.sb_group_create(C.byref(d), devs, len(self.devices), (native.SB_GROUP_WALK if self.walk else 0) | (native.SB_GROUP_WHOLE_MESH if self.whole_mesh else 0), C.byref(g)))
        self._g = g
        try:
            tune = native.tuning_from_env() if self.tuning is None else self.tuning
            if tune is not None:
                for r in range(len(self.devices)):
                    check(L.sb_set_tuning(self._rank_handle(r), C.byref(tune)))
            m = self.mesh
            pos = f32(m.pos, (-1, 3)); vel = f32(m.vel, (-1, 3)); w = f32(m.inv_mass, (-1,))
            self.n = pos.shape[0]
            check(L.sb_group_set_particles(g, ptr(pos), ptr(vel), ptr(w), self.n))
            if m.rest_pos is not None:
                rest = f32(m.rest_pos, (-1, 3))
                check(L.sb_group_set_rest_positions(g, ptr(rest), self.n))
            if len(m.dist_rest):
                ij = i32(m.dist_ij, (-1, 2)); r = f32(m.dist_rest, (-1,))
                check(L.sb_group_set_distance_constraints(g, ptr(ij), ptr(r), r.shape[0], self.compliance[0]))
            if len(m.vol_rest):
                q = i32(m.vol_ijkl, (-1, 4)); r = f32(m.vol_rest, (-1,))
                check(L.sb_group_set_volume_constraints(g, ptr(q), ptr(r), r.shape[0], self.compliance[1]))
            if len(m.bend_rest):
                q = i32(m.bend_ijkl, (-1, 4)); r = f32(m.bend_rest, (-1, 2))
                check(L.sb_group_set_bending_constraints(g, ptr(q), ptr(r), r.shape[0], self.compliance[2]))
            if self.ground_plane is not None:
                check(L.sb_group_set_ground_plane(g, *[float(c) for c in self.ground_plane], 1))
            check(L.sb_group_finalize(g))
            self.vertices = pos.copy()
        except Exception:
            self.OnDestroy()
            raise
        return self

    def FixedUpdate(self, readback=True):
        check(native.lib().sb_group_step(self._g, self.fixed_delta_time, self.substeps))
        if readback:
            self.get_positions(self.vertices)
        return self.vertices

    def OnDestroy(self):
        if self._g is not None:
            native.lib().sb_group_destroy(self._g)
            self._g = None

    def __enter__(self):
        return self.Start()

    def __exit__(self, *a):
        self.OnDestroy()

    def step(self, dt=None, substeps=None):
        check(native.lib().sb_group_step(self._g, self.fixed_delta_time if dt is None else dt, self.substeps if substeps is None else substeps))

    def synchronize(self):
        check(native.lib().sb_group_synchronize(self._g))

    def get_positions(self, out=None):
        out = np.zeros((self.n, 3), np.float32) if out is None else out
        check(native.lib().sb_group_get_positions(self._g, ptr(out), self.n))
        return out

    def get_velocities(self, out=None):
        out = np.zeros((self.n, 3), np.float32) if out is None else out
        check(native.lib().sb_group_get_velocities(self._g, ptr(out), self.n))
        return out

    def set_state(self, pos, vel):
        pos = f32(pos, (-1, 3)); vel = f32(vel, (-1, 3))
        check(native.lib().sb_group_set_state(self._g, ptr(pos), ptr(vel), self.n))

    def set_kinematic_positions(self, ids, pos):
        ids = i32(ids); pos = f32(pos, (-1, 3))
        assert pos.shape[0] == ids.shape[0]
        check(native.lib().sb_group_set_kinematic_positions(self._g, ptr(ids), ptr(pos), int(ids.shape[0])))

    def apply_impulses(self, items):
        """Softbody.apply_impulses in the whole mesh's numbering; SURFACE items against the group's triangles / embedding."""
        _apply_impulses(native.lib().sb_group_apply_impulses, self._g, items)

    def apply_surface_forces(self, wind=(0, 0, 0), normal=0.0, tangential=0.0, pressure=0.0, dt=None):
        """Wind, air drag and pressure on the render triangles between two ticks (sb_group_apply_surface_forces, SPEC.md 2e): per triangle of
        area A and unit normal n the force A (normal (u.n) n + tangential (u - (u.n) n)) + pressure A n, u = wind - the triangle's velocity,
        acts for dt (None = the fixed delta time) and is shared in thirds by the corners. Velocities change, positions do not; the next step
        starts unfused. A group of one rank; more ranks and a render embedding are unsupported. A prepared native.SbSurfaceForce may be
        given as wind."""
        f = wind if isinstance(wind, native.SbSurfaceForce) else make_surface_force(wind, normal, tangential, pressure, self.fixed_delta_time if dt is None else dt)
        check(native.lib().sb_group_apply_surface_forces(self._g, C.byref(f)))

    def place(self, m=None, frm=(0, 0, 0), to=(0, 0, 0), lin=None, ang=None, from_reference=False, keep_pinned=False):
        """Move, rotate or respawn the whole body between two ticks, on the devices (sb_group_place, SPEC.md 2d): x' = m (src - frm) + to with
        src the positions, or the reference pose under from_reference (a respawn: undeformed). Velocities turn with m, or -- lin / ang given, and
        always under from_reference -- become lin + ang x (x' - to). Pinned particles move along unless keep_pinned. m: (3, 3), any finite
        matrix (placement_from_rotation builds one from a quaternion); None = identity. A prepared native.SbPlacement may be given as m."""
        p = m if isinstance(m, native.SbPlacement) else make_placement(m, frm, to, lin, ang, from_reference, keep_pinned)
        check(native.lib().sb_group_place(self._g, C.byref(p)))

    def collide(self, colliders):
        """Resolve contacts of every particle with a list of moving spheres, capsules and boxes between two ticks, on the devices
        (sb_group_collide, SPEC.md 2f): a penetrating particle is pushed to the surface and, when it approaches, takes the collider's
        velocity there with restitution along the normal and Coulomb friction across it. In list order; pinned particles and particles
        nothing touches keep every bit. colliders: native.SbCollider entries (sphere_collider, capsule_collider, box_collider); an empty
        list does nothing at all."""
        items = (native.SbCollider * max(1, len(colliders)))(*colliders)
        check(native.lib().sb_group_collide(self._g, items, len(colliders)))

    def collide_with_reactions(self, colliders):
        """collide(colliders), bit for bit, which also adds up on the devices what the body gives back to each collider
        (sb_group_collide_reactions, SPEC.md 2g); collider_reactions() fetches it. At most native.SB_COLLIDE_REACTIONS_MAX colliders."""
        items = (native.SbCollider * max(1, len(colliders)))(*colliders)
        check(native.lib().sb_group_collide_reactions(self._g, items, len(colliders)))

    REACTION_DTYPE = np.dtype([("impulse", np.float64, 3), ("angular_impulse", np.float64, 3), ("contact_mass", np.float64), ("n_contacts", np.int64)])

    def collider_reactions(self, capacity=native.SB_COLLIDE_REACTIONS_MAX):
        """The reactions of the last collide_with_reactions call (sb_group_get_collider_reactions): a structured array (REACTION_DTYPE), one
        record per collider in list order -- impulse and angular_impulse (about the collider's point a) in simulation space, the mass
        and the number of the particles it hit. Waits for that call alone; may be called again and returns the same bits. `capacity`
        cuts the answer short."""
        out = np.zeros(max(1, capacity), self.REACTION_DTYPE)
        count = C.c_int32(0)
        check(native.lib().sb_group_get_collider_reactions(self._g, out.ctypes.data_as(C.POINTER(native.SbColliderReaction)), capacity, C.byref(count)))
        return out[:min(count.value, capacity)]

    def set_heightfield(self, desc, heights):
        """Put a terrain height map on every rank's device (sb_group_set_heightfield, SPEC.md 2h): desc and heights as
        native.heightfield(a, cell, heights2d, rot, thickness) returns them. Copies; replaces a table set before; does not complete a
        held-back tick."""
        h = np.ascontiguousarray(heights, dtype=np.float32)
        if h.size != desc.nx * desc.nz:
            raise ValueError("heights must hold nx * nz samples")
        check(native.lib().sb_group_set_heightfield(self._g, C.byref(desc), h.ctypes.data_as(C.POINTER(C.c_float))))

    def clear_heightfield(self):
        """Clear the heightfield and release its device memory; collide_heightfield then does nothing."""
        check(native.lib().sb_group_set_heightfield(self._g, None, None))

    def collide_heightfield(self, friction=0.0, restitution=0.0):
        """Resolve the contacts of every particle with the heightfield set last, between two ticks, on the devices
        (sb_group_collide_heightfield, SPEC.md 2h): a particle under the surface, by less than the table's thickness along the normal, is
        pushed onto the triangle above it and, when it approaches, loses its normal velocity but for `restitution` and its tangential one
        by Coulomb `friction`. Everything else keeps every bit; with no heightfield set the call does nothing at all."""
        check(native.lib().sb_group_collide_heightfield(self._g, friction, restitution))

    def set_distance_field(self, slot, desc, samples):
        """Put a prop's signed-distance table into `slot` on every rank's device (sb_group_set_distance_field, SPEC.md 2i): desc and
        samples as native.distance_field(samples3d, cell, offset, thickness) returns them. Copies; replaces the slot's table; does not
        complete a held-back tick."""
        s = np.ascontiguousarray(samples, dtype=np.float32)
        if s.size != desc.nx * desc.ny * desc.nz:
            raise ValueError("samples must hold nx * ny * nz values")
        check(native.lib().sb_group_set_distance_field(self._g, slot, C.byref(desc), s.ctypes.data_as(C.POINTER(C.c_float))))

    def clear_distance_field(self, slot):
        """Clear `slot` and release its device memory; collide_distance_field on it then does nothing."""
        check(native.lib().sb_group_set_distance_field(self._g, slot, None, None))

    def collide_distance_field(self, slot, pose):
        """Resolve the contacts of every particle with the prop in `slot`, standing and moving as `pose` says
        (native.distance_field_pose), between two ticks, on the devices (sb_group_collide_distance_field, SPEC.md 2i): a particle under
        the contact surface phi = offset, by less than the table's thickness, is pushed onto it along the field's gradient and, when it
        approaches the moving prop, loses its normal velocity but for `restitution` and its tangential one by Coulomb `friction`.
        Everything else keeps every bit; with nothing set in the slot the call does nothing at all."""
        check(native.lib().sb_group_collide_distance_field(self._g, slot, C.byref(pose)))

    def set_render_triangles(self, tri):
        tri = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
        check(native.lib().sb_group_set_render_triangles(self._g, tri.ctypes.data_as(C.POINTER(C.c_int32)), tri.shape[0]))

    def set_render_embedding(self, cage, weights, tri=None):
        """Softbody.set_render_embedding on the gathered snapshot: cage indices in the whole mesh's numbering."""
        cage, weights, tri, m = _embedding_args(cage, weights, tri)
        check(native.lib().sb_group_set_render_embedding(self._g, _ip(cage), _fp(weights), m, _ip(tri), 0 if tri is None else tri.shape[0]))
        self._embedded = m

    def set_render_uvs(self, uv):
        """Softbody.set_render_uvs on the gathered snapshot: UVs per whole-mesh particle, or per render vertex of the embedding."""
        uv, count = _uv_args(uv)
        check(native.lib().sb_group_set_render_uvs(self._g, _fp(uv), count))

    def set_readback_render_set_only(self, on=True):
        check(native.lib().sb_group_set_readback_render_set_only(self._g, 1 if on else 0))
        self._render_set_only = bool(on)

    def readback_begin(self):
        check(native.lib().sb_group_readback_begin(self._g))

    def render_set(self):
        ids = C.POINTER(C.c_int32)(); cnt = C.c_int32()
        check(native.lib().sb_group_readback_get_render_set(self._g, C.byref(ids), C.byref(cnt)))
        return np.ctypeslib.as_array(ids, shape=(cnt.value,)) if cnt.value else np.zeros(0, np.int32)

    def readback_end(self, normals=False, tangents=False, bounds=False):
        p = C.POINTER(C.c_float)()
        check(native.lib().sb_group_readback_end(self._g, C.byref(p)))
        rows = self._embedded if self._embedded else (len(self.render_set()) if self._render_set_only else self.n)
        out = [np.ctypeslib.as_array(p, shape=(rows, 3))]
        if normals or tangents:
            q = C.POINTER(C.c_float)()
            check(native.lib().sb_group_readback_get_normals(self._g, C.byref(q)))
            out.append(np.ctypeslib.as_array(q, shape=(rows, 3)))
        if tangents:
            t = C.POINTER(C.c_float)()
            check(native.lib().sb_group_readback_get_tangents(self._g, C.byref(t)))
            out.append(np.ctypeslib.as_array(t, shape=(rows, 4)))
        if bounds:
            out.append(_box(native.lib().sb_group_readback_get_bounds, self._g))
        return out[0] if len(out) == 1 else tuple(out)

    def set_readback_bounds(self, on=True):
        """Softbody.set_readback_bounds on the array the group delivers."""
        check(native.lib().sb_group_set_readback_bounds(self._g, 1 if on else 0))

    def raycast(self, rays):
        """Softbody.raycast against the snapshot the group delivered last, on the render device."""
        return _raycast(native.lib().sb_group_readback_raycast, self._g, rays)

    def closest_points(self, points, max_distance=np.inf):
        """The nearest point of the deformed render mesh of the snapshot the group delivered last to each of points (SPEC.md 6g,
        sb_group_readback_closest_points). points: (Q, 3) with max_distance a scalar or (Q,) -- or (Q, 4) rows x, y, z, max_distance as
        make_closest_queries builds them. -> structured array (Q,) with fields triangle (int32, -1 = nothing within max_distance),
        distance, u, v (float32): (u, v) barycentric in the triangle's corners b and c, as raycast() gives them, so impulse_hits takes
        the array as it is."""
        q = np.asarray(points, dtype=np.float32)
        q = np.ascontiguousarray(q) if q.ndim == 2 and q.shape[1] == 4 else make_closest_queries(q, max_distance)
        hits = np.zeros(q.shape[0], CLOSEST_HIT)
        check(native.lib().sb_group_readback_closest_points(self._g, _fp(q), q.shape[0], hits.ctypes.data_as(C.POINTER(native.SbClosestHit))))
        return hits

    def get_bounds(self):
        """-> (lo, hi): every rank's box of what it owns, combined on the host."""
        return _box(native.lib().sb_group_get_bounds, self._g)

    def get_body_state(self, what=native.SB_BODY_POSE | native.SB_BODY_MOTION):
        """-> dict of sb_body_state's fields (SPEC.md 6f): mass centre, momenta, kinetic energy, best-fit rotation as a quaternion
        (x, y, z, w). what = SB_BODY_POSE (peeks: the tick stays fusable), SB_BODY_MOTION (completes the tick) or both."""
        st = native.SbBodyState()
        check(native.lib().sb_group_get_body_state(self._g, int(what), C.byref(st)))
        return st.as_dict()

    def _rank_handle(self, r):
        h = C.c_void_p()
        check(native.lib().sb_group_get_rank(self._g, int(r), C.byref(h)))
        return h

    def rank(self, r):
        """Borrowed Softbody view of rank r (inspection only: stats, owner, validate, plan)."""
        sb = Softbody.__new__(Softbody)
        sb._h = self._rank_handle(r)
        sb.world, sb.rank = len(self.devices), int(r)
        st = native.SbStats()
        check(native.lib().sb_get_stats(sb._h, C.byref(st)))
        sb.n = None       # (the rank's own numbering may be its window's: use stats / validate, which need no n)
        sb._cpu_plan = None
        return sb
