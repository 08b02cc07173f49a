"""Frame sequences: every between-tick call of the group API interleaved with ticks, readbacks and queries, the way csharp/Softbody.cs drives
the plugin every FixedUpdate. A SCENARIO is a pure function of an integer seed: a body configuration and a SCRIPT, a list of steps
[name, args] with plain numbers, lists and strings as arguments, so that dumps(scenario) is enough to replay it (loads).

Two drivers walk the same script and return the same list of OBSERVATIONS (kind, label, payload):
  run_reference(oracle_mod, scenario)   on the CPU oracle's o.x, o.v, o.w with the tests/*_ref.py modules, each call applied at once, in call order
  run_group(group, scenario)            on a SoftbodyGroup (open_group builds it from the scenario)
mismatch(a, b) compares one observation of each under the rule of its kind: "bits" (uint32 views equal: positions, velocities, snapshot
arrays, boxes), "ray" / "closest" (same_hits), "body" (body_state_ref.check_sums, the counts exact), "react" (collider_reaction_ref.check,
a repeated fetch identical), "status" (the code of a refusal), "counters" (sb_stats ticks_fused, ticks_fused_kinematic, readback_peeks
after every step). No tolerance of its own.

What the reference takes from SPEC.md and include/softbody.h:
  2   a kinematic move takes effect at once as far as anything can tell: a position read shows it (softbody.h, sb_set_kinematic_positions:
      "position reads in between already show them") and every state write lands it first ("as every state write does")
  2c  impulses change velocities only, of particles with w > 0; SURFACE items go through the triangles of the render mode in force
  2d  placement maps every particle, pinned ones (and so the moved pins) included unless KEEP_PINNED
  2e  surface forces need render triangles, one rank and no embedding (SB_ERR_UNSUPPORTED otherwise)
  2f  colliders leave w = 0 alone (the moved pins too); 2g at most SB_COLLIDE_REACTIONS_MAX colliders; 2h the heightfield likewise
  2i  a signed-distance table lives in a slot with a lifetime of its own: set, replace and clear complete nothing, a call on a full slot
      completes the tick, a call on an empty slot does nothing at all (softbody_group.h: "the tick stays held back")
  6a-6d a snapshot is the state at ITS readback_begin; 6e, 6g queries answer for the snapshot ended last; 6f POSE reads positions only
The counters are predicted by TickModel, from begin_tick / flush_deferred / can_peek (csrc/schedule.hip) as softbody.h states them.

The fixed slice has two blocks. FIRST_BLOCK (seeds 0 .. 199) was written before the signed-distance volumes and stays byte for byte what
it was (tests/golden/frame_slice_v1.sha256.txt): its generator draws no distance-field step. SECOND_BLOCK (seeds 200 .. 279) and every
seed behind it use the extended generator, in which collide_distance_field is one more call that must complete the tick."""
import functools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import body_state_ref                        # noqa: E402
import bounds_ref                            # noqa: E402
import closest_ref                           # noqa: E402
import collider_reaction_ref                 # noqa: E402
import collider_ref                          # noqa: E402
import distance_field_cases                  # noqa: E402
import distance_field_ref                    # noqa: E402
import heightfield_cases                     # noqa: E402
import heightfield_ref                       # noqa: E402
import impulse_ref                           # noqa: E402
import placement_ref                         # noqa: E402
import raycast_ref                           # noqa: E402
import surface_force_ref                     # noqa: E402
import tangent_ref                           # noqa: E402
from embedding_ref import embedded_ref, lattice_cell_cages       # noqa: E402
from helpers import build_plan, make_oracle                      # noqa: E402

F = np.float32
SB_OK, SB_ERR_INVALID_ARG, SB_ERR_STATE, SB_ERR_UNSUPPORTED = 0, -1, -2, -7        # checked against native in constants_match()
POSE, MOTION = 1, 2
REACTIONS_MAX = 1024

BODIES = ("cube16", "cube10", "bunny", "cloth")
# the calls that must complete the tick (the pair matrix runs over these), under the names the coverage tables use
STATE_CHANGING = ("impulses", "impulse_surface", "place", "surface_forces", "collide", "collide_with_reactions", "collide_heightfield",
                  "set_state", "get_velocities", "body_motion")
LEFT_STATES = ("held back and peeked", "held back and unread", "completed by a velocity read", "held back with a kinematic move pending")
TICK_SHAPES = ("same", "other even S", "odd S", "other dt")
N_PAIRS = len(STATE_CHANGING) ** 2
N_PLANTED = len(STATE_CHANGING) * 4
N_RANDOM = 60
FIRST_BLOCK = tuple(range(N_PAIRS + N_PLANTED + N_RANDOM))
# the second block: the signed-distance calls (SPEC.md 2i) against everything above. D on a FULL slot must complete the tick.
D = "collide_distance_field"
ALL = STATE_CHANGING + (D,)
DF_SLOTS = 4
DF_PAIRS = tuple(p for X in STATE_CHANGING for p in ((D, X), (X, D))) + ((D, D),)
DF_LIFETIMES = ("a set between two ticks", "a replacement of equal size right behind a call", "a replacement of another size right behind a call",
                "a clear right behind a call, then a collide on the slot now empty", "a collide on an empty slot beside a full one",
                "one slot at two poses and a second slot behind colliders and terrain", "a snapshot pending across the call")
N2_PAIRS, N2_PLANTED, N2_LIFETIMES, N2_RANDOM = len(DF_PAIRS), 4, len(DF_LIFETIMES), 48
SECOND_BLOCK = tuple(range(len(FIRST_BLOCK), len(FIRST_BLOCK) + N2_PAIRS + N2_PLANTED + N2_LIFETIMES + N2_RANDOM))
FIXED_SLICE = FIRST_BLOCK + SECOND_BLOCK
CHUNK = 8                                    # scenarios per parametrised chunk: see tests/test_frame_sequences.py for the measured reference time


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def constants_match():
    from softbodyunity_amd import native
    return ((SB_OK, SB_ERR_INVALID_ARG, SB_ERR_STATE, SB_ERR_UNSUPPORTED, POSE, MOTION, REACTIONS_MAX) ==
            (native.SB_OK, native.SB_ERR_INVALID_ARG, native.SB_ERR_STATE, native.SB_ERR_UNSUPPORTED, native.SB_BODY_POSE, native.SB_BODY_MOTION,
             native.SB_COLLIDE_REACTIONS_MAX))


# ---- bodies ------------------------------------------------------------------------------------------------------------------------------------

def _surface_triangles_of_tets(mesh):
    """boundary faces of a tet mesh, as tests/test_gpu_peek.py takes them"""
    t = mesh.vol_ijkl.reshape(-1, 4)
    faces = np.concatenate([t[:, [0, 1, 2]], t[:, [0, 1, 3]], t[:, [0, 2, 3]], t[:, [1, 2, 3]]])
    key = np.sort(faces, axis=1)
    _, idx, cnt = np.unique(key, axis=0, return_index=True, return_counts=True)
    return faces[idx[cnt == 1]].astype(np.int32)


def _grid_cloth(a, b):
    xs, ys = np.meshgrid(np.arange(a), np.arange(b), indexing="ij")
    V = np.stack([xs.ravel(), np.zeros(a * b), ys.ravel()], axis=1).astype(np.float32)
    Fc = []
    for i in range(a - 1):
        for j in range(b - 1):
            p, q, r, s = i * b + j, (i + 1) * b + j, (i + 1) * b + j + 1, i * b + j + 1
            Fc += [(p, q, r), (p, r, s)]
    return V, np.array(Fc, np.int32)


@functools.lru_cache(maxsize=None)
def body(kind):
    """-> dict: mesh, pins, tri (render triangles over particles), uv, lattice (n or None), kw (SoftbodyGroup keywords), okw (make_oracle
    keywords), plan_kw (build_plan keywords), env (tuning variables in force while the group is built), S and dt of its usual tick.
    Built once and never written to."""
    from readback_bench import surface_triangles
    from softbodyunity_amd.mesh import bunny_surrogate, from_triangle_mesh, jelly_cube
    env, plan_kw, lattice = {}, {}, None
    if kind == "cube16":                     # the narrow launch with 8-byte previous-position codes (SB_NARROW_MIN_TILES=1)
        mesh = jelly_cube(16)
        top = mesh.pos[:, 1] > mesh.pos[:, 1].max() - 0.5
        mesh.inv_mass[top & (mesh.pos[:, 0] > mesh.pos[:, 0].max() - 0.5)] = 0.0      # one upper edge, for the kinematic moves
        tri, lattice = surface_triangles(16), 16
        kw = dict(damping=0.02); okw = dict(damping=0.02)
        env = {"SB_NARROW_MIN_TILES": "1"}
        S = 6
    elif kind == "cube10":                   # 64-particle tiles, a pinned top layer
        mesh = jelly_cube(10, pin_top=True)
        tri, lattice = surface_triangles(10), 10
        kw = dict(tile_particles=64); okw = {}; plan_kw = dict(tile_particles=64)
        S = 4
    elif kind == "bunny":                    # tets and hinges
        mesh = bunny_surrogate(target_verts=2000, seed=9)
        mesh.inv_mass[np.argsort(mesh.pos[:, 1])[-20:]] = 0.0
        tri = _surface_triangles_of_tets(mesh)
        kw = dict(distance_compliance=1e-7, volume_compliance=1e-7, bending_compliance=1e-4); okw = dict(compliance=(1e-7, 1e-7, 1e-4))
        S = 6
    else:                                    # a 24 x 24 cloth with hinges, held at its corners
        V, Fc = _grid_cloth(24, 24)
        mesh, pov = from_triangle_mesh(V, Fc)
        tri = np.ascontiguousarray(pov[Fc], dtype=np.int32)
        x, z = mesh.rest_pos[:, 0], mesh.rest_pos[:, 2]
        mesh.inv_mass[((x == x.min()) | (x == x.max())) & ((z == z.min()) | (z == z.max()))] = 0.0
        kw = dict(bending_compliance=1e-3, damping=0.02); okw = dict(compliance=(0.0, 0.0, 1e-3), damping=0.02)
        S = 4
    pins = np.nonzero(mesh.inv_mass == 0)[0].astype(np.int32)
    mesh.vel[pins] = 0.0
    rng = np.random.default_rng(1000 + BODIES.index(kind))
    uv = (tangent_ref.lattice_uvs(lattice) if lattice else rng.uniform(0, 1, size=(mesh.n, 2))).astype(np.float32)
    out = dict(kind=kind, mesh=mesh, pins=pins, tri=np.ascontiguousarray(tri, np.int32), used=np.unique(tri), uv=uv, lattice=lattice, kw=kw, okw=okw,
               plan_kw=plan_kw, env=env, S=S, dt=0.02, lo=mesh.pos.min(axis=0).astype(np.float64), hi=mesh.pos.max(axis=0).astype(np.float64),
               q=np.ascontiguousarray(mesh.pos if mesh.rest_pos is None else mesh.rest_pos, np.float32))
    if lattice:                              # the embedding of the lattice bodies (tests/embedding_ref.py lattice_cell_cages)
        m = 300
        out["cage"] = lattice_cell_cages(lattice, rng.integers(0, lattice - 1, size=(m, 3)), rng)
        out["w4"] = rng.uniform(-0.25, 1.25, size=(m, 4)).astype(np.float32)
        out["etri"] = rng.integers(0, m, size=(700, 3)).astype(np.int32)
        out["euv"] = rng.uniform(0, 1, size=(m, 2)).astype(np.float32)
    return out


# ---- the tick model: sb_stats counters from the rules in include/softbody.h ------------------------------------------------------------------

class TickModel:
    """The host-side state csrc/schedule.hip keeps between two ticks, and the three counters it moves.
      - a tick holds its last kernel back when the body is tiled and S is even (begin_tick: defer_last)
      - the next tick FUSES (ticks_fused) when one is held back, it defers its own last kernel too, S and dt are unchanged; pending
        kinematic targets then ride in the fused kernel (ticks_fused_kinematic)
      - a state-changing call completes the tick and lands pending targets (flush_deferred)
      - a position read PEEKS (readback_peeks) where can_peek holds -- peeking on (SB_PEEK_MIN_TILES=0 on these small bodies), a kernel held
        back, on T0 tiles -- and leaves everything as it is; elsewhere it completes the tick
      - a second kinematic move with one pending completes the tick first ("the earlier one takes effect first")
    Decision recorded here: the issue lists "set_kinematic_positions twice without a tick between" among the steps that leave the tick held
    back; softbody.h and sb_group_set_kinematic_positions say the earlier move takes effect first, which is a completed tick. The header
    wins, the model follows it, and softbody.h now says so in as many words."""

    def __init__(self, peeking, tiled=True):
        self.peeking, self.tiled = bool(peeking), bool(tiled)
        self.deferred, self.S, self.dt, self.kin = False, None, None, False
        self.slots = set()                   # the signed-distance slots that hold a table
        self.fused = self.kin_fused = self.peeks = 0

    def counters(self):
        return (self.fused, self.kin_fused, self.peeks)

    def complete(self):
        self.deferred = False
        self.kin = False

    def step(self, dt, S):
        defer_last = (not self.tiled) or S % 2 == 0
        fuse = self.deferred and defer_last and self.S == S and F(self.dt) == F(dt)
        if fuse:
            self.fused += 1
            if self.kin:
                self.kin_fused += 1
            self.kin = False
        else:
            self.complete()
        self.deferred, self.S, self.dt = defer_last, S, dt

    def read_positions(self):
        if self.peeking and self.deferred and ((not self.tiled) or self.S % 2 == 0):
            self.peeks += 1
        else:
            self.complete()

    def kinematic(self):
        if self.kin:
            self.complete()
        self.kin = True

    def nothing(self):
        pass

    # signed-distance slots (softbody_group.h): a table has a lifetime of its own -- a set, a replacement and a clear complete nothing;
    # a call completes the tick where the slot holds a table and "does nothing at all (the tick stays held back)" where it holds none
    def set_distance_field(self, slot):
        self.slots.add(slot)
        self.nothing()

    def clear_distance_field(self, slot):
        self.slots.discard(slot)
        self.nothing()

    def collide_distance_field(self, slot):
        if slot in self.slots:
            self.complete()
        else:
            self.nothing()


# ---- arguments -> the records both drivers use -----------------------------------------------------------------------------------------------

def _colliders(spec):
    out = []
    for c in spec:
        if c[0] == "sphere":
            _, a, radius, lin, ang, fr, re = c
            out.append(collider_ref.sphere(a, radius, lin, ang, fr, re))
        elif c[0] == "capsule":
            _, a, b, radius, lin, ang, fr, re = c
            out.append(collider_ref.capsule(a, b, radius, lin, ang, fr, re))
        else:
            _, a, half, quat, lin, ang, fr, re = c
            out.append(collider_ref.box(a, placement_ref.rotation(quat).T, half, lin, ang, fr, re))
    return out


def _heightfield(a):
    hf = heightfield_cases.ticking_field(a["lo"], a["hi"])
    hf["h"] = (hf["h"] * F(a["scale"]) + F(a["lift"])).astype(np.float32)
    return hf


def _distance_field(a):
    """-> (table, side): the prop of a set_distance_field step, a pure function of its arguments. "sphere": |p| - radius on n^3 samples
    (distance_field_cases.sampled_sphere); "floor": the plane field phi = y - y0 about the table's middle on 3^3 samples, with a thick band"""
    if a["prop"] == "sphere":
        return distance_field_cases.sampled_sphere(a["radius"], a["n"], thickness=a["thickness"])
    assert a["prop"] == "floor", a["prop"]
    side = float(a["side"])
    y = side / 2 * np.arange(3) - side / 2 - a["y0"]
    return distance_field_ref.make(np.broadcast_to(y[None, :, None], (3, 3, 3)), side / 2, 0.0, a["thickness"]), side


def _pose(a, side):
    """the pose of a collide_distance_field step for the table in its slot (any side where the slot is empty: nothing reads it)"""
    return distance_field_cases.pose_about(a["centre"], side, a["quat"], lin=a["lin"], ang=a["ang"], friction=a["friction"], restitution=a["restitution"])


def _placement(a):
    if a["mirror"] is not None:
        m = np.eye(3, dtype=np.float32); m[a["mirror"], a["mirror"]] = -1.0
    elif a["quat"] is not None:
        m = placement_ref.rotation(a["quat"])
    else:
        m = np.eye(3, dtype=np.float32)
    flags = ((placement_ref.FROM_REFERENCE if a["from_reference"] else 0) | (placement_ref.KEEP_PINNED if a["keep_pinned"] else 0) |
             (placement_ref.SET_VELOCITY if (a["lin"] is not None or a["ang"] is not None) else 0))
    z = (0.0, 0.0, 0.0)
    return dict(m=m, frm=a["frm"], to=a["to"], lin=z if a["lin"] is None else a["lin"], ang=z if a["ang"] is None else a["ang"], flags=flags)


def _state(b, a):
    rng = np.random.default_rng(a["seed"])
    mesh = b["mesh"]
    x = (mesh.pos + np.asarray(a["shift"], np.float32) + rng.uniform(-a["dx"], a["dx"], mesh.pos.shape).astype(np.float32)).astype(np.float32)
    v = rng.uniform(-a["dv"], a["dv"], mesh.pos.shape).astype(np.float32)
    v[b["pins"]] = 0.0
    return np.ascontiguousarray(x), np.ascontiguousarray(v)


def _impulse_items(b, spec, hits):
    from softbodyunity_amd.softbody import IMPULSE, impulse_explosion, impulse_hits, impulse_particles
    out = []
    for it in spec:
        if it[0] == "P":
            out.append(impulse_particles(it[1], it[2], velocity_change=bool(it[3])))
        elif it[0] == "R":
            out.append(impulse_explosion(it[1], it[2], it[3], linear_falloff=bool(it[4]), velocity_change=bool(it[5])))
        else:
            assert hits is not None, "a SURFACE item needs the hits of an earlier raycast or closest_points step of the script"
            out.append(impulse_hits(hits, it[1], velocity_change=bool(it[2])))
    return np.concatenate(out) if out else np.zeros(0, IMPULSE)


class PinTracker:
    """Where the pinned particles are, kept by BOTH drivers from the script alone (a placement maps them by tests/placement_ref.py's rule
    on their rows, set_state and a kinematic move put them): a kinematic step's targets are these positions plus the step's offset, the
    same arrays on either side, and nobody has to read the device to build them."""

    def __init__(self, b):
        self.b, self.pins = b, b["pins"]
        self.x = np.ascontiguousarray(b["mesh"].pos[self.pins], np.float32).copy()

    def place(self, P):
        if P["flags"] & placement_ref.KEEP_PINNED:
            return
        n = len(self.pins)
        placement_ref.apply(self.x, np.zeros((n, 3), np.float32), np.zeros(n, np.float32), self.b["q"][self.pins], **P)

    def set_state(self, x):
        self.x = np.ascontiguousarray(x[self.pins], np.float32).copy()

    def targets(self, a):
        sel = np.arange(len(self.pins))[::2] if a["half"] else np.arange(len(self.pins))
        t = (self.x[sel] + np.asarray(a["offset"], np.float32)).astype(np.float32)
        self.x[sel] = t
        return self.pins[sel].copy(), np.ascontiguousarray(t)


def _refusal_expected(sc, what, pending, world):
    """the status the reference gives a planted refusal, or None where it would accept the call"""
    if what == "surface_forces_embedding":
        return SB_ERR_UNSUPPORTED if (sc["mode"] == "embedding" or world > 1) else None
    if what == "surface_forces_ranks":
        return SB_ERR_UNSUPPORTED if world > 1 else None
    if what == "reactions_1025":
        return SB_ERR_INVALID_ARG
    if what == "third_snapshot":
        return SB_ERR_STATE if pending == 2 else None
    if what == "kinematic_free_particle":
        b = body(sc["body"])
        return SB_ERR_INVALID_ARG if b["mesh"].inv_mass[_free_particle(b)] != 0 else None
    if what == "step_dt_zero":
        return SB_ERR_INVALID_ARG
    if what in ("distance_field_slot_4", "distance_field_restitution"):
        return SB_ERR_INVALID_ARG
    raise ValueError(what)


def _free_particle(b):
    return int(np.nonzero(b["mesh"].inv_mass != 0)[0][0])


def coverage_name(name, a):
    """the name a step goes by in the coverage tables (STATE_CHANGING's for the calls that must complete the tick)"""
    if name == "apply_impulses":
        return "impulse_surface" if any(it[0] == "S" for it in a["items"]) else "impulses"
    if name == "get_body_state":
        return "body_motion" if a["what"] & MOTION else "body_pose"
    return {"apply_surface_forces": "surface_forces"}.get(name, name)


# ---- the reference driver ------------------------------------------------------------------------------------------------------------------------

def _render_arrays(b, sc, x):
    """what a snapshot of positions x delivers in the scenario's render mode: positions, normals, tangents or None, box; and (p, tri) for queries"""
    from oracle import oracle
    mode = sc["mode"]
    if mode == "embedding":
        p = embedded_ref(x, b["cage"], b["w4"])
        tri, uv, rows = b["etri"], b["euv"], slice(None)
    else:
        p, tri, uv = x, b["tri"], b["uv"]
        rows = b["used"] if mode == "render_set" else slice(None)
    nrm = oracle.vertex_normals(p, tri)
    tan = tangent_ref.tangents_ref(p, nrm, tri, uv)[rows] if sc["uvs"] else None
    pos = np.array(p[rows], np.float32, copy=True)       # (a snapshot: the oracle's arrays change in place)
    return dict(pos=pos, nrm=np.array(nrm[rows], np.float32, copy=True), tan=tan, box=bounds_ref.bounds_ref(pos), p=np.ascontiguousarray(p, np.float32).copy(), tri=tri)


def run_reference(oracle_mod, sc, world=1, info=None):
    """Walk the script on the oracle's state. -> observations. `info` (a dict) receives what the CPU module asserts about the scenario:
    hits per contact call, whether velocities changed per force call, the refusals met."""
    b = body(sc["body"])
    mesh = b["mesh"]
    o = make_oracle(oracle_mod, mesh, build_plan(mesh, **b["plan_kw"]), **b["okw"])
    model = TickModel(peeking=sc["peek0"])
    pins = PinTracker(b)
    obs = []
    pending, ended, hits, hf, react = [], None, None, None, None
    tables = {}                              # signed-distance slot -> (table, side)
    info = {} if info is None else info
    info.update(contact_hits=[], distance_field_hits=[], velocity_changed=[], refusals=[], call_left=[], call_shape=[])
    awaiting, last_tick, peeked, by_velocity_read = [], None, False, False
    tri_kw = dict(tri=b["etri"], cage=b["cage"], w4=b["w4"]) if sc["mode"] == "embedding" else dict(tri=b["tri"])

    for k, (name, a) in enumerate(sc["script"]):
        lab = f"step {k} {name}"
        cov = coverage_name(name, a)
        completes = cov in STATE_CHANGING or (cov == D and a["slot"] in tables)
        if completes:                        # what the call meets, and (once the next tick comes) what shape of tick it stands in front of
            left = (LEFT_STATES[3] if model.deferred and model.kin else LEFT_STATES[0] if model.deferred and peeked else LEFT_STATES[1] if model.deferred
                    else LEFT_STATES[2] if by_velocity_read else None)
            info["call_left"].append((cov, left))
            awaiting.append(cov)
        if name == "step":
            shape = None
            if last_tick is not None:
                shape = ("odd S" if a["S"] % 2 else "other dt" if a["dt"] != last_tick[0] and a["S"] == last_tick[1] else
                         "other even S" if a["S"] != last_tick[1] and a["dt"] == last_tick[0] else "same" if (a["dt"], a["S"]) == last_tick else None)
            info["call_shape"] += [(c, shape) for c in awaiting]
            awaiting, last_tick, peeked, by_velocity_read = [], (a["dt"], a["S"]), False, False
            o.step(a["dt"], a["S"]); model.step(a["dt"], a["S"])
        elif name == "apply_impulses":
            before = o.v.copy()
            impulse_ref.apply(o.x, o.v, o.w, _impulse_items(b, a["items"], hits), **tri_kw)
            info["velocity_changed"].append(not np.array_equal(bits(before), bits(o.v)))
            model.complete()
        elif name == "place":
            P = _placement(a)
            placement_ref.apply(o.x, o.v, o.w, b["q"], **P); pins.place(P)
            model.complete()
        elif name == "apply_surface_forces":
            before = o.v.copy()
            surface_force_ref.apply(o.x, o.v, o.w, b["tri"], wind=a["wind"], normal=a["normal"], tangential=a["tangential"], pressure=a["pressure"], dt=a["dt"])
            info["velocity_changed"].append(not np.array_equal(bits(before), bits(o.v)))
            model.complete()
        elif name == "collide":
            h = collider_ref.apply(o.x, o.v, o.w, _colliders(a["colliders"]))
            info["contact_hits"].append(int(h.sum()))
            model.complete()
        elif name == "collide_with_reactions":
            own = None
            h, react = collider_reaction_ref.apply(o.x, o.v, o.w, _colliders(a["colliders"]), own)
            info["contact_hits"].append(int(h.sum()))
            model.complete()
        elif name == "collide_heightfield":
            if hf is not None:
                h = heightfield_ref.apply(o.x, o.v, o.w, hf, a["friction"], a["restitution"])
                info["contact_hits"].append(int(h.sum()))
                model.complete()               # (with no table set the call does nothing at all: softbody_group.h)
        elif name == "set_heightfield":
            hf = _heightfield(a)
        elif name == "clear_heightfield":
            hf = None
        elif name == "set_distance_field":
            tables[a["slot"]] = _distance_field(a)
            model.set_distance_field(a["slot"])
        elif name == "clear_distance_field":
            tables.pop(a["slot"], None)
            model.clear_distance_field(a["slot"])
        elif name == "collide_distance_field":
            if a["slot"] in tables:          # (on an empty slot the call does nothing at all: softbody_group.h)
                df, side = tables[a["slot"]]
                h = distance_field_ref.apply(o.x, o.v, o.w, df, _pose(a, side))
                info["contact_hits"].append(int(h.sum())); info["distance_field_hits"].append(int(h.sum()))
            model.collide_distance_field(a["slot"])
        elif name == "set_state":
            x, v = _state(b, a)
            o.x[:] = x; o.v[:] = v; pins.set_state(x)
            model.complete()
        elif name == "get_velocities":
            model.complete()
            obs.append(("bits", lab, o.v.copy()))
        elif name == "get_positions":
            model.read_positions()
            obs.append(("bits", lab, o.x.copy()))
        elif name == "get_bounds":
            model.read_positions()
            obs.append(("bits", lab, np.concatenate(bounds_ref.bounds_ref(o.x))))
        elif name == "get_body_state":
            if a["what"] & MOTION:
                model.complete()
            model.read_positions()           # (behind a completed tick this completes nothing, and lands pending targets as every read does)
            obs.append(("body", lab, (a["what"], body_state_ref.sums_ref(o.x, o.v, o.w, b["q"], a["what"]))))
        elif name == "set_kinematic_positions":
            ids, t = pins.targets(a)
            o.set_kinematic_positions(ids, t)
            model.kinematic()
        elif name == "readback_begin":
            assert len(pending) < 2
            model.read_positions()
            pending.append(_render_arrays(b, sc, o.x))
        elif name == "readback_end":
            ended = pending.pop(0)
            obs.append(("bits", lab + " positions", ended["pos"]))
            obs.append(("bits", lab + " normals", ended["nrm"]))
            if ended["tan"] is not None:
                obs.append(("bits", lab + " tangents", ended["tan"]))
            obs.append(("bits", lab + " box", np.concatenate(ended["box"])))
        elif name == "raycast":
            hits = raycast_ref.raycast_ref(ended["p"], ended["tri"], np.asarray(a["rays"], np.float32))
            obs.append(("ray", lab, hits))
        elif name == "closest_points":
            hits = closest_ref.closest_ref(ended["p"], ended["tri"], np.asarray(a["queries"], np.float32))
            obs.append(("closest", lab, hits))
        elif name == "collider_reactions":
            obs.append(("react", lab, react))
        elif name == "refuse":
            want = _refusal_expected(sc, a["what"], len(pending), world)
            info["refusals"].append((a["what"], want))
            obs.append(("status", lab + " " + a["what"], want))
        else:
            raise ValueError(f"unknown step {name}")
        if name in ("get_positions", "get_bounds", "readback_begin") or (name == "get_body_state" and a["what"] == POSE):
            peeked = model.deferred
        by_velocity_read = (name == "get_velocities") or (by_velocity_read and not model.deferred and not completes)
        obs.append(("counters", lab, model.counters()))
    info["final"] = (o.x.copy(), o.v.copy())
    return obs


# ---- the group driver ----------------------------------------------------------------------------------------------------------------------------

def open_group(sc, devices=(0,), **extra):
    """The SoftbodyGroup of a scenario, started, its render mode set. The tuning variables of the body and the scenario hold while it is
    built (native.tuning_from_env is read in Start) and are put back afterwards."""
    from softbodyunity_amd import SoftbodyGroup
    b = body(sc["body"])
    env = dict(b["env"])
    env["SB_PEEK_MIN_TILES"] = "0" if sc["peek0"] else None
    for k in ("SB_NO_PEEK", "SB_NO_LAZY_TICK", "SB_NO_KIN_FUSE", "SB_NO_LANE_PACK", "SB_TILE_LANES", "SB_NO_WIDE_SLOTS"):
        env.setdefault(k, None)
    env.setdefault("SB_NARROW_MIN_TILES", None)
    saved = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        g = SoftbodyGroup(b["mesh"], list(devices), substeps=b["S"], fixed_delta_time=b["dt"], use_graph=sc["graph"], **b["kw"], **extra).Start()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        g.set_readback_bounds(True)
        if sc["mode"] == "embedding":
            g.set_render_embedding(b["cage"], b["w4"], b["etri"])
        else:
            g.set_render_triangles(b["tri"])
            if sc["mode"] == "render_set":
                g.set_readback_render_set_only(True)
        if sc["uvs"]:
            g.set_render_uvs(b["euv"] if sc["mode"] == "embedding" else b["uv"])
    except Exception:
        g.OnDestroy()
        raise
    return g


def coded_format_in_force(g):
    """tests/test_gpu_heightfield.py's check that the narrow launch hands previous positions on as 8-byte codes"""
    st = g.rank(0).stats()
    lb, n = st["launch_bytes"], st["n_particles_local"]
    return lb[2] - lb[0] == 4 * n and lb[3] - lb[0] == 4 * n


def _status(fn):
    from softbodyunity_amd import native
    try:
        fn()
    except native.SoftbodyError as e:
        return e.code
    return SB_OK


def group_counters(g):
    """ticks_fused, ticks_fused_kinematic, readback_peeks. One rank: its own. Several: ticks_fused must agree on every rank (they decide
    alike), the kinematic count is the largest (a rank that owns no target carries none along), the peeks are rank 0's business only in
    the one-rank test."""
    W = len(g.devices)
    st = [g.rank(r).stats() for r in range(W)]
    if W == 1:
        return (st[0]["ticks_fused"], st[0]["ticks_fused_kinematic"], st[0]["readback_peeks"])
    fused = {s["ticks_fused"] for s in st}
    return (fused.pop() if len(fused) == 1 else tuple(s["ticks_fused"] for s in st), max(s["ticks_fused_kinematic"] for s in st), None)


def run_group(g, sc, upto=None):
    """Walk the script on a SoftbodyGroup (open_group(sc)). -> observations, in run_reference's order."""
    from softbodyunity_amd import native
    b = body(sc["body"])
    pins = PinTracker(b)
    obs = []
    hits, n_pending = None, 0
    sides = {}                               # signed-distance slot -> the side of its table (the pose is built from it)
    W = len(g.devices)
    for k, (name, a) in enumerate(sc["script"][:upto]):
        lab = f"step {k} {name}"
        if name == "step":
            g.step(a["dt"], a["S"])
        elif name == "apply_impulses":
            g.apply_impulses(_impulse_items(b, a["items"], hits))
        elif name == "place":
            P = _placement(a)
            p = native.SbPlacement()
            p.flags = P["flags"]
            p.m[:] = np.asarray(P["m"], np.float32).reshape(9).tolist()
            for field in ("frm", "to", "lin", "ang"):
                getattr(p, field)[:] = np.asarray(P[field], np.float32).reshape(3).tolist()
            g.place(p); pins.place(P)
        elif name == "apply_surface_forces":
            g.apply_surface_forces(a["wind"], a["normal"], a["tangential"], a["pressure"], a["dt"])
        elif name == "collide":
            g.collide([collider_ref.to_native(c) for c in _colliders(a["colliders"])])
        elif name == "collide_with_reactions":
            g.collide_with_reactions([collider_ref.to_native(c) for c in _colliders(a["colliders"])])
        elif name == "collide_heightfield":
            g.collide_heightfield(a["friction"], a["restitution"])
        elif name == "set_heightfield":
            g.set_heightfield(*heightfield_ref.to_native(_heightfield(a)))
        elif name == "clear_heightfield":
            g.clear_heightfield()
        elif name == "set_distance_field":
            df, sides[a["slot"]] = _distance_field(a)
            g.set_distance_field(a["slot"], *distance_field_ref.to_native(df))
        elif name == "clear_distance_field":
            g.clear_distance_field(a["slot"]); sides.pop(a["slot"], None)
        elif name == "collide_distance_field":
            g.collide_distance_field(a["slot"], distance_field_ref.pose_to_native(_pose(a, sides.get(a["slot"], 1.0))))
        elif name == "set_state":
            x, v = _state(b, a)
            g.set_state(x, v); pins.set_state(x)
        elif name == "get_velocities":
            obs.append(("bits", lab, g.get_velocities().copy()))
        elif name == "get_positions":
            obs.append(("bits", lab, g.get_positions().copy()))
        elif name == "get_bounds":
            obs.append(("bits", lab, np.concatenate(g.get_bounds())))
        elif name == "get_body_state":
            obs.append(("body", lab, (a["what"], g.get_body_state(a["what"]))))
        elif name == "set_kinematic_positions":
            g.set_kinematic_positions(*pins.targets(a))
        elif name == "readback_begin":
            g.readback_begin(); n_pending += 1
        elif name == "readback_end":
            got = g.readback_end(normals=True, tangents=sc["uvs"], bounds=True)
            n_pending -= 1
            obs.append(("bits", lab + " positions", np.array(got[0], copy=True)))
            obs.append(("bits", lab + " normals", np.array(got[1], copy=True)))
            if sc["uvs"]:
                obs.append(("bits", lab + " tangents", np.array(got[2], copy=True)))
            obs.append(("bits", lab + " box", np.concatenate(got[-1])))
        elif name == "raycast":
            hits = g.raycast(np.asarray(a["rays"], np.float32)).copy()
            obs.append(("ray", lab, hits))
        elif name == "closest_points":
            hits = g.closest_points(np.asarray(a["queries"], np.float32)).copy()
            obs.append(("closest", lab, hits))
        elif name == "collider_reactions":
            first = g.collider_reactions().copy()
            obs.append(("react", lab, (first, g.collider_reactions().copy() if a["twice"] else None)))
        elif name == "refuse":
            what = a["what"]
            if what in ("surface_forces_embedding", "surface_forces_ranks"):
                rc = _status(lambda: g.apply_surface_forces((1.0, 0.0, 0.0), 0.5, 0.1, 0.0, 0.02))
            elif what == "reactions_1025":
                one = collider_ref.to_native(collider_ref.sphere((0, -1e6, 0), 0.5))
                rc = _status(lambda: g.collide_with_reactions([one] * (REACTIONS_MAX + 1)))
            elif what == "third_snapshot":
                rc = _status(g.readback_begin)
                n_pending += rc == SB_OK
            elif what == "kinematic_free_particle":
                rc = _status(lambda: g.set_kinematic_positions(np.array([_free_particle(b)], np.int32), np.zeros((1, 3), np.float32)))
            elif what == "step_dt_zero":
                rc = _status(lambda: g.step(0.0, 4))
            elif what == "distance_field_slot_4":
                rc = _status(lambda: g.collide_distance_field(DF_SLOTS, distance_field_ref.pose_to_native(_pose(a["pose"], 1.0))))
            elif what == "distance_field_restitution":      # on a full slot: refused before the table is looked at
                assert a["slot"] in sides and a["pose"]["restitution"] == 1.5
                rc = _status(lambda: g.collide_distance_field(a["slot"], distance_field_ref.pose_to_native(_pose(a["pose"], sides[a["slot"]]))))
            else:
                raise ValueError(what)
            obs.append(("status", lab + " " + what, rc))
        else:
            raise ValueError(f"unknown step {name}")
        obs.append(("counters", lab, group_counters(g)))
    return obs


# ---- the rules -----------------------------------------------------------------------------------------------------------------------------------

def mismatch(want, got, world=1):
    """-> None, or what is wrong with `got` (run_group's observation) against `want` (run_reference's), under the rule of its kind"""
    kind, lab, w = want
    kind2, lab2, g = got
    if kind != kind2 or lab != lab2:
        return f"the drivers disagree about the observation itself: {kind} '{lab}' and {kind2} '{lab2}'"
    if kind == "bits":
        if np.shape(g) != np.shape(w):
            return f"shape {np.shape(g)} for {np.shape(w)}"
        bad = bits(g) != bits(w)
        return None if not bad.any() else f"{int(bad.sum())} of {bad.size} words differ, the first at {tuple(int(i) for i in np.argwhere(bad)[0])}"
    if kind == "ray":
        return None if raycast_ref.same_hits(g, w) else "the hits differ"
    if kind == "closest":
        return None if closest_ref.same_hits(g, w) else "the hits differ"
    if kind == "body":
        what, ref = w
        st = g[1]
        why = body_state_ref.check_sums(st["sums"], ref, what)
        if (st["n_dynamic"], st["n_pinned"]) != (ref["n_dynamic"], ref["n_pinned"]):
            why.append(f"counts {(st['n_dynamic'], st['n_pinned'])} for {(ref['n_dynamic'], ref['n_pinned'])}")
        return "; ".join(why) or None
    if kind == "react":
        first, second = g
        if len(first) != len(w):
            return f"{len(first)} records for {len(w)}"
        why = [f"collider {k}: {t}" for k, (rec, ref) in enumerate(zip(first, w)) for t in collider_reaction_ref.check(rec, ref)]
        if second is not None and first.tobytes() != second.tobytes():
            why.append("the repeated fetch returned other bits")
        return "; ".join(why) or None
    if kind == "status":
        return None if w == g else f"status {g} for {w}"
    if kind == "counters":
        names = ("ticks_fused", "ticks_fused_kinematic", "readback_peeks")
        why = [f"{names[i]} {g[i]} for {w[i]}" for i in range(3) if g[i] is not None and g[i] != w[i]]
        return "; ".join(why) or None
    raise ValueError(kind)


def first_mismatch(want, got):
    """-> None, or (index, explanation) of the first differing observation"""
    for i, (w, g) in enumerate(zip(want, got)):
        why = mismatch(w, g)
        if why:
            return i, why
    if len(want) != len(got):
        return min(len(want), len(got)), f"{len(got)} observations for {len(want)}"
    return None


def dumps(sc):
    """a scenario as text that loads() turns back into the same scenario: one line of configuration, one line per step"""
    head = {k: v for k, v in sc.items() if k != "script"}
    return "\n".join([json.dumps(head)] + [json.dumps(step) for step in sc["script"]])


def loads(text):
    lines = [ln for ln in text.splitlines() if ln.strip()]
    sc = json.loads(lines[0])
    sc["script"] = [json.loads(ln) for ln in lines[1:]]
    return sc


def report(sc, want, got, index, why, command):
    """the failure text: the seed, the first differing observation, the step that produced it, the script up to there, the command to replay"""
    lab = want[index][1] if index < len(want) else got[index][1]
    k = int(lab.split()[1])
    head = dict(sc); head["script"] = sc["script"][:k + 1]
    return (f"seed {sc['seed']}: observation {index} ({want[index][0] if index < len(want) else '?'}, '{lab}') differs: {why}\n"
            f"the script up to that step:\n{dumps(head)}\nreplay: {command}")


# ---- the generator -------------------------------------------------------------------------------------------------------------------------------

def _r(x, nd=4):
    """a number that prints short; both drivers round it to binary32 where it enters a record, in the same way"""
    return round(float(x), nd)


def _v(xs, nd=4):
    return [_r(x, nd) for x in xs]


class _Gen:
    """The script writer of one scenario. It keeps the little it needs to write well-formed scripts: how many snapshots are pending, whether
    one has ended (queries), whether hits exist (SURFACE items), whether a heightfield is set, and roughly where the body is (colliders and
    fields are placed from the body's reference box moved by the placements so far, so that contacts happen)."""

    def __init__(self, seed, rng, b, sc):
        self.rng, self.b, self.sc, self.script = rng, b, sc, []
        self.pending, self.ended, self.have_hits, self.hf = 0, False, False, False
        self.shift = np.zeros(3)
        self.dt, self.S = b["dt"], b["S"]
        self.reacted = self.refused = False
        self.df = {}                         # signed-distance slot -> the arguments of the set that filled it

    # -- geometry
    def box(self):
        return self.b["lo"] + self.shift, self.b["hi"] + self.shift

    def add(self, name, **a):
        self.script.append([name, a])

    # -- ticks
    def tick(self, shape="same"):
        if shape == "other even S":
            self.S = self.S + 2 if self.S <= 6 else 4
        elif shape == "odd S":
            self.S = 3 if self.S != 3 else 5
        elif shape == "other dt":
            self.dt = 0.01 if self.dt != 0.01 else 0.02
        self.add("step", dt=self.dt, S=self.S)
        if self.S % 2:
            self.S = self.b["S"]            # an odd S is a visit: the tick after it is an ordinary one again

    # -- state-changing calls
    def impulses(self):
        rng, b = self.rng, self.b
        lo, hi = self.box()
        free = np.nonzero(b["mesh"].inv_mass != 0)[0]
        ids = rng.choice(free, size=3, replace=False)
        items = [["P", int(ids[0]), _v(rng.uniform(-1, 1, 3)), 0], ["P", int(b["pins"][0]), _v(rng.uniform(-1, 1, 3)), 0],
                 ["P", int(ids[1]), _v(rng.uniform(-0.5, 0.5, 3)), 1],
                 ["R", _v(lo + rng.uniform(0.2, 0.8, 3) * (hi - lo)), _r(0.5 * float((hi - lo).max())), _r(rng.uniform(-0.6, 0.6)), int(rng.integers(0, 2)), int(rng.integers(0, 2))]]
        self.add("apply_impulses", items=items)

    def need_hits(self):
        if not self.have_hits:
            self.need_snapshot()
            self.query()

    def need_snapshot(self):
        if not self.ended:
            if self.pending == 0:
                self.begin()
            self.end()

    def impulse_surface(self):
        self.need_hits()
        self.add("apply_impulses", items=[["S", _v(self.rng.uniform(-0.6, 0.6, 3)), int(self.rng.integers(0, 2))]])

    def place(self, style=None):
        rng = self.rng
        lo, hi = self.box()
        mid = (lo + hi) / 2
        style = style or str(rng.choice(["rigid", "mirror", "reference", "keep_pinned"]))
        move = rng.uniform(-0.05, 0.05, 3) * (hi - lo)
        quat = _v(np.concatenate([rng.uniform(-0.08, 0.08, 3), [1.0]]))
        a = dict(quat=None, mirror=None, frm=_v(mid), to=_v(mid + move), lin=None, ang=None, from_reference=False, keep_pinned=False)
        if style == "rigid":
            a["quat"] = quat
            if rng.random() < 0.4:
                a["lin"], a["ang"] = _v(rng.uniform(-0.3, 0.3, 3)), _v(rng.uniform(-0.1, 0.1, 3))
            self.shift = self.shift + move
        elif style == "mirror":
            a["mirror"] = int(rng.integers(0, 3)) if self.b["kind"] != "cloth" else 0
            a["to"] = a["frm"]
        elif style == "reference":
            rest_mid = (self.b["lo"] + self.b["hi"]) / 2
            a.update(quat=quat, frm=_v(rest_mid), to=_v(rest_mid + move), from_reference=True, lin=_v(rng.uniform(-0.3, 0.3, 3)), ang=_v(rng.uniform(-0.1, 0.1, 3)))
            self.shift = move
        else:                                # the free particles nudged, the pinned ones left where they are
            a.update(keep_pinned=True, to=_v(mid + 0.2 * move))
        self.add("place", **a)

    def surface_forces(self):
        rng = self.rng
        if self.sc["mode"] == "embedding":   # unsupported there (2e): the scenario's one planted refusal, or where that is spent, impulses
            return self.refuse("surface_forces_embedding") if not self.refused else self.impulses()
        self.add("apply_surface_forces", wind=_v(rng.uniform(-3, 3, 3)), normal=_r(rng.uniform(0.05, 0.4)), tangential=_r(rng.uniform(0.0, 0.1)),
                 pressure=_r(rng.uniform(-0.05, 0.05)), dt=self.dt)

    def colliders(self):
        rng = self.rng
        lo, hi = self.box()
        mid, ext = (lo + hi) / 2, hi - lo
        radius = 0.2 * float(ext.max()) if self.b["kind"] == "cloth" else 0.15 * float(ext.min())      # (under a sheet only its cap pokes through)
        cy = lo[1] - 0.9 * radius if self.b["kind"] == "cloth" else lo[1] + 0.1 * ext[1]
        sphere = ["sphere", _v(np.array([mid[0], cy, mid[2]]) + rng.uniform(-0.05, 0.05, 3) * ext), _r(radius),
                  _v([0.0, 0.1 * max(float(ext[1]), 1.0), 0.0]), _v(rng.uniform(-0.2, 0.2, 3)), _r(rng.uniform(0, 0.6)), _r(rng.uniform(0, 0.5))]
        half = [0.6 * ext[0], max(0.3 * ext[1], 0.3), 0.6 * ext[2]]
        box = ["box", _v([mid[0], lo[1] + 0.04 * max(ext[1], 1.0) - half[1], mid[2]]), _v(half), _v(np.concatenate([rng.uniform(-0.03, 0.03, 3), [1.0]])),
               _v(rng.uniform(-0.1, 0.1, 3)), [0.0, 0.0, 0.0], _r(rng.uniform(0, 0.6)), _r(rng.uniform(0, 0.5))]
        pick = int(rng.integers(0, 3))
        return [sphere] if pick == 0 else [box] if pick == 1 else [sphere, box]

    def collide(self):
        self.add("collide", colliders=self.colliders())

    def collide_with_reactions(self):
        self.add("collide_with_reactions", colliders=self.colliders())
        self.reacted = True

    def set_heightfield(self, scale=1.0, lift=0.0):
        lo, hi = self.box()
        if self.b["kind"] == "cloth":        # a sheet has no height of its own: the field's waves come from its span
            hi = hi + np.array([0.0, 0.25 * float((hi - lo).max()), 0.0])
            lift = lift + 0.004 * float((hi - lo).max())
        else:
            lift = lift + 0.03 * float(hi[1] - lo[1])
        self.add("set_heightfield", lo=_v(lo), hi=_v(hi), scale=_r(scale), lift=_r(lift))
        self.hf = True

    def collide_heightfield(self):
        if not self.hf:
            self.set_heightfield()
        self.add("collide_heightfield", friction=_r(self.rng.uniform(0, 0.8)), restitution=_r(self.rng.uniform(0, 0.5)))

    # -- signed-distance props (SPEC.md 2i): sized and placed from box(), as colliders() does
    def set_distance_field(self, slot=None, size=None, prop=None):
        """a table into `slot` (drawn where None). Over a full slot this is a replacement: size "same" keeps the sample count, so the memory
        is written over; "other" changes it, so the old table is released (drawn where None). `prop` names the prop of an empty slot."""
        rng = self.rng
        lo, hi = self.box()
        ext = hi - lo
        slot = int(rng.integers(0, DF_SLOTS)) if slot is None else slot
        old, n = self.df.get(slot), None
        if old is not None:
            size = size or ("same", "other")[int(rng.integers(0, 2))]
            if size == "same":
                prop, n = old["prop"], old.get("n")
            elif old["prop"] == "floor":
                prop = "sphere"
            elif rng.random() < 0.5:
                prop, n = "sphere", 26 - old["n"]      # 9 <-> 17
            else:
                prop = "floor"
        prop = prop or ("sphere", "floor")[int(rng.integers(0, 2))]
        if prop == "sphere":
            radius = (0.2 * float(ext.max()) if self.b["kind"] == "cloth" else 0.3 * float(min(ext[0], ext[2]))) * float(rng.uniform(0.9, 1.1))
            a = dict(slot=slot, prop="sphere", radius=_r(radius), n=int(n or rng.choice([9, 17])), thickness=_r(0.6 * radius))
        else:
            up = max(float(ext.max()), 1.0)
            a = dict(slot=slot, prop="floor", side=_r(4.0 * up), y0=_r(rng.uniform(-0.01, 0.01) * max(float(ext[1]), 1.0)), thickness=_r(2.0 * up))
        self.add("set_distance_field", **a)
        self.df[slot] = a

    def clear_distance_field(self, slot):
        self.add("clear_distance_field", slot=slot)
        self.df.pop(slot, None)

    def df_pose(self, slot):
        """where the prop of `slot` goes: the sphere with its cap in the body's underside (under the cloth only the cap pokes through), the
        floor a little above the body's lowest point; at rest or moving, half and half"""
        rng = self.rng
        lo, hi = self.box()
        mid, ext = (lo + hi) / 2, hi - lo
        t = self.df.get(slot, dict(prop="sphere", radius=1.0))
        up = max(float(ext[1]), 1.0)
        if t["prop"] == "sphere":
            radius = t["radius"]
            cy = lo[1] - 0.85 * radius if self.b["kind"] == "cloth" else lo[1] - radius + 0.12 * ext[1]
            centre = np.array([mid[0], cy, mid[2]]) + rng.uniform(-0.04, 0.04, 3) * np.array([ext[0], 0.25 * up, ext[2]])
            quat = np.concatenate([rng.uniform(-0.5, 0.5, 3), [1.0]])
        else:
            centre = np.array([mid[0], lo[1] + 0.05 * up, mid[2]]) + rng.uniform(-0.02, 0.02, 3) * np.array([ext[0], 0.25 * up, ext[2]])
            quat = np.concatenate([rng.uniform(-0.02, 0.02, 3), [1.0]])
        moving = bool(rng.integers(0, 2))
        lin = [0.0, 0.1 * up, 0.0] + rng.uniform(-0.05, 0.05, 3) * up if moving else np.zeros(3)
        ang = rng.uniform(-0.2, 0.2, 3) if moving else np.zeros(3)
        return dict(centre=_v(centre), quat=_v(quat), lin=_v(lin), ang=_v(ang), friction=_r(rng.uniform(0, 0.8)), restitution=_r(rng.uniform(0, 0.5)))

    def collide_distance_field(self, slot=None, empty=False):
        """a call on a full slot (one is filled where none is); with `empty`, on a slot that holds nothing (where there is one)"""
        rng = self.rng
        free = [s for s in range(DF_SLOTS) if s not in self.df]
        if slot is None and empty and free:
            slot = free[int(rng.integers(0, len(free)))]
        elif slot is None:
            if not self.df:
                self.set_distance_field()
            full = sorted(self.df)
            slot = full[int(rng.integers(0, len(full)))]
        self.add("collide_distance_field", slot=slot, **self.df_pose(slot))

    def set_state(self):
        self.add("set_state", seed=int(self.rng.integers(0, 2 ** 31)), shift=_v(self.shift), dx=0.02, dv=0.4)

    def get_velocities(self):
        self.add("get_velocities")

    def body_motion(self):
        self.add("get_body_state", what=int(self.rng.choice([MOTION, POSE | MOTION])))

    def call(self, name, k=None):
        if name == "place" and k is not None:      # the planted blocks walk through the four styles
            return self.place(("rigid", "mirror", "reference", "keep_pinned")[k % 4])
        getattr(self, name)()

    # -- steps that leave the tick held back
    def kinematic(self, twice=False):
        ext = self.b["hi"] - self.b["lo"]
        for _ in range(2 if twice else 1):
            self.add("set_kinematic_positions", offset=_v(self.rng.uniform(-0.002, 0.002, 3) * max(float(ext.max()), 1.0), 5), half=bool(self.rng.integers(0, 2)))

    def begin(self):
        assert self.pending < 2
        self.add("readback_begin"); self.pending += 1

    def end(self):
        assert self.pending > 0
        self.add("readback_end"); self.pending -= 1; self.ended = True

    def query(self, kind=None):
        rng = self.rng
        lo, hi = self.box()
        mid, ext = (lo + hi) / 2, np.maximum(hi - lo, 0.5)
        kind = kind or str(rng.choice(["raycast", "closest_points"]))
        m = int(rng.integers(2, 9))
        if kind == "raycast":
            org = mid + rng.choice([-1.0, 1.0], size=(m, 3)) * rng.uniform(0.7, 1.2, size=(m, 3)) * ext
            aim = mid + rng.uniform(-0.35, 0.35, size=(m, 3)) * ext
            rays = [_v(o) + [float("inf") if i % 3 else _r(3.0 * float(ext.max()))] + _v(t - o) + [0.0] for i, (o, t) in enumerate(zip(org, aim))]
            self.add("raycast", rays=rays)
        else:
            pts = mid + rng.uniform(-0.9, 0.9, size=(m, 3)) * ext
            self.add("closest_points", queries=[_v(p) + [float("inf") if i % 3 else _r(0.2 * float(ext.max()))] for i, p in enumerate(pts)])
        self.have_hits = True

    def fetch(self, twice=False):
        if self.reacted:
            self.add("collider_reactions", twice=bool(twice))

    def refuse(self, what):
        if what == "distance_field_slot_4":              # a valid pose on the slot behind the last
            self.add("refuse", what=what, pose=self.df_pose(0))
        elif what == "distance_field_restitution":       # restitution 1.5 on a full slot
            if not self.df:
                self.set_distance_field()
            slot = sorted(self.df)[int(self.rng.integers(0, len(self.df)))]
            self.add("refuse", what=what, slot=slot, pose=dict(self.df_pose(slot), restitution=1.5))
        else:
            self.add("refuse", what=what)
        self.refused = True

    def reads(self):
        self.add("get_positions"); self.add("get_velocities")

    def finish(self):
        while self.pending:
            self.end()
        self.reads()


def _config(seed, rng, body_kind=None, mode=None, peek0=None):
    kind = body_kind or BODIES[int(rng.integers(0, 4))]
    b = body(kind)
    if mode is None:
        mode = str(rng.choice(["full", "render_set", "embedding"])) if b["lattice"] else str(rng.choice(["full", "render_set"]))
    if mode == "embedding" and not b["lattice"]:
        mode = "render_set"
    return dict(seed=int(seed), body=kind, peek0=bool(rng.integers(0, 2)) if peek0 is None else bool(peek0), graph=bool(rng.integers(0, 2)), mode=mode,
                uvs=bool(rng.integers(0, 2)), every_tick=bool(rng.integers(0, 2)))


_REFUSALS = ("reactions_1025", "third_snapshot", "kinematic_free_particle", "step_dt_zero", "surface_forces_embedding")


_REFUSALS_2 = _REFUSALS + ("distance_field_slot_4", "distance_field_restitution")      # drawn from for seeds behind the first block


def _plant_refusal(G, rng, refusals=_REFUSALS):
    """one refusal per scenario, where it IS one: a third snapshot needs two pending, the surface forces an embedding"""
    what = str(rng.choice(refusals))
    if G.refused:
        return
    if G.sc["mode"] == "embedding" and rng.random() < 0.5:
        what = "surface_forces_embedding"
    elif what == "surface_forces_embedding" and G.sc["mode"] != "embedding":
        what = "reactions_1025"
    if what == "third_snapshot":
        while G.pending < 2:
            G.begin()
    G.refuse(what)


def _random_script(G, rng, sc, extended):
    """the randomly drawn script. `extended` (every seed behind the first block): state-changing calls are drawn from ALL -- a call on a
    slot that holds nothing one time in four --, the branch that sets or clears the heightfield is shared evenly with set / replace / clear
    of a signed-distance slot, and the refusal is drawn from the extended list. Without it not one draw differs from what the first block
    was generated with."""
    calls, refusals = (ALL, _REFUSALS_2) if extended else (STATE_CHANGING, _REFUSALS)
    frames = int(rng.integers(4, 8))
    refusal_at = int(rng.integers(0, frames))
    late_fetch = False
    for f in range(frames):
        n_between = int(rng.integers(0, 4))
        for _ in range(n_between):
            r = rng.random()
            if r < 0.55:
                call = str(rng.choice(calls))
                if call == D:
                    G.collide_distance_field(empty=rng.random() < 0.25)
                else:
                    G.call(call)
                if call == "collide_with_reactions":
                    if rng.random() < 0.5:
                        G.fetch(twice=rng.random() < 0.5)
                    else:
                        late_fetch = True
            elif r < 0.7:
                G.kinematic(twice=rng.random() < 0.3)
            elif r < 0.8:
                if extended and rng.random() < 0.5:
                    slot = int(rng.integers(0, DF_SLOTS))
                    if slot in G.df and rng.random() < 0.4:
                        G.clear_distance_field(slot)
                    else:
                        G.set_distance_field(slot)                                        # (a replacement where the slot is full)
                elif G.hf and rng.random() < 0.6:
                    G.add("clear_heightfield"); G.hf = False
                else:
                    G.set_heightfield(scale=float(rng.choice([1.0, 1.5, 0.5])))      # (a replacement, where one is set, right behind a call)
            elif r < 0.9:
                G.add(str(rng.choice(["get_positions", "get_bounds"])))
            else:
                G.add("get_body_state", what=POSE)
        if f == refusal_at:
            _plant_refusal(G, rng, refusals)
        G.tick(str(rng.choice(TICK_SHAPES, p=[0.55, 0.15, 0.15, 0.15])))
        if late_fetch:
            G.fetch(twice=rng.random() < 0.5); late_fetch = False
        r = rng.random()
        if r < 0.35 and G.pending < 2:      # ended at once
            G.begin(); G.end()
        elif r < 0.7:                        # pipelined: at most two pending, the oldest ended first
            if G.pending == 2:
                G.end()
            G.begin()
        elif G.pending and rng.random() < 0.5:
            G.end()
        if G.ended and rng.random() < 0.5:
            G.query()
        if sc["every_tick"]:
            G.reads()
    G.finish()


def _second_block_scenario(seed, rng):
    """Seeds behind the first block. N2_PAIRS scenarios: (D, X) and (X, D) for each of the ten calls of STATE_CHANGING and (D, D) on two
    slots, in the shape of the first block's pairs -- the table set before the first tick -- and closed by what happens to a prop sooner or
    later: it is replaced (even j) or cleared and called once more (odd j) right behind a call. N2_PLANTED: D behind each left state, in
    front of each tick shape. N2_LIFETIMES: DF_LIFETIMES, the tick held back (every body's S is even); sc["leaves_held_back"] lists the
    steps that must not complete it, each with nothing but such steps between it and the next tick, which therefore fuses. All others: the
    random generator, extended."""
    j = seed - len(FIRST_BLOCK)
    if j < N2_PAIRS:
        A, B = DF_PAIRS[j]
        mode = ["full", "render_set"][j % 2] if "surface_forces" in (A, B) else None
        # (every sixth scenario moves the pins right in front of D on a lattice body: tests/frame_group_case.py cuts windows from those)
        sc = _config(seed, rng, BODIES[(j // 6) % 2] if j % 6 == 0 else BODIES[(j + j // 4) % 4], mode)
        sc["plan"] = f"pair {A} -> {B}"
        G = _Gen(seed, rng, body(sc["body"]), sc)
        if "collide_heightfield" in (A, B):
            G.set_heightfield()
        slots = [j % DF_SLOTS, (j + 1 + j // DF_SLOTS % 3) % DF_SLOTS]
        G.set_distance_field(slots[0], prop=("sphere", "floor")[j % 2])
        if (A, B) == (D, D):
            G.set_distance_field(slots[1], prop="floor")
        G.tick(); G.tick()
        if "impulse_surface" in (A, B):
            G.need_hits()
        if sc["every_tick"]:
            G.add("get_positions")
        if j % 3 == 0 and len(G.b["pins"]):
            G.kinematic()
        for k, c in enumerate((A, B)):
            if c == D:
                G.collide_distance_field(slots[k] if (A, B) == (D, D) else slots[0])
            else:
                G.call(c, j + k)
        if "collide_with_reactions" in (A, B):
            G.fetch(twice=j % 2 == 0)
        G.tick(); G.tick()
        G.collide_distance_field(slots[0])
        if j % 2 == 0:
            G.set_distance_field(slots[0], size=("same", "other")[j // 2 % 2])
            G.collide_distance_field(slots[0])
        else:
            G.clear_distance_field(slots[0])
            G.collide_distance_field(slots[0])
        _plant_refusal(G, rng, _REFUSALS_2)
        G.tick()
        G.finish()
    elif j < N2_PAIRS + N2_PLANTED:
        k = j - N2_PAIRS
        left, shape = LEFT_STATES[k], TICK_SHAPES[(k + 1) % 4]
        sc = _config(seed, rng, BODIES[(k + 1) % 4], None, peek0=True if k == 0 else None)
        sc["plan"] = f"{D} behind '{left}', in front of a tick of shape '{shape}'"
        G = _Gen(seed, rng, body(sc["body"]), sc)
        G.set_distance_field(k, prop=("sphere", "floor")[k % 2])
        G.tick(); G.tick()
        if k == 0:
            G.add("get_positions")
        elif k == 2:
            G.add("get_velocities")
        elif k == 3:
            G.kinematic()
        G.collide_distance_field(k)
        G.tick(shape); G.tick()
        _plant_refusal(G, rng, _REFUSALS_2)
        G.tick()
        G.finish()
    elif j < N2_PAIRS + N2_PLANTED + N2_LIFETIMES:
        k = j - N2_PAIRS - N2_PLANTED
        sc = _config(seed, rng, BODIES[k % 4], None)
        sc["plan"] = "table lifetime: " + DF_LIFETIMES[k]
        G = _Gen(seed, rng, body(sc["body"]), sc)
        held = []                            # the steps that must leave the tick held back
        s0, s1 = k % DF_SLOTS, (k + 2) % DF_SLOTS

        def quiet(fn, *a, **kw):
            fn(*a, **kw); held.append(len(G.script) - 1)
        if k == 0:
            G.tick(); G.tick()
            quiet(G.set_distance_field, s0, prop="sphere")
            G.tick(); G.tick()
            G.collide_distance_field(s0)
            G.tick(); G.tick()
            quiet(G.set_distance_field, s0, size="other")      # (nothing reads the slot any more: the tick stays held back all the same)
            G.tick()
        elif k in (1, 2):
            G.set_distance_field(s0, prop=("floor", "sphere")[k - 1])
            G.tick(); G.tick()
            G.collide_distance_field(s0)
            G.set_distance_field(s0, size=("same", "other")[k - 1])
            G.collide_distance_field(s0)
            G.tick(); G.tick()
            G.collide_distance_field(s0)
            G.tick(); G.tick()
            quiet(G.set_distance_field, s0, size=("same", "other")[k - 1])      # the pass before is long done: the wait finds nothing
            G.tick()
            G.collide_distance_field(s0)
        elif k == 3:
            G.set_distance_field(s0, prop="sphere")
            G.tick(); G.tick()
            G.collide_distance_field(s0)
            G.clear_distance_field(s0)
            G.collide_distance_field(s0)
            G.tick(); G.tick()
            G.set_distance_field(s0, prop="floor")
            G.tick()
            G.collide_distance_field(s0)
            G.tick(); G.tick()
            quiet(G.clear_distance_field, s0)
            quiet(G.collide_distance_field, s0)
            G.tick()
        elif k == 4:
            G.set_distance_field(s0, prop="floor")
            G.tick(); G.tick()
            quiet(G.collide_distance_field, s1)
            G.tick()
            quiet(G.collide_distance_field, s1)
            G.tick()
            G.collide_distance_field(s1); G.collide_distance_field(s0)
            G.tick(); G.tick()
            G.collide_distance_field(s0); G.collide_distance_field(s1)
        elif k == 5:                         # the order of csharp/Softbody.cs: colliders, terrain, then props
            G.set_heightfield()
            G.set_distance_field(s0, prop="sphere"); G.set_distance_field(s1, prop="floor")
            G.tick(); G.tick()
            for _ in range(2):
                G.collide_with_reactions(); G.collide_heightfield()
                G.collide_distance_field(s0); G.collide_distance_field(s0); G.collide_distance_field(s1)
                G.fetch()
                G.tick()
        else:                                # the snapshot is the state at ITS readback_begin
            G.set_distance_field(s0, prop="sphere")
            G.tick(); G.tick()
            G.begin()
            G.collide_distance_field(s0)
            G.end()
            G.query("raycast"); G.query("closest_points")
            G.tick()
            G.begin()
            G.collide_distance_field(s0)
            G.tick()
            G.end()
            G.query("closest_points"); G.query("raycast")
        G.tick(); G.tick()
        _plant_refusal(G, rng, _REFUSALS_2)
        G.tick()
        G.finish()
        sc["leaves_held_back"] = held
    else:
        sc = _config(seed, rng)
        sc["plan"] = "random"
        G = _Gen(seed, rng, body(sc["body"]), sc)
        _random_script(G, rng, sc, extended=True)
    sc["script"] = G.script
    return sc


def make_scenario(seed):
    """The scenario of a seed. 0 .. N_PAIRS-1: the ordered pair (A, B) of state-changing calls back to back in one frame; the next N_PLANTED:
    each call behind each state the last tick can have left, and in front of each tick shape; the rest of FIRST_BLOCK drawn at random, without
    a signed-distance step. Every seed behind FIRST_BLOCK: _second_block_scenario."""
    rng = np.random.default_rng([20250611, int(seed)])
    if seed >= len(FIRST_BLOCK):
        return _second_block_scenario(seed, rng)
    nC = len(STATE_CHANGING)
    if seed < N_PAIRS:
        A, B = STATE_CHANGING[seed // nC], STATE_CHANGING[seed % nC]
        mode = None
        if "surface_forces" in (A, B):
            mode = ["full", "render_set"][seed % 2]
        sc = _config(seed, rng, BODIES[(seed // nC + 2 * (seed % nC)) % 4], mode)
        sc["plan"] = f"pair {A} -> {B}"
        G = _Gen(seed, rng, body(sc["body"]), sc)
        if "collide_heightfield" in (A, B):
            G.set_heightfield()
        G.tick(); G.tick()
        if "impulse_surface" in (A, B):
            G.need_hits()                    # (a snapshot and a query: they leave the tick as it is where peeking is on)
        if sc["every_tick"]:
            G.add("get_positions")
        if seed % 3 == 0 and len(G.b["pins"]):
            G.kinematic()
        G.call(A, seed); G.call(B, seed + 1)
        if A == "collide_with_reactions" or B == "collide_with_reactions":
            G.fetch(twice=seed % 2 == 0)
        G.tick(); G.tick()
        _plant_refusal(G, rng)
        G.tick()
        G.finish()
    elif seed < N_PAIRS + N_PLANTED:
        j = seed - N_PAIRS
        c, k = j // 4, j % 4
        call, left, shape = STATE_CHANGING[c], LEFT_STATES[k], TICK_SHAPES[(k + c) % 4]
        mode = ["full", "render_set"][j % 2] if call == "surface_forces" else None
        sc = _config(seed, rng, BODIES[(c + k) % 4], mode, peek0=True if k == 0 else None)
        sc["plan"] = f"{call} behind '{left}', in front of a tick of shape '{shape}'"
        G = _Gen(seed, rng, body(sc["body"]), sc)
        if call == "collide_heightfield":
            G.set_heightfield()
        G.tick(); G.tick()
        if call == "impulse_surface":
            G.need_hits()
        if k == 0:
            G.add("get_positions")
        elif k == 2:
            G.add("get_velocities")
        elif k == 3:
            G.kinematic()
        G.call(call, j)
        if call == "collide_with_reactions":
            G.fetch()
        G.tick(shape); G.tick()
        _plant_refusal(G, rng)
        G.tick()
        G.finish()
    else:
        sc = _config(seed, rng)
        sc["plan"] = "random"
        G = _Gen(seed, rng, body(sc["body"]), sc)
        _random_script(G, rng, sc, extended=False)
    sc["script"] = G.script
    return sc


def for_ranks(sc):
    """the scenario for a group of several ranks: surface forces are unsupported there (2e), so each such step becomes an expected refusal"""
    out = dict(sc)
    out["script"] = [["refuse", {"what": "surface_forces_ranks"}] if name == "apply_surface_forces" else [name, a] for name, a in sc["script"]]
    return out


def defer_fetches(sc):
    """the twin of a scenario: every collider_reactions fetch moved behind the next tick (or to the end of the script)"""
    out, held = [], []
    for name, a in sc["script"]:
        if name == "collider_reactions":
            held.append([name, a])
            continue
        out.append([name, a])
        if name == "step" and held:
            out += held; held = []
    twin = dict(sc)
    twin["script"] = out + held
    return twin


def chunks():
    return [FIXED_SLICE[i:i + CHUNK] for i in range(0, len(FIXED_SLICE), CHUNK)]
