"""Inputs of the float-range tests (tests/test_float_range_oracles.py on the CPU, tests/test_gpu_float_range.py on the GPU): tets and
hinges whose size sweeps the binary32 range, the exact degeneracies that reach every skip predicate of SPEC.md 5 and 6, and free particles
whose whole state is subnormal. No test lives here.

Every constrained mesh is a set of INDEPENDENT constraints (no two share a particle) around the origin, like the springs of
test_spring_lengths_across_the_float_range: a constraint of scale L = 2^e has coordinates of order L, so its intermediates are
    tet:   g ~ L^2, dot(g, g) ~ L^4, C6 ~ L^3          hinge: n ~ L^2, q1, q2 ~ L^4, el ~ L
and L^4 is subnormal for e in about (-37, -31.5), zero below, infinite above e = 32. Gravity must be (0, 0, 0) in every run of them: h*h*g is
about 1e-6 and would lift the small scales off the origin.

The meshes carry what the tests need to place a failure: mesh.units, one Unit per constraint type with the particles, the scale exponent
and the row class of every constraint.
"""
import functools
from dataclasses import dataclass

import numpy as np

from softbodyunity_amd.mesh import SoftbodyMesh

f32 = np.float32
SEED = 5
DT = 0.02
NO_GRAVITY = (0.0, 0.0, 0.0)
SWEEP_TICKS, SWEEP_SUBSTEPS = 1, 2
# (distance, volume, bending) compliance: rigid reaches den = 0 on fully pinned constraints and wherever L^4 underflows; compliant turns
# those into den = at and den ~ at
COMPLIANCES = {"rigid": (0.0, 0.0, 0.0), "compliant": (1e-6, 1e-6, 1e-4)}
SUBNORMAL_RUN = dict(gravity=NO_GRAVITY, damping=0.5, ground_plane=(0.0, 1.0, 0.0, 0.0), ticks=2, substeps=3)
W_CHOICES = np.array([0.0, 0.5, 1.0, 3.0], f32)


def n_degenerate(m):
    """The first rows of a unit of m tets or hinges are degenerate, a quarter of them per degeneracy: 64 of 4096 (rows 0 .. 63, 16 each)."""
    return 4 * (m // 256)

ROW_CLASSES = ("degenerate", "underflow cluster", "overflow cluster", "sweep")


@dataclass
class Unit:
    kind: str                # "dist", "vol" or "bend"
    particles: np.ndarray    # (m, 2 or 4) particle ids
    e: np.ndarray            # (m,) scale exponent: L = 2^e
    row_class: np.ndarray    # (m,) index into ROW_CLASSES


def _exponents(rng, m):
    """m - m/4 exponents over the whole range, then m/8 where L^4 is subnormal or underflows, then m/8 where it overflows."""
    return np.concatenate([rng.uniform(-44.0, 40.0, m - 2 * (m // 8)), rng.uniform(-38.5, -30.5, m // 8), rng.uniform(27.5, 33.5, m // 8)])


def _row_classes(m, quads):
    c = np.full(m, 3, np.int8)
    c[m - 2 * (m // 8):m - m // 8] = 1
    c[m - m // 8:] = 2
    if quads:
        c[:n_degenerate(m)] = 0
    return c


def _quad_positions(rng, m):
    e = _exponents(rng, m)
    base = rng.normal(size=(m, 4, 3))
    d = n_degenerate(m) // 4
    base[0:d, 1] = base[0:d, 0]                                             # hinge: el = 0; tet: flat
    base[d:2 * d, 2] = 0.5 * (base[d:2 * d, 0] + base[d:2 * d, 1])          # hinge: wing c on the edge, q1 at or near 0
    base[2 * d:3 * d, 3] = base[2 * d:3 * d, 0]                             # hinge: wing d on vertex a, q2 = 0; tet: flat
    base[3 * d:4 * d, :, 2] = 0.0                                           # flat tet; hinge with phi = 0 or pi
    return e, (base * np.exp2(e)[:, None, None]).astype(f32)


def _vol_rest(rng, pos):
    p = pos.astype(np.float64)
    vol = np.einsum("ij,ij->i", p[:, 1] - p[:, 0], np.cross(p[:, 2] - p[:, 0], p[:, 3] - p[:, 0])) / 6.0
    return (vol * rng.uniform(0.5, 1.5, len(pos))).astype(f32)      # inverted and zero rest volumes as they fall


def _bend_rest(rng, m):
    phi0 = rng.uniform(-3.0, 3.0, m)
    return np.stack([np.cos(phi0), np.sin(phi0)], axis=1).astype(f32)


def _assemble(parts, w):
    """parts: [(kind, e, pos (m, k, 3), rest)] -> mesh whose particles are the parts' vertices in order."""
    kw, units, first = {}, [], 0
    for kind, e, pos, rest in parts:
        m, k = pos.shape[:2]
        ids = (first + np.arange(m * k)).reshape(m, k).astype(np.int32)
        first += m * k
        kw.update({"dist": dict(dist_ij=ids, dist_rest=rest), "vol": dict(vol_ijkl=ids, vol_rest=rest), "bend": dict(bend_ijkl=ids, bend_rest=rest)}[kind])
        units.append(Unit(kind, ids, e, _row_classes(m, k == 4)))
    kw.setdefault("dist_ij", np.zeros((0, 2), np.int32)); kw.setdefault("dist_rest", np.zeros(0, f32))
    pos = np.concatenate([p.reshape(-1, 3) for _, _, p, _ in parts])
    mesh = SoftbodyMesh(rest_pos=pos.copy(), pos=pos.copy(), vel=np.zeros_like(pos), inv_mass=w, **kw)
    mesh.units = units
    return mesh


def quad_sweep(kind, seed=SEED, n=4096):
    """n independent tets ("vol") or hinges ("bend") on particles 4k .. 4k+3."""
    rng = np.random.default_rng(seed)
    e, pos = _quad_positions(rng, n)
    w = rng.choice(W_CHOICES, 4 * n)                                # (0.4 % of the quads are pinned four times)
    rest = _vol_rest(rng, pos) if kind == "vol" else _bend_rest(rng, n)
    return _assemble([(kind, e, pos, rest)], w)


def mixed_sweep(seed=SEED, n=4096):
    """n/2 springs on their own particle pairs, n/4 tets, n/4 hinges, every type over the whole range of scales: the tiles hold hinge
    rows, tet quads and spring lanes side by side."""
    rng = np.random.default_rng(seed)
    e_d = _exponents(rng, n // 2)
    ends = (rng.normal(size=(n // 2, 2, 3)) * np.exp2(e_d)[:, None, None]).astype(f32)
    length = np.linalg.norm(ends[:, 0].astype(np.float64) - ends[:, 1], axis=1)
    e_v, tets = _quad_positions(rng, n // 4)
    e_b, hinges = _quad_positions(rng, n // 4)
    w = rng.choice(W_CHOICES, 2 * (n // 2) + 8 * (n // 4))
    rest_d = (length * rng.uniform(0.5, 1.5, n // 2)).astype(f32)
    return _assemble([("dist", e_d, ends, rest_d), ("vol", e_v, tets, _vol_rest(rng, tets)), ("bend", e_b, hinges, _bend_rest(rng, n // 4))], w)


def subnormal_particles(seed=SEED, n=4096):
    """n particles without constraints: velocities +-2^U(-140,-116) per component, positions 0 (first half) or 2^U(-149,-120)."""
    rng = np.random.default_rng(seed)
    vel = (rng.choice([-1.0, 1.0], (n, 3)) * np.exp2(rng.uniform(-140.0, -116.0, (n, 3)))).astype(f32)
    pos = np.zeros((n, 3), f32)
    pos[n // 2:] = np.exp2(rng.uniform(-149.0, -120.0, (n - n // 2, 3))).astype(f32)
    w = rng.choice(W_CHOICES, n)
    mesh = SoftbodyMesh(rest_pos=pos.copy(), pos=pos.copy(), vel=vel, inv_mass=w, dist_ij=np.zeros((0, 2), np.int32), dist_rest=np.zeros(0, f32))
    mesh.units = []
    return mesh


SWEEP_CASES = ("vol", "bend", "mixed")


@functools.lru_cache(maxsize=None)
def case(name, seed=SEED):
    """The shared, never modified mesh of a case name."""
    if name == "mixed":
        return mixed_sweep(seed)
    if name == "subnormal":
        return subnormal_particles(seed)
    return quad_sweep(name, seed)


# ---- conditions on the inputs (not tolerances): the sweep reaches both sides of every skip, the subnormal state stays subnormal --------

def moved_units(mesh, x):
    """Per unit: which constraints have a particle whose position differs from the initial one."""
    changed = (np.asarray(x) != mesh.pos).any(axis=1)
    return [changed[u.particles].any(axis=1) for u in mesh.units]


def check_sweep_conditions(mesh, x, rigid):
    """No tet or hinge moved where L^4 is zero (e < -40) or infinite (e > 34); rigid: at least 0.95 of the constraints of every type with
    -34 < e < 26 and a free particle moved. -> the moved shares, per unit."""
    assert np.isfinite(x).all(), f"{int((~np.isfinite(x)).any(axis=1).sum())} particles with a non-finite coordinate"
    shares = []
    for u, moved in zip(mesh.units, moved_units(mesh, x)):
        if u.particles.shape[1] == 4:
            still = (u.e < -40.0) | (u.e > 34.0)
            assert still.sum() >= 0.05 * len(u.e) and not moved[still].any(), f"{u.kind}: {int(moved[still].sum())} constraints outside the range of L^4 moved"
        live = (u.e > -34.0) & (u.e < 26.0) & (mesh.inv_mass[u.particles] > 0).any(axis=1)
        shares.append(float(moved[live].mean()))
        if rigid:
            assert live.sum() >= 0.3 * len(u.e) and shares[-1] >= 0.95, f"{u.kind}: only {shares[-1]:.3f} of the constraints in range moved"
    return shares


def _subnormal_rows(a):
    a = np.abs(np.asarray(a))
    return ((a > 0) & (a < np.finfo(f32).tiny)).any(axis=1)


def check_subnormal_conditions(mesh, x, v):
    """At least 0.8 of the free particles end with a nonzero subnormal coordinate in x, and in v. -> the two shares."""
    assert np.isfinite(x).all() and np.isfinite(v).all()
    free = mesh.inv_mass > 0
    sx, sv = float(_subnormal_rows(x)[free].mean()), float(_subnormal_rows(v)[free].mean())
    assert sx >= 0.8 and sv >= 0.8, f"subnormal share of the free particles: x {sx:.3f}, v {sv:.3f}"
    return sx, sv


def describe_mismatch(mesh, got, want, what, limit=6):
    """Where a bitwise comparison failed: how many constraints (or particles), the scale exponent and row class of the first few."""
    bad = (np.ascontiguousarray(got, f32).view(np.uint32) != np.ascontiguousarray(want, f32).view(np.uint32)).any(axis=1)
    lines = [f"{what}: {int(bad.sum())} of {len(bad)} particles differ"]
    for u in mesh.units:
        rows = np.nonzero(bad[u.particles].any(axis=1))[0]
        if len(rows):
            first = ", ".join(f"row {r} e={u.e[r]:.2f} ({ROW_CLASSES[u.row_class[r]]})" for r in rows[:limit])
            lines.append(f"  {u.kind}: {len(rows)} of {len(u.e)} constraints differ; first: {first}")
    if not mesh.units:
        rows = np.nonzero(bad)[0][:limit]
        lines.append("  first: " + ", ".join(f"particle {r} w={mesh.inv_mass[r]} got {got[r]} want {want[r]}" for r in rows))
    return "\n".join(lines)
