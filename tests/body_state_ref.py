"""Reference for the body state (SPEC.md 6f; sb_group_get_body_state / sb_group_body_state_from_sums), shared by tests/test_body_state.py,
tests/test_gpu_body_state.py and tests/body_state_group_case.py.

The 32 sums and, per slot, A_k -- the sum of the absolute values of every elementary product -- in np.longdouble (64-bit mantissa on x86:
the reference's own error is n 2^-63 A_k, 2^-11 of the bound it checks); the derived values from given sums in numpy float64, the polar
factor through np.linalg.svd."""
import numpy as np

LD = np.longdouble
POSE, MOTION = 1, 2
NO_MASS, DEGENERATE_POSE, DEGENERATE_INERTIA = 1, 2, 4
GROUPS_CAP = 1024           # mirrors kBodyMaxGroups of csrc/body_state_kernels.hip.hpp
LANES = 256
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1000, GROUPS_CAP * LANES + 1, 3 * GROUPS_CAP * LANES + 77)
SEED = 20240611
U = 2.0 ** -53


def longdouble_is_extended():
    return np.finfo(LD).nmant == 63


def requested(what):
    """bool[32]: the slots a query for `what` produces (SPEC.md 6f's table)"""
    r = np.zeros(32, bool)
    r[0:4] = True; r[7:13] = True
    if what & POSE:
        r[4:7] = True; r[13:22] = True
    if what & MOTION:
        r[22:29] = True
    return r


def sums_ref(x, v, w, q, what):
    """-> dict: sums (32, longdouble; unrequested slots 0), A (32: sum of |elementary product|), min_term (32: the smallest |contribution
    of one dynamic particle|, inf without one), n_dynamic, n_pinned. Pinned rows (w <= 0 or NaN) are only counted."""
    w = np.asarray(w, np.float32)
    dyn = w > 0
    n_dyn = int(dyn.sum())
    m = LD(1) / w[dyn].astype(LD)
    X = np.asarray(x, np.float32)[dyn].astype(LD)
    V = np.asarray(v, np.float32)[dyn].astype(LD)
    Q = np.asarray(q, np.float32)[dyn].astype(LD)
    terms = {}       # slot -> the elementary products of a particle's contribution, one array each (made when the slot is summed)
    terms[0] = lambda: [m]
    for c in range(3):
        terms[1 + c] = lambda c=c: [m * X[:, c]]
        terms[4 + c] = lambda c=c: [m * Q[:, c]]
        terms[22 + c] = lambda c=c: [m * V[:, c]]
    for k, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        terms[7 + k] = lambda a=a, b=b: [m * X[:, a] * X[:, b]]
    for a in range(3):
        for b in range(3):
            terms[13 + 3 * a + b] = lambda a=a, b=b: [m * X[:, a] * Q[:, b]]
    for c, (a, b) in enumerate(((1, 2), (2, 0), (0, 1))):
        terms[25 + c] = lambda a=a, b=b: [m * X[:, a] * V[:, b], -(m * X[:, b] * V[:, a])]
    terms[28] = lambda: [m * V[:, c] * V[:, c] for c in range(3)]
    req = requested(what)
    sums = np.zeros(32, LD); A = np.zeros(32, LD); min_term = np.full(32, np.inf)
    for k, make in terms.items():
        if not req[k]:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            parts = make()
            contribution = parts[0] if len(parts) == 1 else np.sum(np.stack(parts), axis=0)
            sums[k] = contribution.sum()
            A[k] = sum(np.abs(p).sum() for p in parts)
            if n_dyn:
                min_term[k] = float(np.abs(contribution).min())
    return dict(sums=sums, A=A, min_term=min_term, n_dynamic=n_dyn, n_pinned=int(w.shape[0] - n_dyn))


def bound(ref):
    """SPEC.md 6f, binding: |sum_k - exact_k| <= (n_dyn + 16) 2^-52 A_k"""
    return LD(ref["n_dynamic"] + 16) * LD(2.0 ** -52) * ref["A"]


def check_sums(got, ref, what):
    """-> list of complaints: a requested slot outside the bound, an unrequested slot that is not exactly 0"""
    why = []
    req = requested(what)
    b = bound(ref)
    got = np.asarray(got, np.float64)
    for k in range(32):
        if not req[k]:
            if got[k] != 0.0 or np.signbit(got[k]):
                why.append(f"slot {k} was not requested and reads {got[k]!r}")
            continue
        err = abs(LD(got[k]) - ref["sums"][k])
        if not err <= b[k]:
            why.append(f"slot {k}: {got[k]!r} for {ref['sums'][k]!r}, off by {float(err):.3e}, bound {float(b[k]):.3e}")
    return why


def worst_ratio(got, ref, what):
    """max over the requested slots of error / bound (0 where the bound is 0 and the sum exact): the figure a test prints"""
    req = requested(what); b = bound(ref); worst = 0.0
    for k in np.nonzero(req)[0]:
        err = abs(LD(got[k]) - ref["sums"][k])
        if b[k] > 0:
            worst = max(worst, float(err / b[k]))
        elif err != 0:
            worst = float("inf")
    return worst


# ---- derived values -------------------------------------------------------------------------------------------------------------------------

def quaternion_of(R):
    """unit quaternion (x, y, z, w), w >= 0, of a rotation matrix"""
    tr = np.trace(R)
    if tr > 0:
        S = 2 * np.sqrt(tr + 1)
        q = [(R[2, 1] - R[1, 2]) / S, (R[0, 2] - R[2, 0]) / S, (R[1, 0] - R[0, 1]) / S, S / 4]
    else:
        i = int(np.argmax(np.diag(R))); j, k = (i + 1) % 3, (i + 2) % 3
        S = 2 * np.sqrt(1 + R[i, i] - R[j, j] - R[k, k])
        q = [0.0, 0.0, 0.0, (R[k, j] - R[j, k]) / S]
        q[i] = S / 4; q[j] = (R[j, i] + R[i, j]) / S; q[k] = (R[k, i] + R[i, k]) / S
    q = np.array(q, np.float64)
    q /= np.linalg.norm(q)
    return -q if q[3] < 0 else q


def rotation_of(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def kabsch(apq):
    """-> (R or None below rank 2, singular values, sign of det): the polar factor of apq with det = +1, the smallest direction flipped
    where det(apq) < 0"""
    Uu, s, Vt = np.linalg.svd(apq)
    d = np.sign(np.linalg.det(Uu) * np.linalg.det(Vt))
    if not s[1] > 1e-12 * s[0]:
        return None, s, d
    D = np.diag([1.0, 1.0, d if d != 0 else 1.0])
    if s[2] <= 1e-12 * s[0]:            # planar pose: the third pair is whatever completes two right-handed frames
        u3 = np.cross(Uu[:, 0], Uu[:, 1]); v3 = np.cross(Vt[0], Vt[1])
        return np.outer(Uu[:, 0], Vt[0]) + np.outer(Uu[:, 1], Vt[1]) + np.outer(u3, v3), s, d
    return Uu @ D @ Vt, s, d


def derive_ref(sums, n_dynamic, n_pinned, what):
    """SPEC.md 6f "Derived values" in numpy float64 from 32 given sums -> dict with sb_body_state's field names"""
    S = np.where(requested(what), np.asarray(sums, np.float64), 0.0)
    o = dict(n_dynamic=n_dynamic, n_pinned=n_pinned, what=what, flags=0, sums=S, mass=0.0, com=np.zeros(3), ref_com=np.zeros(3),
             second_moment=np.zeros(6), apq=np.zeros((3, 3)), rotation=np.array([0.0, 0.0, 0.0, 1.0]), momentum=np.zeros(3), velocity=np.zeros(3),
             angular_momentum=np.zeros(3), angular_velocity=np.zeros(3), kinetic_energy=0.0)
    if n_dynamic == 0:
        o["flags"] = NO_MASS; o["sums"] = np.zeros(32)
        return o
    M = S[0]
    o["mass"] = M
    com = S[1:4] / M
    o["com"] = com
    xx = np.array([com[0] * com[0], com[1] * com[1], com[2] * com[2], com[0] * com[1], com[0] * com[2], com[1] * com[2]])
    C6 = S[7:13] - M * xx
    o["second_moment"] = C6
    C = np.array([[C6[0], C6[3], C6[4]], [C6[3], C6[1], C6[5]], [C6[4], C6[5], C6[2]]])
    if what & POSE:
        o["ref_com"] = S[4:7] / M
        o["apq"] = S[13:22].reshape(3, 3) - M * np.outer(com, o["ref_com"])
        R, _, _ = kabsch(o["apq"])
        if R is None:
            o["flags"] |= DEGENERATE_POSE
        else:
            o["rotation"] = quaternion_of(R)
    if what & MOTION:
        P = S[22:25]
        o["momentum"] = P; o["velocity"] = P / M
        o["angular_momentum"] = S[25:28] - np.cross(com, P)
        o["kinetic_energy"] = 0.5 * S[28]
        inertia = np.trace(C) * np.eye(3) - C
        lam = np.linalg.eigvalsh(inertia)
        if lam[0] <= 1e-12 * lam[2]:
            o["flags"] |= DEGENERATE_INERTIA
        else:
            o["angular_velocity"] = np.linalg.solve(inertia, o["angular_momentum"])
    return o


def inertia_of(second_moment):
    C6 = np.asarray(second_moment, np.float64)
    C = np.array([[C6[0], C6[3], C6[4]], [C6[3], C6[1], C6[5]], [C6[4], C6[5], C6[2]]])
    return np.trace(C) * np.eye(3) - C


def field_scales(sums, n_dynamic):
    """The natural magnitude of every derived field, from the sums themselves: L the rms distance of the mass from the origin, Lq the same
    of the reference pose's centre, Uv the rms speed. An error of eps relative to A_k in the sums moves a field by about eps times its scale
    (times the condition number of the solve behind angular_velocity and rotation: kappa_inertia, kappa_pose)."""
    S = np.asarray(sums, np.float64)
    M = S[0]
    L = np.sqrt((S[7] + S[8] + S[9]) / M)
    Uv = np.sqrt(max(S[28], 0.0) / M)
    Lq = max(np.linalg.norm(S[4:7]) / M, np.linalg.norm(S[13:22]) / (M * L))
    return dict(M=M, L=L, Lq=Lq, Uv=Uv)


# ---- data sets of the reduction tests -------------------------------------------------------------------------------------------------------

def reference_pose(n, seed):
    """q: magnitudes in [3.5, 4], random signs (no entry near zero: every x q^T term of the benign set is large)"""
    rng = np.random.default_rng(seed + 7)
    return (rng.uniform(3.5, 4.0, size=(n, 3)) * rng.choice([-1.0, 1.0], size=(n, 3))).astype(np.float32)


def benign_rows(n, seed):
    """-> x, v, w. w in [0.5, 2], coordinates and velocities in [-4, 4], shaped so that NO particle's contribution to any slot is small:
    |x| in [3.5, 4] per component, |v| = ([3.2, 4], [0.25, 0.3], [1, 1.2]) -- the three cross-product components x_a v_b - x_b v_a then
    never cancel below 0.55 of their larger product."""
    rng = np.random.default_rng(seed)
    sign = lambda: rng.choice([-1.0, 1.0], size=(n, 3))       # noqa: E731
    x = (rng.uniform(3.5, 4.0, size=(n, 3)) * sign()).astype(np.float32)
    mag = np.stack([rng.uniform(3.2, 4.0, n), rng.uniform(0.25, 0.3, n), rng.uniform(1.0, 1.2, n)], axis=1)
    v = (mag * sign()).astype(np.float32)
    w = rng.uniform(0.5, 2.0, n).astype(np.float32)
    return x, v, w


def hostile_rows(n, seed):
    """-> x, v, w. w over 2^+-100 with subnormal inverse masses among them and w = 0 in about 1/7 of the rows; coordinates and velocities
    over 2^+-20 in both signs, -0 and +0 among them; the pinned rows carry NaN and infinities, which must not reach any sum."""
    rng = np.random.default_rng(seed + 1)

    def spread(shape):
        a = np.ldexp(rng.uniform(1.0, 2.0, size=shape), rng.integers(-20, 21, size=shape)) * rng.choice([-1.0, 1.0], size=shape)
        z = rng.random(size=shape)
        a = np.where(z < 0.03, -0.0, np.where(z < 0.06, 0.0, a))
        return a.astype(np.float32)
    x, v = spread((n, 3)), spread((n, 3))
    w = np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-100, 101, n)).astype(np.float32)
    sub = rng.random(n) < 0.1
    w[sub] = np.ldexp(rng.uniform(1.0, 2.0, int(sub.sum())), rng.integers(-148, -126, int(sub.sum()))).astype(np.float32)
    pinned = rng.random(n) < 1.0 / 7.0
    w[pinned] = 0.0
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    k = int(pinned.sum())
    x[pinned] = bad[rng.integers(0, 3, size=(k, 3))]
    v[pinned] = bad[rng.integers(0, 3, size=(k, 3))]
    return x, v, w
