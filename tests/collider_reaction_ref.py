"""Reference for what the body gives back to each collider (SPEC.md 2g; sb_group_collide_reactions / sb_group_get_collider_reactions), shared
by tests/test_collider_reactions.py, tests/test_gpu_collider_reactions.py and tests/collider_reaction_group_case.py.

The state comes from tests/collider_ref.py, one collider at a time with a snapshot of x and v around each, so the bits of x and v are that
module's. The sums and, per sum, A -- the sum of the absolute values of every elementary product -- are taken in np.longdouble (64-bit
mantissa on x86: the reference's own error is n 2^-63 A, 2^-11 of the bound it checks), as tests/body_state_ref.py takes its sums."""
import numpy as np

import collider_ref

LD = np.longdouble
NAMES = ("impulse x", "impulse y", "impulse z", "angular impulse x", "angular impulse y", "angular impulse z", "contact mass")


def longdouble_is_extended():
    return np.finfo(LD).nmant == 63


def apply(x, v, w, colliders, owned=None):
    """collider_ref.apply on x, v (changed in place), collider after collider; -> hits (len(colliders), n) and one dict per collider:
    sums (7, longdouble: impulse xyz, angular impulse xyz about the collider's a, contact mass), A (7) and n_contacts, over the particles
    the collider hit -- those of them `owned` (a bool mask) marks, if given."""
    hits = np.zeros((len(colliders), x.shape[0]), bool)
    out = []
    for k, col in enumerate(colliders):
        vb = v.copy()
        hit = collider_ref.apply(x, v, w, [col])[0]
        hits[k] = hit
        sel = hit if owned is None else hit & owned
        out.append(_sums(col, x[sel], vb[sel], v[sel], w[sel]))
    return hits, out


def _sums(col, xa, vb, va, w):
    """xa: the positions the collider left (x'), vb / va: the velocities before / after it (equal bits where it did not write), float32"""
    with np.errstate(all="ignore"):
        m = LD(1) / w.astype(LD)
        p32 = [xa[:, c] - col["a"][c] for c in range(3)]           # binary32, SPEC.md 2f's own p
        assert all(q.dtype == np.float32 for q in p32)
        p = [q.astype(LD) for q in p32]
        VB, VA = vb.astype(LD), va.astype(LD)
        j = [m * (VB[:, c] - VA[:, c]) for c in range(3)]
        aj = [m * (np.abs(VB[:, c]) + np.abs(VA[:, c])) for c in range(3)]
        sums = np.zeros(7, LD); A = np.zeros(7, LD)
        for c in range(3):
            sums[c] = j[c].sum()
            A[c] = aj[c].sum()
        for c, (a, b) in enumerate(((1, 2), (2, 0), (0, 1))):
            sums[3 + c] = (p[a] * j[b] - p[b] * j[a]).sum()
            A[3 + c] = (np.abs(p[a]) * aj[b] + np.abs(p[b]) * aj[a]).sum()
        sums[6] = A[6] = m.sum()
    return dict(sums=sums, A=A, n_contacts=int(w.shape[0]))


def bound(ref):
    """SPEC.md 2g, binding: |sum - exact| <= (n_contacts + 16) 2^-52 A"""
    return LD(ref["n_contacts"] + 16) * LD(2.0 ** -52) * ref["A"]


def record_sums(rec):
    """the 7 doubles of a fetched record (an element of SoftbodyGroup.collider_reactions())"""
    return np.concatenate([np.asarray(rec["impulse"], np.float64), np.asarray(rec["angular_impulse"], np.float64), [np.float64(rec["contact_mass"])]])


def _class(t):
    return "nan" if np.isnan(t) else "+inf" if t == np.inf else "-inf" if t == -np.inf else "finite"


def check(rec, ref):
    """-> list of complaints about one fetched record: a wrong count, a sum outside the bound, a non-finite sum of another class"""
    why = []
    if int(rec["n_contacts"]) != ref["n_contacts"]:
        why.append(f"n_contacts {int(rec['n_contacts'])} for {ref['n_contacts']}")
    got = record_sums(rec)
    b = bound(ref)
    for k in range(7):
        want = ref["sums"][k]
        if not np.isfinite(want):
            if _class(got[k]) != _class(want):
                why.append(f"{NAMES[k]}: {got[k]!r} where the reference is {_class(want)}")
            continue
        err = abs(LD(got[k]) - want)
        if not err <= b[k]:
            why.append(f"{NAMES[k]}: {got[k]!r} for {want!r}, off by {float(err):.3e}, bound {float(b[k]):.3e}")
    return why


def worst_ratio(rec, ref):
    """max over the finite sums of error / bound (0 where the bound is 0 and the sum exact): the figure a test prints"""
    got = record_sums(rec); b = bound(ref); worst = 0.0
    for k in range(7):
        if not np.isfinite(ref["sums"][k]):
            continue
        err = abs(LD(got[k]) - ref["sums"][k])
        if b[k] > 0:
            worst = max(worst, float(err / b[k]))
        elif err != 0:
            worst = float("inf")
    return worst


def total(refs):
    """the reference of a whole list taken as one: sums, A and counts added up (for momentum balances)"""
    return dict(sums=sum(r["sums"] for r in refs), A=sum(r["A"] for r in refs), n_contacts=sum(r["n_contacts"] for r in refs))
