"""What the body gives back to each collider (SPEC.md 2g), without a GPU: the record's layout, what sb_group_collide_reactions and
sb_group_get_collider_reactions refuse before they touch a group, a known answer that is exact in binary64, and properties of the reference
the GPU tests compare against (tests/collider_reaction_ref.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

import collider_reaction_ref as rref
import collider_ref
from softbodyunity_amd import SoftbodyGroup, native, sphere_collider
from test_colliders import bad_colliders

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def _list(*items):
    return (native.SbCollider * len(items))(*items)


def _good():
    return sphere_collider((1, 2, 3), 0.5, friction=0.5, restitution=0.25)


def test_the_record_is_64_bytes_in_the_header_and_in_ctypes(tmp_path):
    names = ["impulse", "angular_impulse", "contact_mass", "n_contacts"]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "softbody_group.h"\nint main(void){printf("%zu", sizeof(sb_collider_reaction));\n'
                   + "".join(f'printf(" %zu", offsetof(sb_collider_reaction, {n}));\n' for n in names) + 'printf(" %d\\n", SB_COLLIDE_REACTIONS_MAX); return 0;}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    K = native.SbColliderReaction
    assert got[:5] == [C.sizeof(K)] + [getattr(K, n).offset for n in names] == [64, 0, 24, 48, 56]
    assert got[5] == native.SB_COLLIDE_REACTIONS_MAX == 1024
    D = SoftbodyGroup.REACTION_DTYPE
    assert D.itemsize == 64 and [D.fields[n][1] for n in names] == [0, 24, 48, 56]


def test_null_arguments_and_bad_lists_are_refused_before_the_group_is_touched():
    L = native.lib()
    good = _list(_good())
    assert L.sb_group_collide_reactions(None, good, 1) == native.SB_ERR_INVALID_ARG and b"null group" in L.sb_last_error()
    assert L.sb_group_collide_reactions(None, None, 0) == native.SB_ERR_INVALID_ARG
    # the list's checks come before the group is looked at: a handle that is no group at all is never read
    no_group = C.create_string_buffer(64)
    h = C.cast(no_group, C.c_void_p)
    assert L.sb_group_collide_reactions(h, None, 1) == native.SB_ERR_INVALID_ARG and b"null colliders" in L.sb_last_error()
    assert L.sb_group_collide_reactions(h, good, -1) == native.SB_ERR_INVALID_ARG and b"negative count" in L.sb_last_error()
    for c, word in bad_colliders():
        for items, where in ((_list(c), "collider 0"), (_list(_good(), _good(), c), "collider 2")):
            assert L.sb_group_collide_reactions(h, items, len(items)) == native.SB_ERR_INVALID_ARG
            err = L.sb_last_error().decode()
            assert word in err and where in err and "sb_group_collide_reactions" in err, (word, err)
    # one collider too many: a list of good records that is longer than the result can hold
    many = _list(*[_good()] * (native.SB_COLLIDE_REACTIONS_MAX + 1))
    assert L.sb_group_collide_reactions(h, many, len(many)) == native.SB_ERR_INVALID_ARG and b"SB_COLLIDE_REACTIONS_MAX" in L.sb_last_error()
    # the fetch
    out = (native.SbColliderReaction * 2)()
    n = C.c_int32(-7)
    assert L.sb_group_get_collider_reactions(None, out, 2, C.byref(n)) == native.SB_ERR_INVALID_ARG
    assert L.sb_group_get_collider_reactions(h, out, 2, None) == native.SB_ERR_INVALID_ARG
    assert L.sb_group_get_collider_reactions(h, out, -1, C.byref(n)) == native.SB_ERR_INVALID_ARG and b"capacity" in L.sb_last_error()
    assert L.sb_group_get_collider_reactions(h, None, 1, C.byref(n)) == native.SB_ERR_INVALID_ARG and b"null out" in L.sb_last_error()
    assert n.value == -7 and no_group.raw == bytes(64) and bytes(out) == bytes(128)


def test_a_known_answer_exact_in_binary64():
    """one particle of mass 2 inside a static unit box, 0.25 under its top face, falling at 3: restitution 0.5 sends it back up at 1.5"""
    x, v, w = np.float32([[0.25, 0.75, 0.0]]), np.float32([[0.0, -3.0, 0.0]]), np.float32([0.5])
    box = collider_ref.box((0, 0, 0), np.eye(3), (1, 1, 1), friction=0.0, restitution=0.5)
    hits, (r,) = rref.apply(x, v, w, [box])
    assert hits.tolist() == [[True]] and x.tolist() == [[0.25, 1.0, 0.0]] and v.tolist() == [[0.0, 1.5, 0.0]]
    assert [float(t) for t in r["sums"]] == [0.0, -9.0, 0.0, 0.0, 0.0, -2.25, 2.0] and r["n_contacts"] == 1
    assert [float(t) for t in r["A"]] == [0.0, 9.0, 0.0, 0.0, 0.0, 2.25, 2.0]
    arr = np.zeros(1, SoftbodyGroup.REACTION_DTYPE)
    arr["impulse"][0] = (0, -9, 0); arr["angular_impulse"][0] = (0, 0, -2.25); arr["contact_mass"][0] = 2; arr["n_contacts"][0] = 1
    assert rref.check(arr[0], r) == [] and rref.worst_ratio(arr[0], r) == 0.0
    arr["angular_impulse"][0, 2] = np.nextafter(-2.25, 0)       # one ulp off: (1 + 16) 2^-52 2.25 allows it
    assert rref.check(arr[0], r) == []
    arr["n_contacts"][0] = 2                                     # counts are exact
    assert len(rref.check(arr[0], r)) == 1
    arr["n_contacts"][0] = 1; arr["impulse"][0, 1] = -9.0 - 2.0 ** -40
    why = rref.check(arr[0], r)
    assert len(why) == 1 and "impulse y" in why[0]


N = 200_000


def _cloud(seed, pinned=False):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-4, 4, size=(N, 3)).astype(np.float32)
    v = rng.uniform(-2, 2, size=(N, 3)).astype(np.float32)
    w = rng.choice(np.float32([0.5, 1, 2, 0.3]), size=N).astype(np.float32)
    if pinned:
        w[::5] = 0
    return x, v, w


def test_the_reference_balances_the_bodys_momentum():
    """without pinned particles, what the list takes from sum m v is what it reports, collider by collider"""
    assert rref.longdouble_is_extended()
    x, v, w = _cloud(5)
    m = LD(1) / w.astype(LD)
    cols = [collider_ref.sphere((0.5, 0, 0), 2.0, lin=(1, 0.5, 0), ang=(0, 1, 0), friction=0.4, restitution=0.3),
            collider_ref.box((-1, 1, 0), np.eye(3), (2, 1, 2.5), lin=(0, -1, 0), friction=0.8, restitution=0.0),
            collider_ref.capsule((-3, -2, 0), (3, -2.5, 1), 1.25, friction=0.0, restitution=1.0)]
    before = (m[:, None] * v.astype(LD)).sum(axis=0)
    hits, refs = rref.apply(x, v, w, cols)
    after = (m[:, None] * v.astype(LD)).sum(axis=0)
    tot = rref.total(refs)
    assert all(r["n_contacts"] > 1000 for r in refs) and (hits.sum(axis=0) > 1).any()
    # both sides carry the reference's own rounding: n 2^-63 of the absolute sums (the momentum's is at most sum m |v| on either side)
    slack = LD(N) * LD(2.0 ** -62) * ((m[:, None] * np.abs(v.astype(LD))).sum(axis=0) + tot["A"][:3])
    assert (np.abs((before - after) - tot["sums"][:3]) <= slack).all()
    assert (np.abs(tot["sums"][:3]) > 100 * rref.bound(tot)[:3]).all(), "the balance is about something"


def test_a_static_frictionless_sphere_takes_no_torque_about_its_centre():
    """p is parallel to n and so is the velocity change, so each particle's p x m dv is zero in exact arithmetic. The STATE is binary32,
    though: x' = x + depth n, n = d / r and v' each carry roundings of 2^-24 of their operands, so a particle's p and dv are parallel only to
    about 2^-22 (eight such roundings, |x'| up to 2.8 |p| here) and its cross product is that fraction of its elementary products: the sum
    is zero within 2^-21 A, not within the summation bound (n + 16) 2^-52 A of SPEC.md 2g, which speaks of the additions and not of the
    state. Measured on this cloud (20 450 contacts): |torque| = 4.6e-6, 1.3e-5, 9.1e-6 with A = 1.7e5 each, which is 2.7e-11 .. 8.0e-11 A
    (the roundings cancel at random), against a summation bound of 7.7e-7; the same sphere with friction 0.5 takes 2.1e-4 .. 5.7e-4 A."""
    x, v, w = _cloud(6, pinned=True)
    ball = collider_ref.sphere((0.25, -0.5, 0.125), 2.5, friction=0.0, restitution=0.5)
    hits, (r,) = rref.apply(x, v, w, [ball])
    assert r["n_contacts"] == hits.sum() > 10_000 and not hits[0, w == 0].any()
    assert (np.abs(r["sums"][:3]) > 1.0).any()
    print("frictionless sphere: |torque| / A =", [float(abs(r["sums"][k]) / r["A"][k]) for k in (3, 4, 5)], "summation bound / A =", float(rref.bound(r)[3] / r["A"][3]))
    assert (np.abs(r["sums"][3:6]) <= LD(2.0 ** -21) * r["A"][3:6]).all()
    rough = collider_ref.sphere((0.25, -0.5, 0.125), 2.5, friction=0.5, restitution=0.5)
    x, v, w = _cloud(6, pinned=True)
    _, (q,) = rref.apply(x, v, w, [rough])
    assert (np.abs(q["sums"][3:6]) > LD(2.0 ** -13) * q["A"][3:6]).all(), "friction turns the sphere: 2^8 times the frictionless tolerance"


def test_a_list_that_touches_nothing_gives_zeros_and_a_separating_contact_counts_without_an_impulse():
    x, v, w = _cloud(7)
    x0, v0 = x.copy(), v.copy()
    hits, refs = rref.apply(x, v, w, [collider_ref.sphere((100, 100, 100), 1.0), collider_ref.box((0, -50, 0), np.eye(3), (3, 3, 3))])
    assert not hits.any() and np.array_equal(x, x0) and np.array_equal(v, v0)
    for r in refs:
        assert r["n_contacts"] == 0 and not r["sums"].any() and not r["A"].any()
    # every particle flies away from the centre faster than the sphere's surface could follow: hit, pushed out, velocity kept
    v[:] = x * np.float32(2.0)
    v0 = v.copy()
    hits, (r,) = rref.apply(x, v, w, [collider_ref.sphere((0, 0, 0), 3.0, friction=0.5, restitution=0.5)])
    assert hits.sum() > 10_000 and np.array_equal(collider_ref.bits(v), collider_ref.bits(v0)) and not np.array_equal(x, x0)
    assert r["n_contacts"] == hits.sum() and float(r["sums"][6]) > 10_000 * 0.5
    assert not r["sums"][:6].any(), "a separating contact adds exactly 0"
    # owners: a mask splits the counts and the sums
    own = np.arange(N) % 3 == 0
    x, v, w = _cloud(7)
    _, (a,) = rref.apply(x.copy(), v.copy(), w, [collider_ref.sphere((0, 0, 0), 3.0, friction=0.5)], owned=own)
    _, (b,) = rref.apply(x.copy(), v.copy(), w, [collider_ref.sphere((0, 0, 0), 3.0, friction=0.5)], owned=~own)
    _, (c,) = rref.apply(x.copy(), v.copy(), w, [collider_ref.sphere((0, 0, 0), 3.0, friction=0.5)])
    assert a["n_contacts"] + b["n_contacts"] == c["n_contacts"] and 0 < a["n_contacts"] < b["n_contacts"]
    assert (np.abs(a["sums"] + b["sums"] - c["sums"]) <= LD(N) * LD(2.0 ** -62) * c["A"]).all()
