"""Collider contacts between two ticks (SPEC.md 2f), without a GPU: the struct's layout, what sb_group_collide refuses before it touches a
group, known answers and properties of the reference the GPU tests compare against (tests/collider_ref.py), and the branches the module's
random inputs reach."""
import ctypes as C
import os
import subprocess

import numpy as np

import collider_ref
import placement_ref
from collider_ref import bits
from softbodyunity_amd import box_collider, capsule_collider, native, sphere_collider

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

FLOAT_FIELDS = [("a", 3), ("b", 3), ("rot", 9), ("half", 3), ("radius", 0), ("lin", 3), ("ang", 3), ("friction", 0), ("restitution", 0)]


def _good():
    return sphere_collider((1, 2, 3), 0.5, friction=0.5, restitution=0.25)


def _set(c, name, k, val):
    if dict(FLOAT_FIELDS)[name]:
        getattr(c, name)[k] = val
    else:
        setattr(c, name, val)


def bad_colliders():
    """(collider, the word sb_last_error must hold) for everything SPEC.md 2f refuses in a record itself"""
    rows = []
    for name, count in FLOAT_FIELDS:
        for k in sorted({0, max(0, count - 1)}):
            for val in (np.nan, np.inf, -np.inf):
                c = _good(); _set(c, name, k, val)
                rows.append((c, "NaN or infinite"))
    for shape in (3, 0xffffffff):
        c = _good(); c.shape = shape
        rows.append((c, "unknown shape"))
    for flags in (1, 0x80000000):
        c = _good(); c.flags = flags
        rows.append((c, "flags"))
    for k in range(3):
        c = _good(); c.reserved[k] = -1 if k == 1 else 1
        rows.append((c, "reserved"))
    c = _good(); c.radius = -1e-30
    rows.append((c, "negative radius"))
    for k in range(3):
        c = box_collider((0, 0, 0), (1, 1, 1)); c.half[k] = -0.5
        rows.append((c, "negative half"))
    c = _good(); c.friction = -0.125
    rows.append((c, "negative friction"))
    for r in (-0.125, 1.0 + 2.0 ** -23):
        c = _good(); c.restitution = r
        rows.append((c, "restitution"))
    return rows


def _list(*items):
    return (native.SbCollider * len(items))(*items)


def test_the_struct_is_128_bytes_in_the_header_and_in_ctypes(tmp_path):
    names = ["shape", "flags", "a", "b", "rot", "half", "radius", "lin", "ang", "friction", "restitution", "reserved"]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "softbody_group.h"\nint main(void){printf("%zu", sizeof(sb_collider));\n'
                   + "".join(f'printf(" %zu", offsetof(sb_collider, {n}));\n' for n in names) + 'printf(" %u %u %u\\n", SB_COLLIDER_SPHERE, '
                   'SB_COLLIDER_CAPSULE, SB_COLLIDER_BOX); return 0;}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    K = native.SbCollider
    assert got[:13] == [C.sizeof(K)] + [getattr(K, n).offset for n in names] == [128, 0, 4, 8, 20, 32, 68, 80, 84, 96, 108, 112, 116]
    assert got[13:] == [native.SB_COLLIDER_SPHERE, native.SB_COLLIDER_CAPSULE, native.SB_COLLIDER_BOX] == [collider_ref.SPHERE, collider_ref.CAPSULE, collider_ref.BOX] == [0, 1, 2]


def test_null_arguments_and_bad_lists_are_refused_before_the_group_is_touched():
    L = native.lib()
    good = _list(_good())
    assert L.sb_group_collide(None, good, 1) == native.SB_ERR_INVALID_ARG and b"null group" in L.sb_last_error()
    assert L.sb_group_collide(None, None, 0) == native.SB_ERR_INVALID_ARG
    # the list's checks come before the group is looked at: a handle that is no group at all is never read
    no_group = C.create_string_buffer(64)
    h = C.cast(no_group, C.c_void_p)
    assert L.sb_group_collide(h, None, 1) == native.SB_ERR_INVALID_ARG and b"null colliders" in L.sb_last_error()
    assert L.sb_group_collide(h, good, -1) == native.SB_ERR_INVALID_ARG and b"negative count" in L.sb_last_error()
    assert L.sb_group_collide(h, None, -1) == native.SB_ERR_INVALID_ARG
    rows = bad_colliders()
    assert len(rows) == (6 * 2 + 3) * 3 + 2 + 2 + 3 + 1 + 3 + 1 + 2
    for c, word in rows:
        for items, where in ((_list(c), "collider 0"), (_list(_good(), _good(), c), "collider 2")):
            assert L.sb_group_collide(h, items, len(items)) == native.SB_ERR_INVALID_ARG
            err = L.sb_last_error().decode()
            assert word in err and where in err and "sb_group_collide" in err, (word, err)
    assert no_group.raw == bytes(64)


def test_the_makers_fill_the_struct():
    c = sphere_collider((1, 2, 3), 0.5, lin=(4, 5, 6), ang=(7, 8, 9), friction=0.25, restitution=0.75)
    assert (c.shape, c.flags, list(c.reserved)) == (0, 0, [0, 0, 0]) and list(c.a) == [1, 2, 3] and c.radius == 0.5
    assert list(c.lin) == [4, 5, 6] and list(c.ang) == [7, 8, 9] and (c.friction, c.restitution) == (0.25, 0.75)
    c = capsule_collider((1, 2, 3), (4, 5, 6), 2.0)
    assert c.shape == 1 and list(c.a) + list(c.b) == [1, 2, 3, 4, 5, 6] and c.radius == 2.0
    c = box_collider((1, 2, 3), (4, 5, 6))
    assert c.shape == 2 and list(c.half) == [4, 5, 6] and list(c.rot) == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    assert list(box_collider((0, 0, 0), (1, 1, 1), rot=np.arange(9).reshape(3, 3)).rot) == list(range(9))
    col = collider_ref.box((1, 2, 3), placement_ref.rotation((0.3, -0.5, 0.2, 0.7)), (1, 2, 3), lin=(1, 0, 0), ang=(0, 1, 0), friction=0.5, restitution=0.5)
    n = collider_ref.to_native(col)
    assert np.array_equal(bits(np.array(n.rot[:], np.float32)), bits(col["rot"])) and n.shape == 2 and n.friction == 0.5


# ---- known answers ---------------------------------------------------------------------------------------------------------------------------

def _one(x, v, colliders, w=1.0):
    x, v = np.array([x], np.float32), np.array([v], np.float32)
    hits = collider_ref.apply(x, v, np.array([w], np.float32), colliders)
    return x[0], v[0], hits[:, 0]


def test_a_particle_at_the_centre_of_a_sphere_goes_up():
    a = np.float32([0.3, -1.7, 2.9])
    x, v, hit = _one(a, (0, 0, 0), [collider_ref.sphere(a, 0.75)])
    assert hit[0] and np.array_equal(bits(x), bits(a + np.float32([0, 0.75, 0]))) and a[1] + F(0.75) == x[1]


def test_a_bouncing_wall_negates_the_normal_velocity_exactly():
    wall = collider_ref.box((0, 0, 0), np.eye(3), (1, 2, 3), friction=0.0, restitution=1.0)
    x, v, hit = _one((0.9, 0.3, -0.2), (-0.7, 0.31, 0.43), [wall])        # leaves through the +x face, moving into it
    assert hit[0] and np.array_equal(bits(x), bits(np.float32([1.0, 0.3, -0.2])))
    assert np.array_equal(bits(v), bits(np.float32([0.7, 0.31, 0.43]))), v


def test_a_sticking_particle_takes_the_colliders_velocity_bit_for_bit():
    col = collider_ref.sphere((0, 0, 0), 1.0, lin=(0.3, -0.2, 0.1), ang=(0.5, 1.5, -0.25), friction=1e6, restitution=0.0)
    x0 = np.float32([0.1, 0.6, -0.3])
    x, v, hit = _one(x0, (0.2, -3.0, 0.4), [col])
    assert hit[0] and not np.array_equal(bits(x), bits(x0))
    p = x - col["a"]
    cr = np.float32([col["ang"][1] * p[2] - col["ang"][2] * p[1], col["ang"][2] * p[0] - col["ang"][0] * p[2], col["ang"][0] * p[1] - col["ang"][1] * p[0]])
    assert np.array_equal(bits(v), bits(col["lin"] + cr)), (v, col["lin"] + cr)


def test_a_separating_particle_keeps_its_velocity_but_not_its_position():
    col = collider_ref.sphere((0, 0, 0), 1.0, friction=0.5, restitution=0.5)
    v0 = np.array([0.3, 0.9, -0.1], np.float32)
    v0.view(np.uint32)[2] = 0x80000001        # a subnormal: any arithmetic on it would show
    x, v, hit = _one((0.1, 0.6, -0.3), v0, [col])
    assert hit[0] and np.array_equal(bits(v), bits(v0)) and abs(float(np.linalg.norm(x.astype(np.float64))) - 1) < 1e-6


def test_a_capsule_of_no_length_is_the_sphere():
    rng = np.random.default_rng(3)
    n = 4000
    x = rng.uniform(-1.5, 1.5, size=(n, 3)).astype(np.float32)
    v = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    w = np.ones(n, np.float32)
    a = (0.25, -0.5, 0.125)
    kw = dict(lin=(0.1, 0.2, -0.3), ang=(0.3, -0.1, 0.2), friction=0.4, restitution=0.3)
    xs, vs, xc, vc = x.copy(), v.copy(), x.copy(), v.copy()
    hs = collider_ref.apply(xs, vs, w, [collider_ref.sphere(a, 1.25, **kw)])
    hc = collider_ref.apply(xc, vc, w, [collider_ref.capsule(a, a, 1.25, **kw)])
    assert hs.sum() > 1000 and np.array_equal(hs, hc) and np.array_equal(bits(xs), bits(xc)) and np.array_equal(bits(vs), bits(vc))


def test_pinned_and_untouched_particles_keep_every_bit_and_an_empty_list_is_the_identity():
    pool = np.array([0x80000000, 0x00000001, 0x7fc12345, 0xffc00001, 0x7f800001, 0x7f800000, 0xff800000, 0x3f000000], np.uint32)
    x = np.zeros((8, 3), np.float32); v = np.zeros((8, 3), np.float32)
    for c in range(3):
        x.view(np.uint32)[:, c] = np.roll(pool, c); v.view(np.uint32)[:, c] = np.roll(pool, c + 3)
    x[7] = (0.1, 0.2, 0.3)                                  # inside, pinned
    w = np.float32([1, 1, 1, 1, 1, 1, 1, 0])
    x0, v0 = x.copy(), v.copy()
    assert collider_ref.apply(x, v, w, []).shape == (0, 8) and np.array_equal(bits(x), bits(x0)) and np.array_equal(bits(v), bits(v0))
    cols = [collider_ref.sphere((0, 0, 0), 10.0), collider_ref.capsule((0, 0, 0), (1, 0, 0), 10.0), collider_ref.box((0, 0, 0), np.eye(3), (9, 9, 9))]
    hits = collider_ref.apply(x, v, w, cols)
    assert not hits[:, 7].any() and np.array_equal(bits(x[7]), bits(x0[7])) and np.array_equal(bits(v[7]), bits(v0[7]))
    untouched = ~hits.any(axis=0)
    assert untouched.sum() >= 6, "NaN and infinite positions are never hit"
    assert np.array_equal(bits(x[untouched]), bits(x0[untouched])) and np.array_equal(bits(v[untouched]), bits(v0[untouched]))


# ---- properties of the reference on random contacts ------------------------------------------------------------------------------------------

N_CLOUD = 200_000
TILT = placement_ref.rotation((0.3, -0.5, 0.2, 0.7))
STATIC = {
    "sphere": collider_ref.sphere((0.25, -0.5, 0.125), 1.5, friction=0.3, restitution=0.5),
    "capsule": collider_ref.capsule((-0.75, -0.5, 0.25), (0.5, 0.75, -0.25), 1.0, friction=0.3, restitution=0.5),
    "box": collider_ref.box((0.25, -0.5, 0.125), TILT, (1.25, 0.75, 1.0), friction=0.3, restitution=0.5),
}


def _cloud(seed, n=N_CLOUD):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2.5, 2.5, size=(n, 3)).astype(np.float32)
    v = rng.uniform(-2, 2, size=(n, 3)).astype(np.float32)
    w = rng.choice(np.float32([0.5, 1, 2]), size=n).astype(np.float32)
    w[::7] = 0
    return x, v, w


def _surface_error(name, col, x):
    """| distance / radius - 1 | (sphere, capsule) or | |q_k| / half_k - 1 | on the nearest face (box), in binary64, of points x (m, 3)"""
    x = x.astype(np.float64)
    a = col["a"].astype(np.float64)
    if name == "box":
        q = (x - a) @ col["rot"].astype(np.float64).reshape(3, 3).T
        return np.abs(np.abs(q) / col["half"].astype(np.float64) - 1).min(axis=1)
    if name == "capsule":
        ab = col["b"].astype(np.float64) - a
        t = np.clip(((x - a) @ ab) / (ab @ ab), 0, 1)
        a = a + t[:, None] * ab
    return np.abs(np.linalg.norm(x - a, axis=1) / float(col["radius"]) - 1)


def _normal(name, col, x0, x1):
    """the outward unit normal in binary64 at the particles x0 that were pushed to x1: from the geometry for the round shapes, the row of rot
    nearest the push for the box; `ok` leaves out what has no normal to speak of in binary64 (the centre, a push shorter than 1e-4)"""
    x0, d = x0.astype(np.float64), x1.astype(np.float64) - x0.astype(np.float64)
    a = col["a"].astype(np.float64)
    ok = np.linalg.norm(d, axis=1) > 1e-4
    if name == "box":
        R = col["rot"].astype(np.float64).reshape(3, 3)
        p = d @ R.T
        k = np.abs(p).argmax(axis=1)
        return R[k] * np.sign(p[np.arange(len(k)), k])[:, None], ok
    if name == "capsule":
        ab = col["b"].astype(np.float64) - a
        t = np.clip(((x0 - a) @ ab) / (ab @ ab), 0, 1)
        a = a + t[:, None] * ab
    r = np.linalg.norm(x0 - a, axis=1, keepdims=True)
    return (x0 - a) / np.where(r > 0, r, 1), ok & (r[:, 0] > 1e-4)


# Worst cases of collider_ref measured here on the CPU over the 200 000 particles of _cloud(11) (10 000 to 19 000 contacts a shape) with
# (friction, restitution) = (0.3, 0.5), (0, 1) -- nothing dissipates: the energy shows the rounding -- and (0.3, 0) -- the normal velocity
# is zeroed: it shows the rounding --; each bound is twice the largest of its row.
#   surface: | r' / radius - 1 |, box | |q'| / half - 1 |       sphere 1.612e-7    capsule 1.791e-7    box 2.199e-7
#   normal velocity after the call, -un' / |v|                  sphere 1.516e-7    capsule 1.033e-6    box 8.390e-8
#   (the capsule's normal is taken about the binary64 axis point here, the reference's about its binary32 one: that difference is in its figure)
#   kinetic energy, E' / E - 1                                  sphere 1.062e-6    capsule 8.007e-7    box 6.649e-7
SURFACE_TOL = 2 * 2.199e-7
NORMAL_TOL = 2 * 1.033e-6
ENERGY_TOL = 2 * 1.062e-6
MEASURED = {}


def test_pushed_particles_sit_on_the_surface_do_not_approach_and_gain_no_energy():
    x0, v0, w = _cloud(11)
    for name, base in STATIC.items():
        worst = np.zeros(3)
        for friction, restitution in ((0.3, 0.5), (0.0, 1.0), (0.3, 0.0)):
            col = dict(base, friction=F(friction), restitution=F(restitution))
            x, v = x0.copy(), v0.copy()
            hit = collider_ref.apply(x, v, w, [col])[0]
            assert hit.sum() > 10_000 and not hit[w == 0].any()
            assert np.array_equal(bits(x[~hit]), bits(x0[~hit])) and np.array_equal(bits(v[~hit]), bits(v0[~hit]))
            surf = _surface_error(name, col, x[hit])
            n, ok = _normal(name, col, x0[hit], x[hit])
            assert ok.sum() > 0.99 * hit.sum()
            speed = np.linalg.norm(v0[hit].astype(np.float64), axis=1)
            un = (v[hit].astype(np.float64) * n).sum(axis=1)
            e0 = (v0[hit].astype(np.float64) ** 2).sum(axis=1)
            e1 = (v[hit].astype(np.float64) ** 2).sum(axis=1)
            worst = np.maximum(worst, [surf.max(), (-un / speed)[ok].max(), (e1 / e0 - 1).max()])
            print("%s, friction %.1f, restitution %.1f: %d contacts: surface %.3e, normal velocity %.3e, energy %.3e"
                  % (name, friction, restitution, hit.sum(), surf.max(), (-un / speed)[ok].max(), (e1 / e0 - 1).max()))
            assert surf.max() <= SURFACE_TOL
            assert (un[ok] >= -NORMAL_TOL * speed[ok]).all()
            assert (e1 <= e0 * (1 + ENERGY_TOL)).all()
            # a second call finds far fewer left to push: the particles are on the surface, to a rounding
            assert collider_ref.apply(x.copy(), v.copy(), w, [col])[0].sum() < 0.6 * hit.sum()
        MEASURED[name] = worst
    print({k: ["%.3e" % t for t in m] for k, m in MEASURED.items()})


def test_the_random_inputs_reach_every_branch():
    x, v, w = _cloud(12, 60_000)
    rng = np.random.default_rng(13)
    aligned = collider_ref.box((-1.0, 1.0, 0.5), np.eye(3), (1.0, 1.0, 1.0), lin=(0.1, 0, 0), friction=0.2, restitution=0.1)
    moving = collider_ref.sphere((1.0, 1.0, -1.0), 1.25, lin=(0.5, -0.25, 0.0), ang=(0.0, 1.0, 0.5), friction=0.0, restitution=1.0)
    sticky = collider_ref.capsule((-1.5, -1.5, -1.5), (-0.5, -1.0, -1.5), 0.75, friction=50.0, restitution=0.0)
    # random particles snapped onto the places a uniform cloud has measure zero at: the sphere's centre, the aligned box's diagonal planes
    free = np.nonzero(w > 0)[0]
    x[free[:40]] = STATIC["sphere"]["a"]
    s = (np.round(rng.uniform(-0.9, 0.9, size=(200, 1)) * 1024) / 1024).astype(np.float32)      # ten fractional bits: a + e and (a + e) - a are exact
    e = np.repeat(s, 3, axis=1); e[:, 2] = np.float32(1 / 64)     # |q0| == |q1| exactly, and face 2 is farther away
    x[free[40:240]] = aligned["a"] + e * np.float32([1, -1, 1])
    trace = collider_ref.new_trace()
    hits = collider_ref.apply(x, v, w, [aligned, STATIC["sphere"], STATIC["capsule"], STATIC["box"], moving, sticky], trace)
    print(trace)
    assert all(trace[k] > 0 for k in collider_ref.TRACE_KEYS), trace
    assert hits.any(axis=1).all() and trace["sphere_centre"] >= 30 and trace["box_tie"] >= 20
