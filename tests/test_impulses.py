"""Impulses between two ticks (SPEC.md 2c), without a GPU: known answers of the reference the GPU tests compare against (tests/impulse_ref.py),
with power-of-two weights, masses and barycentric coordinates so that every answer is exact; the expansion order of SURFACE items; the
record's layout and the constants in the header, the ctypes twin and the C# binding."""
import ctypes as C
import os
import re

import numpy as np

import impulse_ref
from impulse_ref import LINEAR_FALLOFF, VELOCITY_CHANGE, bits
from softbodyunity_amd import IMPULSE, impulse_explosion, impulse_hits, impulse_particles, native
from softbodyunity_amd.softbody import RAY_HIT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hit(triangle, u, v):
    h = np.zeros(1, RAY_HIT)
    h["triangle"], h["u"], h["v"] = triangle, u, v
    return h


def _state(n, w=None):
    x = (np.arange(3 * n, dtype=np.float32).reshape(n, 3) * np.float32(0.25))
    v = np.zeros((n, 3), np.float32)
    w = np.ones(n, np.float32) if w is None else np.asarray(w, np.float32)
    return x, v, w


def test_the_record_is_48_bytes_everywhere():
    assert C.sizeof(native.SbImpulse) == 48 and IMPULSE.itemsize == 48
    assert [IMPULSE.fields[name][1] for name in IMPULSE.names] == [getattr(native.SbImpulse, name).offset for name, _ in native.SbImpulse._fields_]
    assert [name for name, _ in native.SbImpulse._fields_] == list(IMPULSE.names)
    cs = open(os.path.join(ROOT, "csharp", "SoftbodyNative.cs")).read()
    body = re.search(r"public struct SbImpulse\s*\{(.*?)\}", cs, re.S).group(1)
    fields = re.findall(r"public (int|uint|float) ([^;]+);", body)
    assert sum(len(names.split(",")) for _, names in fields) == 12           # twelve 4-byte fields


def test_the_constants_agree_in_the_header_the_ctypes_twin_and_the_csharp_binding():
    hdr = open(os.path.join(ROOT, "include", "softbody.h")).read()
    cs = open(os.path.join(ROOT, "csharp", "SoftbodyNative.cs")).read()
    names = ("SB_IMPULSE_PARTICLE", "SB_IMPULSE_SURFACE", "SB_IMPULSE_RADIAL", "SB_IMPULSE_VELOCITY_CHANGE", "SB_IMPULSE_LINEAR_FALLOFF")
    want = (0, 1, 2, 1, 2)
    for name, value in zip(names, want):
        assert int(re.search(r"#define\s+%s\s+(\d+)u?\b" % name, hdr).group(1)) == value
        assert getattr(native, name) == value
        assert int(re.search(r"\b%s = (\d+)" % name, cs).group(1)) == value
    assert (impulse_ref.PARTICLE, impulse_ref.SURFACE, impulse_ref.RADIAL, VELOCITY_CHANGE, LINEAR_FALLOFF) == want


def test_particle_items_accumulate_in_order_and_skip_pins():
    x, v, w = _state(4, [0.5, 0.0, 4.0, 2.0])
    big, one = np.float32(2.0 ** 24), np.float32(1.0)
    items = [impulse_particles([0, 1, 2], (1, 2, 4)), impulse_particles([3, 3, 3], [(big, 0, 0), (one, 0, 0), (-big, 0, 0)], velocity_change=True),
             impulse_particles([1], (1, 1, 1), velocity_change=True)]
    impulse_ref.apply(x, v, w, np.concatenate(items))
    assert v[0].tolist() == [0.5, 1.0, 2.0] and v[2].tolist() == [4.0, 8.0, 16.0]
    assert not v[1].any()                                   # inverse mass 0: skipped, with and without VELOCITY_CHANGE
    assert v[3].tolist() == [0.0, 0.0, 0.0]                 # (2^24 + 1) - 2^24 in list order loses the 1: order matters and is kept
    v[:] = 0
    impulse_ref.apply(x, v, w, np.concatenate(items)[[0, 1, 2, 3, 5, 4, 6]])
    assert v[3].tolist() == [1.0, 0.0, 0.0]


def test_a_surface_item_delivers_its_impulse_in_both_render_modes():
    n = 8
    x, v, w = _state(n, [1, 2, 4, 0.5, 0.25, 8, 1, 2])
    tri = np.array([[0, 1, 2], [5, 3, 4]], np.int32)
    J = np.float32([2, -4, 8])
    # render triangles: sum of dv_p / w_p == J
    it = impulse_hits(_hit(1, 0.25, 0.5), J)
    impulse_ref.apply(x, v, w, it, tri=tri)
    assert np.array_equal((v / w[:, None]).sum(axis=0), J) and not v[[0, 1, 2, 6, 7]].any()
    assert np.array_equal(v[5], np.float32(0.25) * J * w[5]) and np.array_equal(v[3], np.float32(0.25) * J * w[3]) and np.array_equal(v[4], np.float32(0.5) * J * w[4])
    # VELOCITY_CHANGE ignores mass
    v[:] = 0
    impulse_ref.apply(x, v, w, impulse_hits(_hit(1, 0.25, 0.5), J, velocity_change=True), tri=tri)
    assert np.array_equal(v.sum(axis=0), J) and np.array_equal(v[3], np.float32(0.25) * J)
    # a miss is skipped
    before = v.copy()
    impulse_ref.apply(x, v, w, impulse_hits(_hit(-1, 0.25, 0.5), J), tri=tri)
    assert np.array_equal(bits(v), bits(before))
    # an embedding whose weights sum to one: the transpose of the skinning delivers J as well
    cage = np.array([[0, 1, 2, 3], [4, 5, 6, 7], [1, 3, 5, 7]], np.int32)
    w4 = np.float32([[0.5, 0.25, 0.125, 0.125], [0.25, 0.25, 0.25, 0.25], [1.0, 0.5, -0.25, -0.25]])
    etri = np.array([[2, 0, 1]], np.int32)
    v[:] = 0
    impulse_ref.apply(x, v, w, impulse_hits(_hit(0, 0.5, 0.25), J), tri=etri, cage=cage, w4=w4)
    assert np.array_equal((v / w[:, None]).sum(axis=0), J)


def test_the_expansion_order():
    J = np.float32([1, 2, 4])
    it = impulse_hits(_hit(1, 0.25, 0.5), J)[0]
    tri = np.array([[0, 1, 2], [5, 3, 4]], np.int32)
    ex = impulse_ref.expand_surface(it, tri)
    assert [p for p, _ in ex] == [5, 3, 4]
    assert [G.tolist() for _, G in ex] == [(np.float32(b) * J).tolist() for b in (0.25, 0.25, 0.5)]
    cage = np.array([[10, 11, 12, 13], [20, 21, 22, 23], [30, 31, 32, 33], [40, 41, 42, 43], [50, 51, 52, 53], [60, 61, 62, 63]], np.int32)
    w4 = np.float32([[1, 2, 4, 8]] * 6)
    ex = impulse_ref.expand_surface(it, tri, cage, w4)
    assert [p for p, _ in ex] == [60, 61, 62, 63, 40, 41, 42, 43, 50, 51, 52, 53]          # corners q = 0, 1, 2 = render vertices 5, 3, 4; then k = 0 .. 3
    assert [float(G[0]) for _, G in ex] == [0.25, 0.5, 1, 2, 0.25, 0.5, 1, 2, 0.5, 1, 2, 4]
    assert impulse_ref.expand_surface(impulse_hits(_hit(-1, 0, 0), J)[0], tri) == []


def test_radial_known_answers():
    c = np.float32([1, 2, 3])
    # antisymmetric about the centre: pairs c + d, c - d
    d = np.float32([[3, 4, 0], [0, 0, 2], [1, 2, 2], [0.5, 0, 0]])
    x = np.concatenate([c + d, c - d]).astype(np.float32)
    w = np.concatenate([np.float32([1, 2, 0.5, 4])] * 2)
    for flags in (0, LINEAR_FALLOFF, VELOCITY_CHANGE, LINEAR_FALLOFF | VELOCITY_CHANGE):
        v = np.zeros_like(x)
        it = impulse_explosion(c, 8.0, 2.0, linear_falloff=bool(flags & LINEAR_FALLOFF), velocity_change=bool(flags & VELOCITY_CHANGE))
        impulse_ref.apply(x, v, w, it)
        assert v.any() and np.array_equal(v[:4], -v[4:]), flags       # (by value: 0 + -0 is +0 on both sides)
    v = np.zeros_like(x)
    impulse_ref.apply(x, v, w, impulse_explosion(c, 8.0, 2.0))
    assert v[0].tolist() == [float(np.float32(2) * (np.float32(3) / np.float32(5))), float(np.float32(2) * (np.float32(4) / np.float32(5))), 0.0]
    assert v[1].tolist() == [0.0, 0.0, 4.0]                  # w = 2, strength 2, direction +z
    # negative strength pulls inwards
    v2 = np.zeros_like(x)
    impulse_ref.apply(x, v2, w, impulse_explosion(c, 8.0, -2.0))
    assert np.array_equal(v2, -v)
    # with falloff: half way out half the strength, zero AT r == radius; without falloff r2 == R2 is inclusive, just outside is not
    x = np.float32([[4, 0, 0], [8, 0, 0], [8.000001, 0, 0], [0, 8, 0]])
    w = np.ones(4, np.float32)
    v = np.zeros_like(x)
    impulse_ref.apply(x, v, w, impulse_explosion((0, 0, 0), 8.0, 2.0, linear_falloff=True))
    assert v.tolist() == [[1, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]] and not np.signbit(v[1, 0])
    v = np.zeros_like(x)
    impulse_ref.apply(x, v, w, impulse_explosion((0, 0, 0), 8.0, 2.0))
    assert v.tolist() == [[2, 0, 0], [2, 0, 0], [0, 0, 0], [0, 2, 0]]
    # radius = +inf: r / radius is 0, the falloff leaves the full strength
    v = np.zeros_like(x)
    impulse_ref.apply(x, v, w, impulse_explosion((0, 0, 0), np.inf, 2.0, linear_falloff=True))
    assert v[:2].tolist() == [[2, 0, 0], [2, 0, 0]]


def test_radial_skips_the_centre_pins_and_nan_positions():
    x = np.float32([[1, 1, 1], [2, 1, 1], [3, 1, 1], [np.nan, 1, 1], [1, np.inf, 1], [1e30, 1, 1]])
    w = np.float32([1, 0, 1, 1, 1, 1])
    v = np.full_like(x, 7.0)
    impulse_ref.apply(x, v, w, np.concatenate([impulse_explosion((1, 1, 1), np.inf, 1.0), impulse_explosion((1, 1, 1), np.inf, 1.0, linear_falloff=True, velocity_change=True)]))
    assert v[2].tolist() == [9, 7, 7]
    assert np.array_equal(v[[0, 1, 3, 4, 5]], np.full((5, 3), 7.0, np.float32))      # centre, pin, NaN, +inf (r2 = inf), r2 overflows to inf


def test_the_builders_fill_the_record():
    hits = np.zeros(3, RAY_HIT)
    hits["triangle"], hits["u"], hits["v"] = [4, -1, 7], [0.25, 0, 0.5], [0.5, 0, 0.125]
    it = impulse_hits(hits, (1, 2, 3), velocity_change=True)
    assert it["kind"].tolist() == [1, 1, 1] and it["index"].tolist() == [4, -1, 7] and it["u"].tolist() == [0.25, 0, 0.5] and it["flags"].tolist() == [1, 1, 1]
    it = impulse_explosion((1, 2, 3), 4, -5, linear_falloff=True)
    assert (it["kind"][0], it["flags"][0], it["radius"][0], it["strength"][0], it["vec"][0].tolist()) == (2, 2, 4, -5, [1, 2, 3])
    it = impulse_particles([3, 5], [(1, 0, 0), (0, 1, 0)])
    assert it["index"].tolist() == [3, 5] and it["vec"].tolist() == [[1, 0, 0], [0, 1, 0]] and not it["reserved"].any()
    raw = np.frombuffer(it.tobytes(), np.int32).reshape(2, 12)
    assert raw[:, 0].tolist() == [0, 0] and raw[:, 2].tolist() == [3, 5]
