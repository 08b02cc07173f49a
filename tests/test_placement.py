"""Placement between two ticks (SPEC.md 2d), without a GPU: what sb_group_place refuses before it touches a group, the struct's layout, and
checks of the reference the GPU tests compare against (tests/placement_ref.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

import placement_ref
from placement_ref import FROM_REFERENCE, KEEP_PINNED, SET_VELOCITY, bits
from softbodyunity_amd import make_placement, native, placement_from_rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = [("m", 9), ("frm", 3), ("to", 3), ("lin", 3), ("ang", 3)]


def bad_placements():
    """(placement, the word sb_last_error must hold) for everything SPEC.md 2d refuses in the struct itself"""
    rows = []
    for name, count in FIELDS:
        for k in (0, count - 1):
            for val in (np.nan, np.inf, -np.inf):
                p = make_placement()
                getattr(p, name)[k] = val
                rows.append((p, "NaN or infinite"))
    for flags in (8, 0x80000000, 7 | 16):
        p = make_placement(); p.flags = flags
        rows.append((p, "unknown flag"))
    for reserved in (1, 0xffffffff):
        p = make_placement(); p.reserved = reserved
        rows.append((p, "reserved"))
    return rows


def test_the_struct_is_92_bytes_in_the_header_and_in_ctypes(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "softbody_group.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu\\n", sizeof(sb_placement), offsetof(sb_placement, m), offsetof(sb_placement, from), '
                   'offsetof(sb_placement, ang)); return 0;}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    P = native.SbPlacement
    assert got == [C.sizeof(P), P.m.offset, P.frm.offset, P.ang.offset] == [92, 8, 44, 80]
    assert (native.SB_PLACE_FROM_REFERENCE, native.SB_PLACE_SET_VELOCITY, native.SB_PLACE_KEEP_PINNED) == (FROM_REFERENCE, SET_VELOCITY, KEEP_PINNED) == (1, 2, 4)


def test_null_arguments_and_bad_structs_are_refused_before_the_group_is_touched():
    L = native.lib()
    good = make_placement(to=(1, 2, 3))
    assert L.sb_group_place(None, C.byref(good)) == native.SB_ERR_INVALID_ARG and b"null" in L.sb_last_error()
    assert L.sb_group_place(None, None) == native.SB_ERR_INVALID_ARG
    # the struct's checks come before the group is looked at: a handle that is no group at all is never read
    no_group = C.create_string_buffer(64)
    assert L.sb_group_place(C.cast(no_group, C.c_void_p), None) == native.SB_ERR_INVALID_ARG and b"null" in L.sb_last_error()
    rows = bad_placements()
    assert len(rows) == 5 * 2 * 3 + 3 + 2
    for p, word in rows:
        assert L.sb_group_place(C.cast(no_group, C.c_void_p), C.byref(p)) == native.SB_ERR_INVALID_ARG
        err = L.sb_last_error().decode()
        assert word in err and "sb_group_place" in err, (word, err)
    assert no_group.raw == bytes(64)


def test_make_placement_sets_the_flags_and_the_matrix():
    p = make_placement()
    assert p.flags == 0 and list(p.m) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(p.frm) + list(p.to) + list(p.lin) + list(p.ang) == [0] * 12
    assert make_placement(lin=(1, 0, 0)).flags == SET_VELOCITY and make_placement(ang=(0, 0, 1)).flags == SET_VELOCITY
    p = make_placement(np.arange(9).reshape(3, 3), frm=(1, 2, 3), to=(4, 5, 6), from_reference=True, keep_pinned=True)
    assert p.flags == FROM_REFERENCE | KEEP_PINNED and list(p.m) == list(range(9)) and list(p.frm) == [1, 2, 3] and list(p.to) == [4, 5, 6]
    q = np.array([0.3, -0.5, 0.2, 0.7])
    assert np.array_equal(bits(placement_from_rotation(q)), bits(placement_ref.rotation(q)))
    assert np.array_equal(placement_from_rotation((0, 0, 0, 2), scale=3.0), 3 * np.eye(3, dtype=np.float32))


def _cloud(n, rng, pinned_every=5):
    x = rng.uniform(-2, 2, size=(n, 3)).astype(np.float32)
    v = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    w = rng.choice(np.float32([0.5, 1, 2]), size=n).astype(np.float32)
    w[::pinned_every] = 0
    q = rng.uniform(-2, 2, size=(n, 3)).astype(np.float32)
    return x, v, w, q


def test_a_rotation_preserves_pairwise_distances():
    # Points in the ball of radius 1/2, from = to = 0, R the float32 rounding of an exact rotation, distances taken in binary64 on the float32
    # results. Per component of x': three products and two sums, each a value below 1 in magnitude (|R d| <= |d| <= 1/2, a partial sum of
    # a row at most sqrt(3)/2), so each rounds by at most half an ulp of [1/2, 1) = 2^-25; d = x - 0 and + 0 are exact. 5 * 2^-25 per
    # component, sqrt(3) times that per point, twice that per pair: 5.2e-7 absolute. R itself: entries at most 1, each off by at most 2^-25,
    # so ||R_f - R||_2 <= ||.||_F <= 3 * 2^-25 = 8.9e-8, relative. For pairs at least 3/4 apart: 5.2e-7 / 0.75 + 8.9e-8 = 7.8e-7 < 1e-6.
    rng = np.random.default_rng(5)
    d = rng.normal(size=(400, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    x = (0.4999 * d * rng.uniform(0, 1, size=(400, 1)) ** (1 / 3)).astype(np.float32)
    assert np.linalg.norm(x.astype(np.float64), axis=1).max() <= 0.5
    i, j = np.triu_indices(400, 1)
    before = np.linalg.norm(x[i].astype(np.float64) - x[j].astype(np.float64), axis=1)
    far = before >= 0.75
    assert far.sum() > 1000
    for quat in ((0.3, -0.5, 0.2, 0.7), (1, 0, 0, 0), (0.5, 0.5, 0.5, 0.5), rng.normal(size=4)):
        y, v = x.copy(), np.zeros_like(x)
        placement_ref.apply(y, v, np.ones(400, np.float32), None, m=placement_ref.rotation(quat))
        after = np.linalg.norm(y[i].astype(np.float64) - y[j].astype(np.float64), axis=1)
        rel = np.abs(after[far] - before[far]) / before[far]
        print("rotation %s: largest relative change of a distance %.3e" % (np.round(np.asarray(quat, float), 3), rel.max()))
        assert rel.max() <= 1e-6


def test_from_reference_with_the_identity_returns_the_reference_pose_except_at_minus_zero():
    rng = np.random.default_rng(6)
    x, v, w, q = _cloud(64, rng)
    q[3] = (-0.0, 1e-40, -1e-40); q[4] = (3e38, -3e38, -0.0); q[7, 1] = np.float32(1e-45)
    placement_ref.apply(x, v, w, q, flags=FROM_REFERENCE)
    neg_zero = bits(q) == 0x80000000
    assert neg_zero.sum() == 2 and (bits(x)[neg_zero] == 0).all(), "(-0 + 0) = +0: the identity is not a bit-identity at -0"
    assert np.array_equal(bits(x)[~neg_zero], bits(q)[~neg_zero])
    assert (v[w > 0] == 0).all() and (v[w == 0] != 0).any(), "at rest; a pinned particle keeps its velocity"


def test_keep_pinned_leaves_pinned_rows_alone_and_every_written_nan_is_canonical():
    rng = np.random.default_rng(7)
    x, v, w, q = _cloud(60, rng)
    payload = np.array([0x7fc12345, 0xffc00001, 0x7f800001], np.uint32)      # quiet, negative quiet, signalling
    x.view(np.uint32)[0] = payload; v.view(np.uint32)[0] = payload[::-1]       # pinned row
    x.view(np.uint32)[1] = payload; v.view(np.uint32)[1] = payload[::-1]       # free row
    x[2] = (np.inf, 1, 1); v[2] = (1, -np.inf, np.inf)                         # free: inf * 0 and inf - inf
    x[5] = (np.inf, -np.inf, 0)                                                # pinned
    m = placement_ref.rotation((0.1, 0.2, 0.3, 0.9))
    pinned = w == 0
    assert pinned[0] and pinned[5] and not pinned[1] and not pinned[2]
    for flags in range(8):
        x1, v1 = x.copy(), v.copy()
        placement_ref.apply(x1, v1, w, q, m=m, frm=(0.5, 0, 0), to=(0, 1, 0), lin=(1, 2, 3), ang=(0, 0, 1), flags=flags)
        assert np.array_equal(bits(v1[pinned]), bits(v[pinned])), "a pinned particle keeps its velocity's bits"
        if flags & KEEP_PINNED:
            assert np.array_equal(bits(x1[pinned]), bits(x[pinned]))
        else:
            assert not np.array_equal(bits(x1[pinned]), bits(x[pinned]))
        written = np.ones_like(x, bool) if not flags & KEEP_PINNED else np.repeat(~pinned[:, None], 3, axis=1)
        nx = np.isnan(x1) & written
        nv = np.isnan(v1) & ~pinned[:, None]
        assert (bits(x1)[nx] == 0x7fc00000).all() and (bits(v1)[nv] == 0x7fc00000).all()
        if not flags & FROM_REFERENCE:
            assert nx[1].all() and nv[1].all() and np.isinf(x1[2]).any()
        assert (bits(x1) != bits(x)).any() and (bits(v1) != bits(v)).any()
