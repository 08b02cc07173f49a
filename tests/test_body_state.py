"""The body state without a GPU (SPEC.md 6f): sb_body_state's layout, the bindings of the two entry points, and the pure host derivation
sb_group_body_state_from_sums against tests/body_state_ref.py's numpy derivation on bodies whose condition numbers the test asserts.

Tolerance, derived: both sides start from the same 32 doubles. The fields that are sums, quotients and differences of them agree to a few
roundings of their natural scale (body_state_ref.field_scales); the 3x3 solve behind angular_velocity and the polar factor behind rotation
are backward stable on both sides, so on inputs with condition number kappa <= 10 their forward errors are at most 64 kappa 2^-53
relative -- 64 roundings is generous for a 3x3 Jacobi iteration and for LAPACK alike."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import body_state_ref as B
from softbodyunity_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = C.POINTER(C.c_double)
TOL = 64 * B.U
NAMES = ("sb_group_get_body_state", "sb_group_body_state_from_sums")


# ---- 1. sizes and bindings ------------------------------------------------------------------------------------------------------------------

def test_the_struct_has_the_headers_size_and_offsets(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "softbody_group.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu %u %u %u %u %u\\n", sizeof(sb_body_state), offsetof(sb_body_state, sums), offsetof(sb_body_state, mass), '
                   'offsetof(sb_body_state, rotation), offsetof(sb_body_state, momentum), offsetof(sb_body_state, kinetic_energy), '
                   'SB_BODY_POSE, SB_BODY_MOTION, SB_BODY_NO_MASS, SB_BODY_DEGENERATE_POSE, SB_BODY_DEGENERATE_INERTIA); return 0;}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(t) for t in subprocess.check_output([str(exe)], text=True).split()]
    T = native.SbBodyState
    assert got == [C.sizeof(T), T.sums.offset, T.mass.offset, T.rotation.offset, T.momentum.offset, T.kinetic_energy.offset,
                   native.SB_BODY_POSE, native.SB_BODY_MOTION, native.SB_BODY_NO_MASS, native.SB_BODY_DEGENERATE_POSE, native.SB_BODY_DEGENERATE_INERTIA]
    assert C.sizeof(T) == 24 + 8 * (32 + 1 + 3 + 3 + 6 + 9 + 4 + 3 + 3 + 3 + 3 + 1)
    assert (B.POSE, B.MOTION, B.NO_MASS, B.DEGENERATE_POSE, B.DEGENERATE_INERTIA) == tuple(got[6:])


def test_both_names_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "softbody_group.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", native.LIB_PATH], text=True)
    cs = open(os.path.join(ROOT, "csharp", "SoftbodyNative.cs")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert re.search(r" T " + name + r"$", exported, re.M), name
        assert name in native.SIGNATURES
        assert re.search(r"static extern int\s+" + name + r"\s*\(", cs), name
    assert "struct SbBodyState" in cs
    # the solver header stays as it was: the feature lives on the group's surface
    assert "body_state" not in open(os.path.join(ROOT, "include", "softbody.h")).read()
    assert native.lib().sb_abi_version() == 8


# ---- 2. the derivation ------------------------------------------------------------------------------------------------------------------------

def _rot(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _box(nx, ny, nz, extent):
    g = np.stack(np.meshgrid(np.linspace(0, extent[0], nx), np.linspace(0, extent[1], ny), np.linspace(0, extent[2], nz), indexing="ij"), -1)
    return g.reshape(-1, 3)


def _sums_of(x, v, q, m):
    """the 32 sums of a body given in float64, as float64 (the derivation is what is under test, not the reduction)"""
    x, v, q, m = (np.asarray(a, np.float64) for a in (x, v, q, m))
    S = np.zeros(32)
    S[0] = m.sum(); S[1:4] = m @ x; S[4:7] = m @ q
    xx = np.einsum("p,pa,pb->ab", m, x, x)
    S[7:13] = [xx[0, 0], xx[1, 1], xx[2, 2], xx[0, 1], xx[0, 2], xx[1, 2]]
    S[13:22] = np.einsum("p,pa,pb->ab", m, x, q).reshape(9)
    S[22:25] = m @ v; S[25:28] = m @ np.cross(x, v); S[28] = m @ (v * v).sum(1)
    return S


def _body(q, m, flags=0, mirror=False):
    """(q, x, v, masses, expected flags): x = R0 q + t (mirror: of the pose reflected in z), v = V0 + W0 x (x - mass centre)"""
    x = (q * np.array([1.0, 1.0, -1.0]) if mirror else q) @ R0.T + T0
    return q, x, V0 + np.cross(W0, x - (m @ x) / m.sum()), m, flags


R0 = _rot([1.0, 2.0, -0.5], 0.7)
T0, V0, W0 = np.array([1.5, -0.75, 2.0]), np.array([0.3, -1.2, 0.8]), np.array([0.4, 0.9, -0.6])
rng = np.random.default_rng(5)
_cube_q = _box(5, 6, 7, (1.0, 1.5, 2.0))
_cloth_q = _box(9, 8, 1, (2.0, 1.5, 0.0))
_line_q = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, -1.0], [2.5, 5.0, -2.5]])
BODIES = {
    "rigid cube": _body(_cube_q, rng.uniform(0.5, 2.0, len(_cube_q))),
    "flat cloth": _body(_cloth_q, rng.uniform(0.5, 2.0, len(_cloth_q))),
    "reflected": _body(_cube_q, rng.uniform(0.5, 2.0, len(_cube_q)), mirror=True),
    "collinear": _body(_line_q, np.array([1.0, 2.0, 0.5]), B.DEGENERATE_POSE | B.DEGENERATE_INERTIA),
    "one particle": _body(_line_q[1:2], np.array([2.0]), B.DEGENERATE_POSE | B.DEGENERATE_INERTIA),
}


def _from_sums(S, n_dyn, n_pin, what):
    st = native.SbBodyState()
    S = np.ascontiguousarray(S, np.float64)
    rc = native.lib().sb_group_body_state_from_sums(S.ctypes.data_as(DP), n_dyn, n_pin, what, C.byref(st))
    assert rc == native.SB_OK, native.lib().sb_last_error()
    return st.as_dict()


def _kappas(ref):
    """condition numbers of the two solves: 2 sigma_1 / (sigma_2 + sign(det) sigma_3) for the polar factor (a reflected pose's Kabsch rotation
    turns on sigma_2 - sigma_3), lambda_max / lambda_min for the inertia"""
    _, s, d = B.kabsch(ref["apq"])
    k_pose = 2 * s[0] / (s[1] + d * s[2]) if s[1] > 1e-12 * s[0] else np.inf
    lam = np.linalg.eigvalsh(B.inertia_of(ref["second_moment"]))
    k_inertia = lam[2] / lam[0] if lam[0] > 1e-12 * lam[2] else np.inf
    return k_pose, k_inertia


def _compare(got, ref, S, what, k_pose, k_inertia):
    sc = B.field_scales(S, ref["n_dynamic"])
    M, L, Lq, Uv = sc["M"], sc["L"], sc["Lq"], sc["Uv"]
    scale = dict(mass=M, com=L, ref_com=Lq, second_moment=M * L * L, apq=M * L * Lq, momentum=M * Uv, velocity=Uv, angular_momentum=M * L * Uv,
                 kinetic_energy=M * Uv * Uv)
    for f, s in scale.items():
        err = np.max(np.abs(np.asarray(got[f]) - np.asarray(ref[f])))
        assert err <= TOL * s, (f, err, TOL * s)
    assert got["flags"] == ref["flags"] and got["what"] == what
    assert np.array_equal(got["sums"], ref["sums"])
    if what & B.POSE and np.isfinite(k_pose):
        assert np.max(np.abs(got["rotation"] - ref["rotation"])) <= TOL * k_pose, (got["rotation"], ref["rotation"])
        assert abs(np.linalg.norm(got["rotation"]) - 1) <= 8 * B.U and got["rotation"][3] >= 0
    else:
        assert np.array_equal(got["rotation"], [0, 0, 0, 1])
    if what & B.MOTION and np.isfinite(k_inertia):
        assert np.max(np.abs(got["angular_velocity"] - ref["angular_velocity"])) <= TOL * k_inertia * np.linalg.norm(ref["angular_velocity"])
    else:
        assert np.array_equal(got["angular_velocity"], np.zeros(3))


@pytest.mark.parametrize("what", [B.POSE, B.MOTION, B.POSE | B.MOTION], ids=["pose", "motion", "both"])
@pytest.mark.parametrize("name", list(BODIES))
def test_the_derivation_matches_numpy(name, what):
    q, x, v, m, flags = BODIES[name]
    S = _sums_of(x, v, q, m)
    ref_all = B.derive_ref(S, len(m), 3, B.POSE | B.MOTION)
    k_pose, k_inertia = _kappas(ref_all)
    if flags == 0:
        assert k_pose <= 10 and k_inertia <= 10, (k_pose, k_inertia)
    else:
        assert np.isinf(k_pose) and np.isinf(k_inertia)
    ref = B.derive_ref(S, len(m), 3, what)
    got = _from_sums(S, len(m), 3, what)
    print(f"{name}: kappa_pose {k_pose:.3g} kappa_inertia {k_inertia:.3g} rotation {got['rotation']} omega {got['angular_velocity']}")
    assert ref["flags"] == (flags & ((B.DEGENERATE_POSE if what & B.POSE else 0) | (B.DEGENERATE_INERTIA if what & B.MOTION else 0)))
    assert got["n_dynamic"] == len(m) and got["n_pinned"] == 3
    _compare(got, ref, S, what, k_pose, k_inertia)
    # fields that were not asked for are exactly 0
    if not what & B.POSE:
        assert not got["ref_com"].any() and not got["apq"].any()
    if not what & B.MOTION:
        assert not got["momentum"].any() and not got["velocity"].any() and not got["angular_momentum"].any() and got["kinetic_energy"] == 0
    # and the known answers behind the bodies that are rigid motions of their reference pose
    if flags == 0:
        if what & B.POSE:
            got_R = B.rotation_of(got["rotation"])
            assert abs(np.linalg.det(got_R) - 1) <= 1e-12, "a reflected pose must come back as a proper rotation"
            det = np.linalg.det(ref_all["apq"])
            assert det < 0 if name == "reflected" else (det == 0 if name == "flat cloth" else det > 0)
            if name != "reflected":        # apq = R0 (sum m q q^T): its polar factor is R0, whatever the masses (cloth: the one proper completion)
                assert np.max(np.abs(got_R - R0)) <= 1e-12, (got_R, R0)
        if what & B.MOTION:
            assert np.max(np.abs(got["angular_velocity"] - W0)) <= 1e-12 and np.max(np.abs(got["velocity"] - V0)) <= 1e-12
            inertia = B.inertia_of(got["second_moment"])
            assert abs(got["kinetic_energy"] - (0.5 * got["mass"] * V0 @ V0 + 0.5 * W0 @ inertia @ W0)) <= 1e-12 * got["kinetic_energy"]


def test_no_dynamic_particle_is_all_zeros_and_the_identity():
    S = np.arange(32, dtype=np.float64) + 1
    got = _from_sums(S, 0, 5, B.POSE | B.MOTION)
    assert got["flags"] == B.NO_MASS and got["n_dynamic"] == 0 and got["n_pinned"] == 5
    for f, v in got.items():
        if f == "rotation":
            assert np.array_equal(v, [0, 0, 0, 1])
        elif f not in ("flags", "n_pinned", "what"):
            assert not np.any(v), f
    ref = B.derive_ref(S, 0, 5, 3)
    assert ref["flags"] == B.NO_MASS


def test_a_compound_body_is_the_sum_of_its_parts():
    # what the pure entry point is for: the sums of two bodies added on the host give the state of the pair
    q, x, v, m, _ = BODIES["rigid cube"]
    half = len(m) // 2
    Sa, Sb = _sums_of(x[:half], v[:half], q[:half], m[:half]), _sums_of(x[half:], v[half:], q[half:], m[half:])
    whole = _from_sums(_sums_of(x, v, q, m), len(m), 0, 3)
    pair = _from_sums(Sa + Sb, len(m), 0, 3)
    assert np.max(np.abs(pair["rotation"] - whole["rotation"])) <= TOL * 10 and np.max(np.abs(pair["com"] - whole["com"])) <= TOL * 4
    assert np.max(np.abs(pair["angular_velocity"] - whole["angular_velocity"])) <= 1e-12


def test_non_finite_sums_propagate_and_return():
    q, x, v, m, _ = BODIES["rigid cube"]
    S = _sums_of(x, v, q, m)
    S[1] = np.nan
    got = _from_sums(S, len(m), 0, 3)
    assert np.isfinite(got["mass"]) and np.isnan(got["com"][0]) and np.isnan(got["rotation"]).any() and np.isnan(got["angular_velocity"]).any()
    S = _sums_of(x, v, q, m)
    S[13] = np.inf
    got = _from_sums(S, len(m), 0, B.POSE)
    assert not np.isfinite(got["rotation"]).all() and np.isfinite(got["com"]).all()


# ---- 3. argument errors of the pure function ----------------------------------------------------------------------------------------------------

def test_argument_errors_leave_out_untouched():
    L = native.lib()
    S = np.ones(32)
    st = native.SbBodyState()
    C.memset(C.byref(st), 0x5A, C.sizeof(st))
    poisoned = bytes(st)
    p = S.ctypes.data_as(DP)
    for args in ((None, 1, 0, 3, C.byref(st)), (p, 1, 0, 3, None), (p, 1, 0, 0, C.byref(st)), (p, 1, 0, 4, C.byref(st)), (p, 1, 0, 7, C.byref(st)),
                 (p, 1, 0, 0x80000001, C.byref(st)), (p, -1, 0, 3, C.byref(st)), (p, 1, -2, 3, C.byref(st))):
        assert L.sb_group_body_state_from_sums(*args) == native.SB_ERR_INVALID_ARG, args
        assert b"sb_group_body_state_from_sums" in L.sb_last_error()
        assert bytes(st) == poisoned
    # the group's entry point refuses the same without a GPU: null handle first
    assert L.sb_group_get_body_state(None, 3, C.byref(st)) == native.SB_ERR_INVALID_ARG and bytes(st) == poisoned
    assert L.sb_group_body_state_from_sums(p, 1, 0, 3, C.byref(st)) == native.SB_OK and bytes(st) != poisoned
