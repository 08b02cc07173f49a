"""Reference for placement between two ticks (SPEC.md 2d): numpy float32, one operation per line, in the spec's bracketing. numpy neither
contracts a product and a sum into an FMA nor flushes denormals, so the GPU must reproduce this bit for bit from the same positions,
velocities, inverse masses and reference pose."""
import numpy as np

FROM_REFERENCE, SET_VELOCITY, KEEP_PINNED = 1, 2, 4
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _canonical(a):
    """a component that is written and comes out NaN is THE quiet NaN 0x7fc00000 (SPEC.md 2d, the rule of 2c)"""
    a = np.array(a, np.float32)
    a.view(np.uint32)[np.isnan(a)] = 0x7fc00000
    return a


def rotation(quat_xyzw):
    """the float32 matrix of a quaternion (x, y, z, w), normalised in binary64 and rounded once: what placement_from_rotation builds"""
    q = np.asarray(quat_xyzw, np.float64)
    x, y, z, w = q / np.sqrt(np.dot(q, q))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float64).astype(np.float32)


def apply(x, v, w, q, m=None, frm=(0, 0, 0), to=(0, 0, 0), lin=(0, 0, 0), ang=(0, 0, 0), flags=0):
    """SPEC.md 2d on float32 arrays x (n,3), v (n,3), w (n,), q (n,3; the reference pose, may be None without FROM_REFERENCE): x and v are
    changed in place. Returns (x, v)."""
    assert x.dtype == np.float32 and v.dtype == np.float32 and w.dtype == np.float32
    m = np.asarray(np.eye(3) if m is None else m, np.float32).reshape(9)
    frm, to, lin, ang = (np.asarray(a, np.float32).reshape(3) for a in (frm, to, lin, ang))
    ref = bool(flags & FROM_REFERENCE)
    setv = ref or bool(flags & SET_VELOCITY)
    moved = (w != 0) if flags & KEEP_PINNED else np.ones(w.shape[0], bool)      # KEEP_PINNED: w == 0 is left entirely alone
    free = moved & (w > 0)                                                      # velocity: particles with w > 0 only
    with np.errstate(all="ignore"):
        src = np.asarray(q, np.float32) if ref else x
        dx = src[:, 0] - frm[0]
        dy = src[:, 1] - frm[1]
        dz = src[:, 2] - frm[2]
        xn = np.empty_like(x)
        for c in range(3):
            a = m[3 * c] * dx
            b = m[3 * c + 1] * dy
            e = m[3 * c + 2] * dz
            ab = a + b
            abe = ab + e
            xn[:, c] = abe + to[c]
        xn = _canonical(xn)
        assert xn.dtype == np.float32 and dx.dtype == np.float32
        vn = np.empty_like(v)
        if setv:
            ax = xn[:, 0] - to[0]
            ay = xn[:, 1] - to[1]
            az = xn[:, 2] - to[2]
            yz = ang[1] * az
            zy = ang[2] * ay
            zx = ang[2] * ax
            xz = ang[0] * az
            xy = ang[0] * ay
            yx = ang[1] * ax
            cx = yz - zy
            cy = zx - xz
            cz = xy - yx
            vn[:, 0] = lin[0] + cx
            vn[:, 1] = lin[1] + cy
            vn[:, 2] = lin[2] + cz
        else:
            vx, vy, vz = v[:, 0].copy(), v[:, 1].copy(), v[:, 2].copy()
            for c in range(3):
                a = m[3 * c] * vx
                b = m[3 * c + 1] * vy
                ab = a + b
                e = m[3 * c + 2] * vz
                vn[:, c] = ab + e
        vn = _canonical(vn)
        assert vn.dtype == np.float32
    # what is not written keeps its bits (copies through uint32: no float operation touches a payload)
    assert x.flags.c_contiguous and v.flags.c_contiguous
    x.view(np.uint32)[moved] = xn.view(np.uint32)[moved]
    v.view(np.uint32)[free] = vn.view(np.uint32)[free]
    return x, v
