"""Reference for heightfield contacts between two ticks (SPEC.md 2h): numpy float32, one operation per line, in the spec's bracketing,
elementwise operations only (no np.dot, no einsum: their summation order is not the spec's). numpy neither contracts a product and a sum
into an FMA nor flushes denormals, and its float32 division and square root are correctly rounded, so the GPU must reproduce this bit for
bit from the same positions, velocities, inverse masses, descriptor and heights. The response is SPEC.md 2f's, restated here with
lin = ang = 0 (the products with 0 stay: they make a NaN of an infinite x')."""
import numpy as np

F = np.float32
MAX_SAMPLES = 4097


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _canonical(a):
    """a component that is written and comes out NaN is THE quiet NaN 0x7fc00000 (SPEC.md 2h, the rule of 2c, 2d and 2f)"""
    a = np.array(a, np.float32)
    a.view(np.uint32)[np.isnan(a)] = 0x7fc00000
    return a


def make(a, cell, heights2d, rot=None, thickness=1.0):
    """a heightfield: heights2d is (nz, nx), heights2d[iz, ix]; cell one spacing or (along ix, along iz); rot (3, 3), rows = ix axis, up, iz axis"""
    h = np.ascontiguousarray(heights2d, np.float32)
    assert h.ndim == 2
    return dict(a=np.asarray(a, np.float32).reshape(3), rot=(np.eye(3, dtype=np.float32) if rot is None else np.asarray(rot, np.float32)).reshape(9).copy(),
                cell=np.broadcast_to(np.asarray(cell, np.float32), (2,)).copy(), nx=int(h.shape[1]), nz=int(h.shape[0]), thickness=F(thickness), h=h.reshape(-1).copy())


def _dot(ax, ay, az, bx, by, bz):
    xx = ax * bx
    yy = ay * by
    zz = az * bz
    xy = xx + yy
    return xy + zz


TRACE_KEYS = ["outside_x_low", "outside_x_high", "outside_z_low", "outside_z_high", "clamp_x", "clamp_z", "lower", "upper", "diagonal",
              "gap_nonpositive", "gap_zero", "too_deep", "depth_equals_thickness", "stick", "slip", "approaching", "separating"]


def new_trace():
    return {k: 0 for k in TRACE_KEYS}


def surface(hf, x):
    """the geometry of SPEC.md 2h for the points x (n, 3), every intermediate float32: a dict of arrays -- q (3 arrays), fx, fz, inside (the
    footprint), ix, iz, tx, tz, lower, sx, sz, height, gap, depth, n (3 arrays), hit (before the inverse mass is looked at)"""
    assert x.dtype == np.float32
    a, R, cell, nx, nz, h = hf["a"], hf["rot"], hf["cell"], hf["nx"], hf["nz"], hf["h"]
    assert h.dtype == np.float32 and h.size == nx * nz and 2 <= nx <= MAX_SAMPLES and 2 <= nz <= MAX_SAMPLES
    with np.errstate(all="ignore"):
        ex = x[:, 0] - a[0]
        ey = x[:, 1] - a[1]
        ez = x[:, 2] - a[2]
        q = [_dot(ex, ey, ez, R[3 * k], R[3 * k + 1], R[3 * k + 2]) for k in range(3)]
        fx = q[0] / cell[0]
        fz = q[2] / cell[1]
        inside = (fx >= 0) & (fx <= F(nx - 1)) & (fz >= 0) & (fz <= F(nz - 1))          # a NaN compares false
        ix0 = np.where(inside, fx, F(0)).astype(np.int32)                              # (int): truncation; only looked at inside
        iz0 = np.where(inside, fz, F(0)).astype(np.int32)
        ix = np.minimum(ix0, nx - 2)
        iz = np.minimum(iz0, nz - 2)
        tx = fx - ix.astype(np.float32)
        tz = fz - iz.astype(np.float32)
        base = iz.astype(np.int64) * nx + ix
        h00 = h[base]
        h10 = h[base + 1]
        h01 = h[base + nx]
        h11 = h[base + nx + 1]
        tt = tx + tz
        lower = tt <= 1
        sx = np.where(lower, h10 - h00, h11 - h01)
        sz = np.where(lower, h01 - h00, h11 - h10)
        ux = np.where(lower, tx, F(1) - tx)
        uz = np.where(lower, tz, F(1) - tz)
        px = ux * sx
        pz = uz * sz
        lo1 = h00 + px
        lo2 = lo1 + pz
        up1 = h11 - px
        up2 = up1 - pz
        height = np.where(lower, lo2, up2)
        gap = height - q[1]
        gx = sx / cell[0]
        gz = sz / cell[1]
        gxx = gx * gx
        gzz = gz * gz
        g1 = gxx + F(1)
        l2 = g1 + gzz
        length = np.sqrt(l2)
        m0 = (-gx) / length
        m1 = F(1) / length
        m2 = (-gz) / length
        depth = gap * m1
        hit = inside & (gap > 0) & (depth < hf["thickness"])
        n = []
        for c in range(3):
            na = m0 * R[c]
            nb = m1 * R[3 + c]
            ne = m2 * R[6 + c]
            nab = na + nb
            n.append(nab + ne)
    out = dict(q=q, fx=fx, fz=fz, inside=inside, ix0=ix0, iz0=iz0, ix=ix, iz=iz, tx=tx, tz=tz, tt=tt, lower=lower, sx=sx, sz=sz, height=height, gap=gap, depth=depth, n=n, hit=hit)
    for k in ("fx", "fz", "tx", "tz", "tt", "sx", "sz", "height", "gap", "depth"):
        assert out[k].dtype == np.float32, k
    for arr in q + n + [px, pz, lo2, up2, gx, l2, length, m0, m1, m2]:
        assert arr.dtype == np.float32
    return out


def apply(x, v, w, hf, friction=0.0, restitution=0.0, trace=None):
    """SPEC.md 2h on float32 arrays x (n,3), v (n,3), w (n,): x and v are changed in place. Returns the hit mask (n,): the particles whose
    position was written. `trace` (new_trace()) counts the branches taken, over the particles with w > 0."""
    assert x.dtype == np.float32 and v.dtype == np.float32 and w.dtype == np.float32 and x.flags.c_contiguous and v.flags.c_contiguous
    friction, restitution = F(friction), F(restitution)
    free = w > 0
    g = surface(hf, x)
    hit = g["hit"] & free
    n, depth, a = g["n"], g["depth"], hf["a"]
    zero = F(0)
    with np.errstate(all="ignore"):
        xn = [_canonical(x[:, c] + depth * n[c]) for c in range(3)]
        # 2f's response with lin = ang = 0, from the rounded x'
        px = xn[0] - a[0]
        py = xn[1] - a[1]
        pz = xn[2] - a[2]
        yz = zero * pz
        zy = zero * py
        zx = zero * px
        xz = zero * pz
        xy = zero * py
        yx = zero * px
        vcx = zero + (yz - zy)
        vcy = zero + (zx - xz)
        vcz = zero + (xy - yx)
        ux = v[:, 0] - vcx
        uy = v[:, 1] - vcy
        uz = v[:, 2] - vcz
        un = _dot(ux, uy, uz, n[0], n[1], n[2])
        approaching = un < 0                       # false for a NaN: the velocity is then not written
        jn = -un
        tx = ux - un * n[0]
        ty = uy - un * n[1]
        tz = uz - un * n[2]
        t2 = _dot(tx, ty, tz, tx, ty, tz)
        tl = np.sqrt(t2)
        lim = friction * jn
        slip = (t2 > 0) & (tl > lim)
        scale = F(1) - lim / tl
        tx = np.where(slip, scale * tx, zero)
        ty = np.where(slip, scale * ty, zero)
        tz = np.where(slip, scale * tz, zero)
        un2 = restitution * jn
        vn = [_canonical(vcx + (tx + un2 * n[0])), _canonical(vcy + (ty + un2 * n[1])), _canonical(vcz + (tz + un2 * n[2]))]
    for arr in (un, tl, scale, un2, vcx, vn[0], xn[0], tx):
        assert arr.dtype == np.float32
    wv = hit & approaching
    if trace is not None:
        nx, nz = hf["nx"], hf["nz"]
        with np.errstate(all="ignore"):
            trace["outside_x_low"] += int((free & (g["fx"] < 0)).sum()); trace["outside_x_high"] += int((free & (g["fx"] > F(nx - 1))).sum())
            trace["outside_z_low"] += int((free & (g["fz"] < 0)).sum()); trace["outside_z_high"] += int((free & (g["fz"] > F(nz - 1))).sum())
            ins = free & g["inside"]
            trace["clamp_x"] += int((ins & (g["ix0"] > nx - 2)).sum()); trace["clamp_z"] += int((ins & (g["iz0"] > nz - 2)).sum())
            trace["diagonal"] += int((ins & (g["tt"] == 1)).sum())
            trace["lower"] += int((ins & (g["tt"] < 1)).sum()); trace["upper"] += int((ins & ~g["lower"]).sum())
            trace["gap_nonpositive"] += int((ins & ~(g["gap"] > 0)).sum()); trace["gap_zero"] += int((ins & (g["gap"] == 0)).sum())
            deep = ins & (g["gap"] > 0) & ~(depth < hf["thickness"])
            trace["too_deep"] += int(deep.sum()); trace["depth_equals_thickness"] += int((deep & (depth == hf["thickness"])).sum())
        trace["approaching"] += int(wv.sum()); trace["separating"] += int((hit & ~approaching).sum())
        trace["slip"] += int((wv & slip).sum()); trace["stick"] += int((wv & ~slip).sum())
    # what is not written keeps its bits (copies through uint32: no float operation touches a payload)
    for c in range(3):
        x.view(np.uint32)[hit, c] = xn[c].view(np.uint32)[hit]
        v.view(np.uint32)[wv, c] = vn[c].view(np.uint32)[wv]
    return hit


def to_native(hf):
    """the reference's heightfield as (native.SbHeightfield, heights) for sb_group_set_heightfield (the fields are float32 already)"""
    from softbodyunity_amd import native
    d = native.SbHeightfield()
    d.a[:] = [float(t) for t in hf["a"]]
    d.rot[:] = [float(t) for t in hf["rot"]]
    d.cell[:] = [float(t) for t in hf["cell"]]
    d.nx, d.nz, d.thickness = hf["nx"], hf["nz"], float(hf["thickness"])
    return d, hf["h"]
