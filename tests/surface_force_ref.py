"""Reference for surface forces between two ticks (SPEC.md 2e): numpy float32, a sequential loop, one operation per line, in the spec's
bracketing. numpy neither contracts a product and a sum into an FMA nor flushes denormals, and its float32 divide and sqrt are correctly
rounded, so the GPU must reproduce this bit for bit from the same positions, velocities, inverse masses and triangles."""
import numpy as np

F = np.float32
SIX, THREE = F(6.0), F(3.0)
L2_MIN = F(2.0 ** -96)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def host_scalars(normal, tangential, pressure, dt):
    """hn, ht, hp: (dt * coefficient) / 6, each product rounded before the division"""
    dt = F(dt)
    with np.errstate(all="ignore"):
        return [F(F(dt * F(k)) / SIX) for k in (normal, tangential, pressure)]


@np.errstate(all="ignore")
def triangle_impulse(x, v, abc, wind, hn, ht, hp):
    """phase 1 for one triangle -> J_t (3,) float32, or None where the triangle is skipped"""
    a, b, c = (int(i) for i in abc)
    e1 = x[b] - x[a]
    e2 = x[c] - x[a]
    f = np.empty(3, np.float32)
    f[0] = F(e1[1] * e2[2]) - F(e1[2] * e2[1])
    f[1] = F(e1[2] * e2[0]) - F(e1[0] * e2[2])
    f[2] = F(e1[0] * e2[1]) - F(e1[1] * e2[0])
    L2 = F(F(f[0] * f[0]) + F(f[1] * f[1])) + F(f[2] * f[2])
    if not (L2 >= L2_MIN) or not (L2 < np.inf):
        return None
    L = np.sqrt(L2)
    u = np.empty(3, np.float32)
    for k in range(3):
        s = v[a, k] + v[b, k]
        s = s + v[c, k]
        vt = s / THREE
        u[k] = wind[k] - vt
    uf = F(F(u[0] * f[0]) + F(u[1] * f[1])) + F(u[2] * f[2])
    q = uf / L2
    J = np.empty(3, np.float32)
    for k in range(3):
        un = q * f[k]
        ut = u[k] - un
        d = F(hn * un) + F(ht * ut)
        J[k] = F(L * d) + F(hp * f[k])
    assert L.dtype == np.float32 and q.dtype == np.float32
    return J


def apply(x, v, w, tri, wind=(0, 0, 0), normal=0.0, tangential=0.0, pressure=0.0, dt=0.02):
    """SPEC.md 2e on float32 arrays x (n,3), v (n,3), w (n,) and triangles (m,3): v is changed in place, nothing else is."""
    assert x.dtype == np.float32 and v.dtype == np.float32 and w.dtype == np.float32
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    wind = np.asarray(wind, np.float32)
    with np.errstate(all="ignore"):
        hn, ht, hp = host_scalars(normal, tangential, pressure, dt)
        J = [triangle_impulse(x, v, abc, wind, hn, ht, hp) for abc in tri]        # phase 1: every triangle from the state before the call
        G = np.zeros((x.shape[0], 3), np.float32)
        met = np.zeros(x.shape[0], bool)
        for t in range(tri.shape[0]):                                                # phase 2: ascending t, once per corner slot
            if J[t] is None:
                continue
            for p in tri[t]:
                G[p] = G[p] + J[t]
                met[p] = True
        for p in np.nonzero(met)[0]:
            if not (w[p] > 0):
                continue
            r = v[p] + w[p] * G[p]
            r.view(np.uint32)[np.isnan(r)] = 0x7fc00000
            v[p] = r
    return v
