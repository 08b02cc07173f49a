// SoftbodyCpuSolver.cs — the C# CPU FixedUpdate path: a sequential restatement of SPEC.md, identical
// operation for operation to oracle/oracle.c (which is what the test-suite actually runs, because no C#
// toolchain exists in the build image). The reference repository has no CPU solver to copy
// (/root/reference/README.md:1 is its only line).
//
// C# evaluates float expressions in at least float precision but MAY use higher precision for
// intermediates; every intermediate below is therefore stored to a float local (an explicit cast forces
// rounding to binary32, ECMA-335 §I.12.1.3), and no Math.FusedMultiplyAdd is used.
using System;
using UnityEngine;

namespace SoftbodyMI355X
{
    public sealed class SoftbodyCpuSolver
    {
        readonly Softbody sb;
        readonly byte[][] orderTypeByParity;   // SPEC.md §3: substep k of a tick walks the order of parity k & 1
        readonly int[][] orderIdByParity;
        readonly Vector3[] prev;

        public SoftbodyCpuSolver(Softbody owner, byte[][] type, int[][] id)
        {
            sb = owner; orderTypeByParity = type; orderIdByParity = id;
            prev = new Vector3[owner.positions.Length];
        }

        public void Step(float dt, int substeps)
        {
            // SPEC.md §2 host-side scalars
            float S = (float)substeps;
            float h = (float)(dt / S);
            float invH = (float)(1.0f / h);
            Vector3 g = sb.Gravity;
            float hgx = (float)(h * g.x), hgy = (float)(h * g.y), hgz = (float)(h * g.z);
            float td = (float)(sb.Damping * h);
            float kd = (float)(1.0f - td); if (kd < 0f) kd = 0f;
            float h2 = (float)(h * h);
            float atD = (float)(sb.ComplianceD / h2);
            float av = (float)(sb.ComplianceV / h2);
            float atV = (float)(36.0f * av);
            float atB = (float)(sb.ComplianceB / h2);
            Vector3[] x = sb.positions; Vector3[] v = sb.velocities; float[] w = sb.inverseMass;
            int n = x.Length;
            for (int it = 0; it < substeps; ++it)
            {
                byte[] orderType = orderTypeByParity[it & 1];
                int[] orderId = orderIdByParity[it & 1];
                for (int p = 0; p < n; ++p)
                {
                    prev[p] = x[p];
                    if (w[p] > 0f)
                    {
                        float vx = (float)(v[p].x + hgx), vy = (float)(v[p].y + hgy), vz = (float)(v[p].z + hgz);
                        v[p] = new Vector3(vx, vy, vz);
                        float ax = (float)(h * vx), ay = (float)(h * vy), az = (float)(h * vz);
                        x[p] = new Vector3((float)(x[p].x + ax), (float)(x[p].y + ay), (float)(x[p].z + az));
                    }
                }
                for (long k = 0; k < orderId.LongLength; ++k)
                {
                    int id = orderId[k];
                    switch (orderType[k])
                    {
                        case 0: ProjectDistance(x, w, sb.distanceIJ[2 * id], sb.distanceIJ[2 * id + 1], sb.distanceRest[id], atD); break;
                        case 1: ProjectVolume(x, w, sb.volumeIJKL, 4 * id, (float)(6.0f * sb.volumeRest[id]), atV); break;
                        default: ProjectBending(x, w, sb.bendingIJKL, 4 * id, sb.bendingRestCosSin[2 * id], sb.bendingRestCosSin[2 * id + 1], atB); break;
                    }
                }
                if (sb.GroundPlane)   // SPEC.md §2 step 2b
                {
                    Vector3 pn = sb.GroundNormal; float pd = sb.GroundOffset;
                    for (int p = 0; p < n; ++p)
                    {
                        if (!(w[p] > 0f)) continue;
                        float a = (float)(pn.x * x[p].x), b = (float)(pn.y * x[p].y), c = (float)(pn.z * x[p].z);
                        float pen = (float)((float)((float)(a + b) + c) - pd);
                        if (pen < 0f)
                            x[p] = new Vector3((float)(x[p].x - (float)(pen * pn.x)), (float)(x[p].y - (float)(pen * pn.y)), (float)(x[p].z - (float)(pen * pn.z)));
                    }
                }
                for (int p = 0; p < n; ++p)
                {
                    float dx = (float)(x[p].x - prev[p].x), dy = (float)(x[p].y - prev[p].y), dz = (float)(x[p].z - prev[p].z);
                    float qx = (float)(dx * invH), qy = (float)(dy * invH), qz = (float)(dz * invH);
                    v[p] = new Vector3((float)(qx * kd), (float)(qy * kd), (float)(qz * kd));
                }
            }
        }

        // SPEC.md 2c: impulses between two ticks, items in list order, velocities only. SURFACE items act against `tri` (particle indices:
        // the CPU branch has no embedding); the validation is the plugin's (softbody.h), here as exceptions before anything is applied.
        public void ApplyImpulses(SbImpulse[] items, int count, int[] tri)
        {
            Vector3[] x = sb.positions; Vector3[] v = sb.velocities; float[] w = sb.inverseMass;
            int n = x.Length, m = tri != null ? tri.Length / 3 : 0;
            for (int i = 0; i < count; ++i)
            {
                SbImpulse it = items[i];
                bool radial = it.kind == SoftbodyNative.SB_IMPULSE_RADIAL;
                if (it.kind < 0 || it.kind > 2 || (it.flags & ~3u) != 0 || it.reserved0 != 0 || it.reserved1 != 0) throw new ArgumentException("impulse: unknown kind or flag bit, or reserved not 0");
                if ((it.flags & SoftbodyNative.SB_IMPULSE_LINEAR_FALLOFF) != 0 && !radial) throw new ArgumentException("impulse: linear falloff on a non-radial item");
                if (!Finite(it.vecX) || !Finite(it.vecY) || !Finite(it.vecZ)) throw new ArgumentException("impulse: NaN or infinite vec");
                if (it.kind == SoftbodyNative.SB_IMPULSE_PARTICLE && (it.index < 0 || it.index >= n)) throw new ArgumentException("impulse: particle index out of range");
                if (it.kind == SoftbodyNative.SB_IMPULSE_SURFACE)
                {
                    if (m == 0) throw new InvalidOperationException("impulse: a SURFACE item while no triangle list is in force");
                    if (it.index < -1 || it.index >= m) throw new ArgumentException("impulse: triangle index out of range");
                    if (it.index >= 0 && (!Finite(it.u) || !Finite(it.v))) throw new ArgumentException("impulse: NaN or infinite barycentric coordinate");
                }
                if (radial && (!(it.radius > 0f) || !Finite(it.strength))) throw new ArgumentException("impulse: radius must be positive, strength finite");
            }
            for (int i = 0; i < count; ++i)
            {
                SbImpulse it = items[i];
                bool vc = (it.flags & SoftbodyNative.SB_IMPULSE_VELOCITY_CHANGE) != 0;
                if (it.kind == SoftbodyNative.SB_IMPULSE_PARTICLE) Entry(v, w, it.index, it.vecX, it.vecY, it.vecZ, vc);
                else if (it.kind == SoftbodyNative.SB_IMPULSE_SURFACE)
                {
                    if (it.index < 0) continue;
                    float b0 = (float)(1.0f - it.u); b0 = (float)(b0 - it.v);
                    Entry(v, w, tri[3 * it.index], (float)(b0 * it.vecX), (float)(b0 * it.vecY), (float)(b0 * it.vecZ), vc);
                    Entry(v, w, tri[3 * it.index + 1], (float)(it.u * it.vecX), (float)(it.u * it.vecY), (float)(it.u * it.vecZ), vc);
                    Entry(v, w, tri[3 * it.index + 2], (float)(it.v * it.vecX), (float)(it.v * it.vecY), (float)(it.v * it.vecZ), vc);
                }
                else
                {
                    float R2 = (float)(it.radius * it.radius);
                    bool falloff = (it.flags & SoftbodyNative.SB_IMPULSE_LINEAR_FALLOFF) != 0;
                    for (int p = 0; p < n; ++p)
                    {
                        float dx = (float)(x[p].x - it.vecX), dy = (float)(x[p].y - it.vecY), dz = (float)(x[p].z - it.vecZ);
                        float xx = (float)(dx * dx), yy = (float)(dy * dy), zz = (float)(dz * dz);
                        float r2 = (float)((float)(xx + yy) + zz);
                        if (!(w[p] > 0f && 0f < r2 && r2 <= R2 && r2 < float.PositiveInfinity)) continue;      // NaN compares false; the centre has no direction
                        float r = (float)Math.Sqrt(r2);      // (the double root of a float, rounded once more, is the correctly rounded float root)
                        float f = it.strength;
                        if (falloff) { float q = (float)(r / it.radius); float g = (float)(1.0f - q); f = (float)(it.strength * g); }
                        float we = vc ? 1.0f : w[p];
                        float s = (float)(we * f);
                        float nx = (float)(dx / r), ny = (float)(dy / r), nz = (float)(dz / r);
                        float ax = (float)(s * nx), ay = (float)(s * ny), az = (float)(s * nz);
                        v[p] = new Vector3(Canonical((float)(v[p].x + ax)), Canonical((float)(v[p].y + ay)), Canonical((float)(v[p].z + az)));
                    }
                }
            }
        }

        // SPEC.md 2e: wind, air drag and pressure on the render triangles `tri` (particle indices) between two ticks, velocities only. Phase 1
        // computes every triangle's J from the state as it is before the call, phase 2 adds them per particle in ascending triangle order,
        // once per corner slot. The validation is the plugin's (softbody_group.h), here as exceptions before anything is applied.
        public void ApplySurfaceForces(SbSurfaceForce f, int[] tri)
        {
            Vector3[] x = sb.positions; Vector3[] v = sb.velocities; float[] w = sb.inverseMass;
            int n = x.Length, m = tri != null ? tri.Length / 3 : 0;
            if (f.flags != 0 || f.reserved0 != 0 || f.reserved1 != 0 || f.reserved2 != 0) throw new ArgumentException("surface force: flags and reserved must be 0");
            if (!Finite(f.windX) || !Finite(f.windY) || !Finite(f.windZ) || !Finite(f.normal) || !Finite(f.tangential) || !Finite(f.pressure) || !Finite(f.dt))
                throw new ArgumentException("surface force: NaN or infinite value");
            if (f.normal < 0f || f.tangential < 0f || !(f.dt > 0f)) throw new ArgumentException("surface force: normal and tangential must not be negative, dt must be positive");
            if (m == 0) throw new InvalidOperationException("surface force: no render triangles are set");
            float hn = (float)((float)(f.dt * f.normal) / 6.0f), ht = (float)((float)(f.dt * f.tangential) / 6.0f), hp = (float)((float)(f.dt * f.pressure) / 6.0f);
            var J = new Vector3[m];
            var skipped = new bool[m];
            for (int t = 0; t < m; ++t)
            {
                int a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
                float e1x = (float)(x[b].x - x[a].x), e1y = (float)(x[b].y - x[a].y), e1z = (float)(x[b].z - x[a].z);
                float e2x = (float)(x[c].x - x[a].x), e2y = (float)(x[c].y - x[a].y), e2z = (float)(x[c].z - x[a].z);
                float fx = (float)((float)(e1y * e2z) - (float)(e1z * e2y)), fy = (float)((float)(e1z * e2x) - (float)(e1x * e2z)), fz = (float)((float)(e1x * e2y) - (float)(e1y * e2x));
                float L2 = (float)((float)((float)(fx * fx) + (float)(fy * fy)) + (float)(fz * fz));
                if (!(L2 >= 1.262177448e-29f) || !(L2 < float.PositiveInfinity)) { skipped[t] = true; continue; }      // 0x1p-96f
                float L = (float)Math.Sqrt(L2);      // (the double root of a float, rounded once more, is the correctly rounded float root)
                float ux = (float)(f.windX - (float)((float)((float)(v[a].x + v[b].x) + v[c].x) / 3.0f));
                float uy = (float)(f.windY - (float)((float)((float)(v[a].y + v[b].y) + v[c].y) / 3.0f));
                float uz = (float)(f.windZ - (float)((float)((float)(v[a].z + v[b].z) + v[c].z) / 3.0f));
                float uf = (float)((float)((float)(ux * fx) + (float)(uy * fy)) + (float)(uz * fz));
                float q = (float)(uf / L2);
                float unx = (float)(q * fx), uny = (float)(q * fy), unz = (float)(q * fz);
                float utx = (float)(ux - unx), uty = (float)(uy - uny), utz = (float)(uz - unz);
                J[t] = new Vector3((float)((float)(L * (float)((float)(hn * unx) + (float)(ht * utx))) + (float)(hp * fx)),
                                   (float)((float)(L * (float)((float)(hn * uny) + (float)(ht * uty))) + (float)(hp * fy)),
                                   (float)((float)(L * (float)((float)(hn * unz) + (float)(ht * utz))) + (float)(hp * fz)));
            }
            var G = new Vector3[n];
            var met = new bool[n];
            for (int t = 0; t < m; ++t)
            {
                if (skipped[t]) continue;
                for (int k = 0; k < 3; ++k)
                {
                    int p = tri[3 * t + k];
                    G[p] = new Vector3((float)(G[p].x + J[t].x), (float)(G[p].y + J[t].y), (float)(G[p].z + J[t].z));
                    met[p] = true;
                }
            }
            for (int p = 0; p < n; ++p)
            {
                if (!met[p] || !(w[p] > 0f)) continue;
                float ax = (float)(w[p] * G[p].x), ay = (float)(w[p] * G[p].y), az = (float)(w[p] * G[p].z);
                v[p] = new Vector3(Canonical((float)(v[p].x + ax)), Canonical((float)(v[p].y + ay)), Canonical((float)(v[p].z + az)));
            }
        }

        // SPEC.md 6g: the nearest point of the triangles `tri` (indices into `p`) to q, the sequential loop -- per triangle the Voronoi-region
        // chain, the first test that holds deciding (u, v); a candidate iff dd <= maxDistance^2 and dd is finite; the smallest dd wins, among
        // equal ones the first triangle. A miss: triangle = -1, distance = u = v = 0. The validation is the plugin's (softbody_group.h).
        public static SbClosestHit ClosestPoint(Vector3[] p, int[] tri, Vector3 q, float maxDistance)
        {
            if (!Finite(q.x) || !Finite(q.y) || !Finite(q.z)) throw new ArgumentException("closest point: NaN or infinite coordinate");
            if (!(maxDistance >= 0f)) throw new ArgumentException("closest point: max_distance is NaN or negative");
            int m = tri != null ? tri.Length / 3 : 0;
            float R2 = (float)(maxDistance * maxDistance);
            var best = new SbClosestHit { triangle = -1 };
            float bestDd = 0f;
            for (int t = 0; t < m; ++t)
            {
                Vector3 pa = p[tri[3 * t]], pb = p[tri[3 * t + 1]], pc = p[tri[3 * t + 2]];
                F3 ab = Sub(pb, pa), ac = Sub(pc, pa), ap = Sub(q, pa), bp = Sub(q, pb), cp = Sub(q, pc);
                float d1 = Dot(ab, ap), d2 = Dot(ac, ap), d3 = Dot(ab, bp), d4 = Dot(ac, bp), d5 = Dot(ab, cp), d6 = Dot(ac, cp);
                float vc = (float)((float)(d1 * d4) - (float)(d3 * d2)), vb = (float)((float)(d5 * d2) - (float)(d1 * d6)), va = (float)((float)(d3 * d6) - (float)(d5 * d4));
                float e = (float)(d4 - d3), f = (float)(d5 - d6);
                float u, v;
                if (d1 <= 0f && d2 <= 0f) { u = 0f; v = 0f; }
                else if (d3 >= 0f && d4 <= d3) { u = 1f; v = 0f; }
                else if (vc <= 0f && d1 >= 0f && d3 <= 0f) { u = (float)(d1 / (float)(d1 - d3)); v = 0f; }
                else if (d6 >= 0f && d5 <= d6) { u = 0f; v = 1f; }
                else if (vb <= 0f && d2 >= 0f && d6 <= 0f) { u = 0f; v = (float)(d2 / (float)(d2 - d6)); }
                else if (va <= 0f && e >= 0f && f >= 0f) { float w = (float)(e / (float)(e + f)); u = (float)(1.0f - w); v = w; }
                else { float den = (float)(1.0f / (float)((float)(va + vb) + vc)); u = (float)(vb * den); v = (float)(vc * den); }
                float cx = (float)(pa.x + (float)((float)(u * ab.x) + (float)(v * ac.x)));
                float cy = (float)(pa.y + (float)((float)(u * ab.y) + (float)(v * ac.y)));
                float cz = (float)(pa.z + (float)((float)(u * ab.z) + (float)(v * ac.z)));
                F3 r = new F3((float)(q.x - cx), (float)(q.y - cy), (float)(q.z - cz));
                float dd = Dot(r, r);
                if (!(dd <= R2 && dd < float.PositiveInfinity)) continue;
                if (best.triangle < 0 || dd < bestDd) { best.triangle = t; best.u = u; best.v = v; bestDd = dd; }
            }
            if (best.triangle >= 0) best.distance = (float)Math.Sqrt(bestDd);      // (the double root of a float, rounded once more, is the correctly rounded float root)
            return best;
        }

        static bool Finite(float f) { return !(float.IsNaN(f) || float.IsInfinity(f)); }

        // v_p.c = v_p.c + (we_p * G.c); a pinned particle is skipped
        static void Entry(Vector3[] v, float[] w, int p, float gx, float gy, float gz, bool velocityChange)
        {
            if (w[p] == 0f) return;
            float we = velocityChange ? 1.0f : w[p];
            float ax = (float)(we * gx), ay = (float)(we * gy), az = (float)(we * gz);
            v[p] = new Vector3(Canonical((float)(v[p].x + ax)), Canonical((float)(v[p].y + ay)), Canonical((float)(v[p].z + az)));
        }

        // SPEC.md 2c: a NaN that comes out of an impulse's addition is the canonical quiet NaN 0x7fc00000
        static float Canonical(float f) { return float.IsNaN(f) ? BitConverter.ToSingle(BitConverter.GetBytes(0x7fc00000), 0) : f; }

        // SPEC.md §4
        static void ProjectDistance(Vector3[] x, float[] w, int i, int j, float L0, float at)
        {
            float wi = w[i], wj = w[j];
            float dx = (float)(x[i].x - x[j].x), dy = (float)(x[i].y - x[j].y), dz = (float)(x[i].z - x[j].z);
            float xx = (float)(dx * dx), yy = (float)(dy * dy), zz = (float)(dz * dz);
            float L2 = (float)((float)(xx + yy) + zz);
            float ws = (float)((float)(wi + wj) + at);
            if (!(L2 >= 1.262177448e-29f) || !(ws > 0f)) return;   // 2^-96 (SPEC.md §4): coincident endpoints give no direction
            float L = (float)Math.Sqrt(L2);        // sqrt of a float in double, rounded to float == correctly rounded sqrtf
            float C = (float)(L - L0);
            float wl = (float)(ws * L);
            float s = (float)((-C) / wl);
            float si = (float)(wi * s), sj = (float)(wj * s);
            float ax = (float)(si * dx), ay = (float)(si * dy), az = (float)(si * dz);
            float bx = (float)(sj * dx), by = (float)(sj * dy), bz = (float)(sj * dz);
            x[i] = new Vector3((float)(x[i].x + ax), (float)(x[i].y + ay), (float)(x[i].z + az));
            x[j] = new Vector3((float)(x[j].x - bx), (float)(x[j].y - by), (float)(x[j].z - bz));
        }

        struct F3 { public float x, y, z; public F3(float a, float b, float c) { x = a; y = b; z = c; } }
        static F3 Sub(Vector3 a, Vector3 b) => new F3((float)(a.x - b.x), (float)(a.y - b.y), (float)(a.z - b.z));
        static F3 Cross(F3 a, F3 b)
        {
            float t0 = (float)(a.y * b.z), t1 = (float)(a.z * b.y), t2 = (float)(a.z * b.x);
            float t3 = (float)(a.x * b.z), t4 = (float)(a.x * b.y), t5 = (float)(a.y * b.x);
            return new F3((float)(t0 - t1), (float)(t2 - t3), (float)(t4 - t5));
        }
        static float Dot(F3 a, F3 b)
        {
            float xx = (float)(a.x * b.x), yy = (float)(a.y * b.y), zz = (float)(a.z * b.z);
            return (float)((float)(xx + yy) + zz);
        }
        static Vector3 AddScaled(Vector3 p, float s, F3 g)
        {
            float a = (float)(s * g.x), b = (float)(s * g.y), c = (float)(s * g.z);
            return new Vector3((float)(p.x + a), (float)(p.y + b), (float)(p.z + c));
        }

        // SPEC.md §5
        static void ProjectVolume(Vector3[] x, float[] w, int[] q, int o, float R6, float atV)
        {
            int i0 = q[o], i1 = q[o + 1], i2 = q[o + 2], i3 = q[o + 3];
            F3 e1 = Sub(x[i1], x[i0]), e2 = Sub(x[i2], x[i0]), e3 = Sub(x[i3], x[i0]);
            F3 g1 = Cross(e2, e3), g2 = Cross(e3, e1), g3 = Cross(e1, e2);
            F3 g0 = new F3(-(float)((float)(g1.x + g2.x) + g3.x), -(float)((float)(g1.y + g2.y) + g3.y), -(float)((float)(g1.z + g2.z) + g3.z));
            float C6 = (float)(Dot(e1, g1) - R6);
            float a0 = (float)(w[i0] * Dot(g0, g0)), a1 = (float)(w[i1] * Dot(g1, g1)), a2 = (float)(w[i2] * Dot(g2, g2)), a3 = (float)(w[i3] * Dot(g3, g3));
            float den = (float)((float)((float)((float)(a0 + a1) + a2) + a3) + atV);
            if (!(den > 0f)) return;
            float s = (float)((-C6) / den);
            x[i0] = AddScaled(x[i0], (float)(w[i0] * s), g0); x[i1] = AddScaled(x[i1], (float)(w[i1] * s), g1);
            x[i2] = AddScaled(x[i2], (float)(w[i2] * s), g2); x[i3] = AddScaled(x[i3], (float)(w[i3] * s), g3);
        }

        // SPEC.md §6
        static void ProjectBending(Vector3[] x, float[] w, int[] q, int o, float c0, float s0, float atB)
        {
            int ia = q[o], ib = q[o + 1], ic = q[o + 2], id = q[o + 3];
            F3 e = Sub(x[ib], x[ia]);
            float el = (float)Math.Sqrt(Dot(e, e));
            F3 ac = Sub(x[ia], x[ic]), bc = Sub(x[ib], x[ic]), bd = Sub(x[ib], x[id]), ad = Sub(x[ia], x[id]);
            F3 n1 = Cross(ac, bc), n2 = Cross(bd, ad);
            float q1 = Dot(n1, n1), q2 = Dot(n2, n2);
            if (!(el > 0f) || !(q1 > 0f) || !(q2 > 0f)) return;
            F3 m1 = new F3((float)(n1.x / q1), (float)(n1.y / q1), (float)(n1.z / q1));
            F3 m2 = new F3((float)(n2.x / q2), (float)(n2.y / q2), (float)(n2.z / q2));
            F3 gc = new F3((float)(el * m1.x), (float)(el * m1.y), (float)(el * m1.z));
            F3 gd = new F3((float)(el * m2.x), (float)(el * m2.y), (float)(el * m2.z));
            F3 cb = Sub(x[ic], x[ib]), db = Sub(x[id], x[ib]);
            float ta1 = (float)(Dot(cb, e) / el), ta2 = (float)(Dot(db, e) / el);
            float tb1 = (float)(Dot(ac, e) / el), tb2 = (float)(Dot(ad, e) / el);
            F3 ga = new F3((float)((float)(ta1 * m1.x) + (float)(ta2 * m2.x)), (float)((float)(ta1 * m1.y) + (float)(ta2 * m2.y)), (float)((float)(ta1 * m1.z) + (float)(ta2 * m2.z)));
            F3 gb = new F3((float)((float)(tb1 * m1.x) + (float)(tb2 * m2.x)), (float)((float)(tb1 * m1.y) + (float)(tb2 * m2.y)), (float)((float)(tb1 * m1.z) + (float)(tb2 * m2.z)));
            float s1 = (float)Math.Sqrt(q1), s2 = (float)Math.Sqrt(q2);
            F3 u1 = new F3((float)(n1.x / s1), (float)(n1.y / s1), (float)(n1.z / s1));
            F3 u2 = new F3((float)(n2.x / s2), (float)(n2.y / s2), (float)(n2.z / s2));
            float cs = Dot(u1, u2);
            float sn = -(float)(Dot(Cross(u1, u2), e) / el);
            float C = (float)((float)(sn * c0) - (float)(cs * s0));
            float a0 = (float)(w[ia] * Dot(ga, ga)), a1 = (float)(w[ib] * Dot(gb, gb)), a2 = (float)(w[ic] * Dot(gc, gc)), a3 = (float)(w[id] * Dot(gd, gd));
            float den = (float)((float)((float)((float)(a0 + a1) + a2) + a3) + atB);
            if (!(den > 0f)) return;
            float s = (float)((-C) / den);
            x[ia] = AddScaled(x[ia], (float)(w[ia] * s), ga); x[ib] = AddScaled(x[ib], (float)(w[ib] * s), gb);
            x[ic] = AddScaled(x[ic], (float)(w[ic] * s), gc); x[id] = AddScaled(x[id], (float)(w[id] * s), gd);
        }
    }
}
