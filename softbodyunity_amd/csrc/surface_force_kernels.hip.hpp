// surface_force_kernels.hip.hpp — wind, air drag and pressure on the render triangles between two ticks (SPEC.md 2e): one pass over the
// triangles that stores each triangle's impulse share, one pass over the render particles that sums the shares of a particle's incident
// triangles. Both in binary32 without FMA, in the order SPEC.md 2e parenthesises; no atomics. Included by surface_force.hip alone.
#pragma once
#include "device_math.hip.hpp"

namespace sbk {

// SPEC.md 2e, "Host scalars": the wind and the three coefficients times dt / 6, computed once per call on the host
struct SurfaceForceParams {
    float wx, wy, wz;
    float hn, ht, hp;
};

constexpr uint32_t kSurfaceSkipped = 1u;    // the w word of a triangle's entry in the scratch array: 0 = J_t is valid

// SPEC.md 2c's rule, which 2e takes over: a velocity component that comes out of the addition as NaN is stored as 0x7fc00000
__device__ __forceinline__ float surface_force_canonical(float v) { return v == v ? v : __uint_as_float(0x7fc00000u); }

// Phase 1, one lane per triangle: J_t from the positions and velocities AS THEY ARE BEFORE THE CALL -- this kernel writes the scratch array
// alone, so no lane can meet a velocity the call has already changed -- and every triangle is computed once, not once per corner. The
// corners are gathered by device particle index (12 bytes each from the positions and the velocities: element-granular, served by the
// L2 for a surface whose triangles follow each other through the mesh); the entry leaves as one 16-byte store.
__global__ __launch_bounds__(256) void surface_force_triangle_kernel(PosView pos, const float *vel, const int32_t *tri, float4 *J, int m, SurfaceForceParams P) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const size_t a = 3 * (size_t)tri[3 * (size_t)t], b = 3 * (size_t)tri[3 * (size_t)t + 1], c = 3 * (size_t)tri[3 * (size_t)t + 2];
    const V3 xa = {pos.xyz[a], pos.xyz[a + 1], pos.xyz[a + 2]}, xb = {pos.xyz[b], pos.xyz[b + 1], pos.xyz[b + 2]}, xc = {pos.xyz[c], pos.xyz[c + 1], pos.xyz[c + 2]};
    const V3 e1 = sub3(xb, xa), e2 = sub3(xc, xa);
    const V3 f = cross3(e1, e2);
    const float L2 = dot3(f, f);
    if (!(L2 >= 0x1p-96f) || !(L2 < __builtin_inff())) {       // no direction (an area below 2^-49), an overflowed or a NaN area: skipped
        J[t] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(kSurfaceSkipped));
        return;
    }
    const float L = sqrtf(L2);
    const float sx = vel[a] + vel[b], sy = vel[a + 1] + vel[b + 1], sz = vel[a + 2] + vel[b + 2];
    const float tx = sx + vel[c], ty = sy + vel[c + 1], tz = sz + vel[c + 2];
    const float vtx = tx / 3.0f, vty = ty / 3.0f, vtz = tz / 3.0f;
    const V3 u = {P.wx - vtx, P.wy - vty, P.wz - vtz};
    const float uf = dot3(u, f);
    const float q = uf / L2;
    const float unx = q * f.x, uny = q * f.y, unz = q * f.z;
    const float utx = u.x - unx, uty = u.y - uny, utz = u.z - unz;
    const float nx = P.hn * unx, ny = P.hn * uny, nz = P.hn * unz;
    const float gx = P.ht * utx, gy = P.ht * uty, gz = P.ht * utz;
    const float dx = nx + gx, dy = ny + gy, dz = nz + gz;
    const float lx = L * dx, ly = L * dy, lz = L * dz;
    const float px = P.hp * f.x, py = P.hp * f.y, pz = P.hp * f.z;
    J[t] = make_float4(lx + px, ly + py, lz + pz, __uint_as_float(0u));
}

// Phase 2, one lane per render particle (part[k], device numbering): the entries off[k] .. off[k + 1] of adj name its incident triangles in
// ascending t, one entry per corner slot that names the particle. G = the sum of their J_t in that order; the particle is written iff it met
// a triangle that was not skipped and its inverse mass is positive: v.c = v.c + (w * G.c). Every other particle keeps its velocity's bits.
__global__ __launch_bounds__(256) void surface_force_vertex_kernel(PosView pos, float *vel, const int32_t *part, const int32_t *off, const int32_t *adj, const float4 *J, int n_part) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_part) return;
    const int p = part[k];
    const float w = pos.w[p];
    if (!(w > 0.0f)) return;
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    bool met = false;
    const int e1 = off[k + 1];
    for (int e = off[k]; e < e1; ++e) {
        const float4 Jt = J[adj[e]];
        if (__float_as_uint(Jt.w) != 0u) continue;
        gx = gx + Jt.x; gy = gy + Jt.y; gz = gz + Jt.z;
        met = true;
    }
    if (!met) return;
    const size_t o = 3 * (size_t)p;
    const float ax = w * gx, ay = w * gy, az = w * gz;
    const float vx = vel[o] + ax, vy = vel[o + 1] + ay, vz = vel[o + 2] + az;
    vel[o] = surface_force_canonical(vx); vel[o + 1] = surface_force_canonical(vy); vel[o + 2] = surface_force_canonical(vz);
}

}  // namespace sbk
