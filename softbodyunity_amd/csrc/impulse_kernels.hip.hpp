// impulse_kernels.hip.hpp — impulses between two ticks (SPEC.md 2c): the sparse kernel (PARTICLE entries and expanded SURFACE entries) and the
// radial pass. Both write velocities only, in binary32 without FMA, in the order SPEC.md 2c parenthesises. Included by impulse.hip alone.
//
// No reference counterpart exists (/root/reference/README.md:1 is the whole reference tree).
#pragma once
#include "device_math.hip.hpp"

namespace sbk {

// SPEC.md 2c: a velocity component that comes out of an impulse's addition as NaN is stored as THE quiet NaN 0x7fc00000 (IEEE 754 leaves
// the sign and payload of a NaN result to the implementation; the canonical value makes the result bit for bit everywhere).
__device__ __forceinline__ float impulse_canonical(float v) { return v == v ? v : __uint_as_float(0x7fc00000u); }

// Sparse impulses: the host sorted the entries (stably) by device particle into runs. Lane k owns particle part[k] and walks entries
// off[k] .. off[k + 1] in list order: v.c = v.c + (we * G.c), we = 1 where the entry's w word is non-zero (VELOCITY_CHANGE), else the
// particle's inverse mass. One lane per distinct particle: no atomics, the order inside a run is the list's. The tables live in mapped
// pinned host memory (a few entries per call: not worth a copy of their own).
__global__ __launch_bounds__(256) void impulse_sparse_kernel(PosView pos, float *vel, const int32_t *part, const int32_t *off, const float4 *entries, int n_runs) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_runs) return;
    const int p = part[k];
    const float w = pv_load(pos, p).w;
    if (w == 0.0f) return;                  // a pinned particle takes no impulse (a hit may land on one)
    const size_t o = 3 * (size_t)p;
    float vx = vel[o], vy = vel[o + 1], vz = vel[o + 2];
    const int e1 = off[k + 1];
    for (int e = off[k]; e < e1; ++e) {
        const float4 G = entries[e];
        const float we = __float_as_uint(G.w) != 0u ? 1.0f : w;
        const float ax = we * G.x, ay = we * G.y, az = we * G.z;
        vx = vx + ax; vy = vy + ay; vz = vz + az;
    }
    vel[o] = impulse_canonical(vx); vel[o + 1] = impulse_canonical(vy); vel[o + 2] = impulse_canonical(vz);
}

constexpr int kRadialBatch = 16;            // RADIAL items one pass applies, from its kernel arguments
struct RadialItem {
    float cx, cy, cz;
    float radius, r2max;                    // R2 = radius * radius, computed once on the host
    float strength;
    uint32_t flags;                         // SB_IMPULSE_VELOCITY_CHANGE | SB_IMPULSE_LINEAR_FALLOFF
};
struct RadialBatch {
    RadialItem item[kRadialBatch];
    int count;
};

// One pass over the owned particles: position and inverse mass of every particle (16 bytes), the velocity only of a particle some item
// reaches (12 bytes read, 12 written). Per particle the items run in item order on the running velocity -- the bits of one pass per item.
__global__ __launch_bounds__(256) void impulse_radial_kernel(PosView pos, float *vel, int64_t n_owned, RadialBatch B) {
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= n_owned) return;
    const float4 P = pv_load(pos, (int)l);
    if (!(P.w > 0.0f)) return;
    const size_t o = 3 * (size_t)l;
    float vx = 0.0f, vy = 0.0f, vz = 0.0f;
    bool loaded = false;
    for (int i = 0; i < B.count; ++i) {     // (uniform across the wave: the items sit in scalar registers)
        const RadialItem &I = B.item[i];
        const float dx = P.x - I.cx, dy = P.y - I.cy, dz = P.z - I.cz;
        const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
        const float r2 = (xx + yy) + zz;
        if (!(0.0f < r2 && r2 <= I.r2max && r2 < __builtin_inff())) continue;      // NaN compares false; the centre has no direction
        const float r = sqrtf(r2);
        float f = I.strength;
        if (I.flags & 2u) {                 // SB_IMPULSE_LINEAR_FALLOFF
            const float q = r / I.radius;
            const float g = 1.0f - q;
            f = I.strength * g;
        }
        const float we = (I.flags & 1u) ? 1.0f : P.w;      // SB_IMPULSE_VELOCITY_CHANGE
        const float s = we * f;
        if (!loaded) { vx = vel[o]; vy = vel[o + 1]; vz = vel[o + 2]; loaded = true; }
        const float nx = dx / r, ny = dy / r, nz = dz / r;
        const float ax = s * nx, ay = s * ny, az = s * nz;
        vx = vx + ax; vy = vy + ay; vz = vz + az;
    }
    if (loaded) { vel[o] = impulse_canonical(vx); vel[o + 1] = impulse_canonical(vy); vel[o + 2] = impulse_canonical(vz); }
}

}  // namespace sbk
