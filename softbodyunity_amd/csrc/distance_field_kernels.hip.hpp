// distance_field_kernels.hip.hpp — contacts with a signed-distance volume between two ticks (SPEC.md 2i): one streaming pass that pushes every
// particle a rank holds out of a prop baked into a 3-D table of distances, along the analytic gradient of the table's trilinear
// interpolation, and gives it 2f's velocity response against a collider moving with the call's pose, in binary32 without FMA, in the order
// SPEC.md 2i parenthesises. Included by distance_field.hip alone.
//
// Code object (gfx950, the compiler's resource usage): 72 VGPRs, 70 SGPRs, no scratch, no LDS, 7 waves per SIMD.
#pragma once
#include "contact_response.hip.hpp"

namespace sbk {

// What the kernel reads of an sb_distance_field and of the call's sb_distance_field_pose, as kernel arguments (uniform for the grid:
// scalar loads)
struct DistanceFieldArgs {
    float a[3], rot[9], cell[3];
    int32_t nx, ny, nz;
    float offset, thickness, lin[3], ang[3], friction, restitution;
};

// Where a point is in the volume: false when it is outside the footprint (a NaN compares false). base: the flat index of sample
// (i0, i1, i2), the cell's corner; t: where the point is in that cell. 0 <= f_k <= n_k - 1 <= 1023, so the conversion is exact and
// 0 <= i_k <= n_k - 2: the cell's far corner, base + nx ny + nx + 1, is at most sample nx ny nz - 1.
__device__ __forceinline__ bool distance_field_locate(const DistanceFieldArgs &D, float x, float y, float z, int &base, float (&t)[3]) {
    const float ex = x - D.a[0], ey = y - D.a[1], ez = z - D.a[2];
    float f[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float a = ex * D.rot[3 * k], b = ey * D.rot[3 * k + 1], c = ez * D.rot[3 * k + 2];
        const float ab = a + b;
        const float q = ab + c;
        f[k] = q / D.cell[k];
    }
    const float m0 = (float)(D.nx - 1), m1 = (float)(D.ny - 1), m2 = (float)(D.nz - 1);
    if (!(f[0] >= 0.0f && f[0] <= m0 && f[1] >= 0.0f && f[1] <= m1 && f[2] >= 0.0f && f[2] <= m2)) return false;
    int i0 = (int)f[0], i1 = (int)f[1], i2 = (int)f[2];
    i0 = i0 > D.nx - 2 ? D.nx - 2 : i0;
    i1 = i1 > D.ny - 2 ? D.ny - 2 : i1;
    i2 = i2 > D.nz - 2 ? D.nz - 2 : i2;
    t[0] = f[0] - (float)i0;
    t[1] = f[1] - (float)i1;
    t[2] = f[2] - (float)i2;
    base = (i2 * D.ny + i1) * D.nx + i0;      // (< nx ny nz <= 2^27)
    return true;
}

// The two samples of an x-pair are side by side in memory: one 8-byte load (the pair's address is a multiple of 4, not of 8)
struct DistanceFieldPair { float lo, hi; };

// A cell's eight samples as four x-pairs, pair j = b + 2 c holding d_0bc and d_1bc
__device__ __forceinline__ void distance_field_gather(const DistanceFieldArgs &D, const float *__restrict__ s, int base, DistanceFieldPair (&d)[4]) {
    const float *p = s + base;
    const int row = D.nx, slab = D.nx * D.ny;
    d[0] = *reinterpret_cast<const DistanceFieldPair *>(p);
    d[1] = *reinterpret_cast<const DistanceFieldPair *>(p + row);
    d[2] = *reinterpret_cast<const DistanceFieldPair *>(p + slab);
    d[3] = *reinterpret_cast<const DistanceFieldPair *>(p + slab + row);
}

// (hit, n, depth) from the cell's eight samples: lerps p + t (r - p) in the order x, y, z, and the gradient from the same intermediates.
// The divisions by cell, the square root and the divisions by len only where 0 < gap < thickness.
__device__ __forceinline__ bool distance_field_contact(const DistanceFieldArgs &D, const float (&t)[3], const DistanceFieldPair (&d)[4], float (&n)[3], float &depth) {
    float dx[4], e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        dx[j] = d[j].hi - d[j].lo;
        const float p = t[0] * dx[j];
        e[j] = d[j].lo + p;
    }
    float dy[2], g[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        dy[c] = e[2 * c + 1] - e[2 * c];
        const float p = t[1] * dy[c];
        g[c] = e[2 * c] + p;
    }
    const float dz = g[1] - g[0];
    const float pz = t[2] * dz;
    const float phi = g[0] + pz;
    const float gap = D.offset - phi;
    if (!(gap > 0.0f && gap < D.thickness)) return false;      // (a NaN or infinite phi compares false)
    float hx[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float dd = dx[2 * c + 1] - dx[2 * c];
        const float p = t[1] * dd;
        hx[c] = dx[2 * c] + p;
    }
    const float hd = hx[1] - hx[0], yd = dy[1] - dy[0];
    const float hp = t[2] * hd, yp = t[2] * yd;
    const float h0 = hx[0] + hp, y0 = dy[0] + yp;
    const float G0 = h0 / D.cell[0], G1 = y0 / D.cell[1], G2 = dz / D.cell[2];
    const float g00 = G0 * G0, g11 = G1 * G1, g22 = G2 * G2;
    const float g01 = g00 + g11;
    const float l2 = g01 + g22;
    const float len = sqrtf(l2);
    if (!(len > 0.0f)) return false;                            // a constant cell has no direction to push along
    const float m0 = G0 / len, m1 = G1 / len, m2 = G2 / len;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = m0 * D.rot[c], b = m1 * D.rot[3 + c], e2 = m2 * D.rot[6 + c];
        const float ab = a + b;
        n[c] = ab + e2;
    }
    depth = gap;
    return true;
}

constexpr int kDistanceFieldLanes = 256, kDistanceFieldPerLane = 4;      // 1 024 particles per workgroup

// heightfield_kernel's access shape: a lane takes FOUR consecutive particles = one aligned 16-byte word of w, read first (four pinned
// particles read nothing more), and three of x; the last n mod 4 particles take one lane each, word by word. Descriptor and pose are
// uniform (scalar registers). A lane with no particle inside the footprint returns before any gather; otherwise the sixteen 8-byte loads
// of its four particles are issued together, before the first use -- a particle that needs none reads cell 0, which every lane of the
// grid shares -- and only a lane with a hit reads velocities. Stored are the 16-byte words a contact changed: an untouched body costs
// 12 + 4 bytes per particle and keeps every bit. No LDS, no atomics, no scratch: a lane writes only words it read. The waves-per-SIMD hint
// is a register budget, as the heightfield's: under a budget for 4 waves the four particles' thirty-two samples and their lerps take 80
// VGPRs (6 waves per SIMD), under this one 72 (7 waves); a budget for 8 waves spills 52 bytes per lane to scratch, so four particles
// at a time stop here.
__global__ __launch_bounds__(kDistanceFieldLanes) __attribute__((amdgpu_waves_per_eu(6))) void distance_field_kernel(float *pos, float *vel, const float *wf, int64_t n, DistanceFieldArgs D, const float *__restrict__ s) {
    ColliderRec C = {};
    C.a[0] = D.a[0]; C.a[1] = D.a[1]; C.a[2] = D.a[2];
    C.lin[0] = D.lin[0]; C.lin[1] = D.lin[1]; C.lin[2] = D.lin[2];
    C.ang[0] = D.ang[0]; C.ang[1] = D.ang[1]; C.ang[2] = D.ang[2];
    C.friction = D.friction; C.restitution = D.restitution;
    const int64_t k = (int64_t)blockIdx.x * kDistanceFieldLanes + threadIdx.x;
    const int64_t n4 = n / kDistanceFieldPerLane;
    if (k < n4) {
        uint4 *px = reinterpret_cast<uint4 *>(pos) + 3 * k, *pv = reinterpret_cast<uint4 *>(vel) + 3 * k;
        const float4 W = reinterpret_cast<const float4 *>(wf)[k];
        const float w[4] = {W.x, W.y, W.z, W.w};
        if (!(W.x > 0.0f || W.y > 0.0f || W.z > 0.0f || W.w > 0.0f)) return;      // four pinned particles: nothing to read
        uint32_t x[12];
        {
            const uint4 a = px[0], b = px[1], c = px[2];
            x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w; x[8] = c.x; x[9] = c.y; x[10] = c.z; x[11] = c.w;
        }
        bool in[4];
        int base[4];
        float t[4][3];
#pragma unroll
        for (int j = 0; j < kDistanceFieldPerLane; ++j) {
            base[j] = 0; t[j][0] = t[j][1] = t[j][2] = 0.0f;
            in[j] = w[j] > 0.0f && distance_field_locate(D, __uint_as_float(x[3 * j]), __uint_as_float(x[3 * j + 1]), __uint_as_float(x[3 * j + 2]), base[j], t[j]);
        }
        if (!(in[0] || in[1] || in[2] || in[3])) return;
        DistanceFieldPair d[4][4];
#pragma unroll
        for (int j = 0; j < kDistanceFieldPerLane; ++j) distance_field_gather(D, s, in[j] ? base[j] : 0, d[j]);      // (cell 0 exists: nx, ny, nz >= 2)
        float nrm[4][3], depth[4];
        bool hit[4];
#pragma unroll
        for (int j = 0; j < kDistanceFieldPerLane; ++j) hit[j] = in[j] && distance_field_contact(D, t[j], d[j], nrm[j], depth[j]);
        if (!(hit[0] || hit[1] || hit[2] || hit[3])) return;
        uint32_t v[12];
        {
            const uint4 a = pv[0], b = pv[1], c = pv[2];
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w; v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
        }
        unsigned wrote_x = 0, wrote_v = 0;      // bit j: particle j of the lane
#pragma unroll
        for (int j = 0; j < kDistanceFieldPerLane; ++j) {
            if (!hit[j]) continue;
            uint32_t xj[3] = {x[3 * j], x[3 * j + 1], x[3 * j + 2]}, vj[3] = {v[3 * j], v[3 * j + 1], v[3 * j + 2]};
            const bool wv = collide_respond(C, nrm[j], depth[j], xj, vj);
            wrote_x |= 1u << j;
#pragma unroll
            for (int c = 0; c < 3; ++c) x[3 * j + c] = xj[c];
            if (wv) {
                wrote_v |= 1u << j;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[3 * j + c] = vj[c];
            }
        }
        // word 0 holds particles 0 and 1 (floats 0..3), word 1 particles 1 and 2, word 2 particles 2 and 3
        if (wrote_x & 0x3u) collide_store4(px, x[0], x[1], x[2], x[3]);
        if (wrote_x & 0x6u) collide_store4(px + 1, x[4], x[5], x[6], x[7]);
        if (wrote_x & 0xcu) collide_store4(px + 2, x[8], x[9], x[10], x[11]);
        if (wrote_v & 0x3u) collide_store4(pv, v[0], v[1], v[2], v[3]);
        if (wrote_v & 0x6u) collide_store4(pv + 1, v[4], v[5], v[6], v[7]);
        if (wrote_v & 0xcu) collide_store4(pv + 2, v[8], v[9], v[10], v[11]);
        return;
    }
    const int64_t p = n4 * kDistanceFieldPerLane + (k - n4);
    if (p >= n) return;
    const float w = wf[p];
    if (!(w > 0.0f)) return;
    uint32_t *xs = reinterpret_cast<uint32_t *>(pos) + 3 * p, *vs = reinterpret_cast<uint32_t *>(vel) + 3 * p;
    uint32_t x[3] = {xs[0], xs[1], xs[2]};
    int base = 0;
    float t[3] = {0.0f, 0.0f, 0.0f};
    if (!distance_field_locate(D, __uint_as_float(x[0]), __uint_as_float(x[1]), __uint_as_float(x[2]), base, t)) return;
    DistanceFieldPair d[4];
    distance_field_gather(D, s, base, d);
    float nrm[3], depth;
    if (!distance_field_contact(D, t, d, nrm, depth)) return;
    uint32_t v[3] = {vs[0], vs[1], vs[2]};
    const bool wv = collide_respond(C, nrm, depth, x, v);
    xs[0] = x[0]; xs[1] = x[1]; xs[2] = x[2];
    if (wv) { vs[0] = v[0]; vs[1] = v[1]; vs[2] = v[2]; }
}

}  // namespace sbk
