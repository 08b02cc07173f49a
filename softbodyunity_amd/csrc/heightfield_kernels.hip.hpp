// heightfield_kernels.hip.hpp — contacts with a terrain heightfield between two ticks (SPEC.md 2h): one streaming pass that lifts every
// particle a rank holds out of the ground under a height map and gives it 2f's velocity response against a collider at rest, in binary32
// without FMA, in the order SPEC.md 2h parenthesises. Included by heightfield.hip alone.
//
// Code object (gfx950, the compiler's resource usage): 59 VGPRs, 60 SGPRs, no scratch, no LDS, 8 waves per SIMD.
#pragma once
#include "contact_response.hip.hpp"

namespace sbk {

// What the kernel reads of an sb_heightfield and of the call, as kernel arguments (uniform for the grid: scalar loads). `top` is made by
// heightfield.hip at set time from the heights alone (heightfield_top there has the bound).
struct HeightfieldArgs {
    float a[3], rot[9], cell[2];
    int32_t nx, nz;
    float thickness, top, friction, restitution;
};

// Where a point is over the grid: false when it cannot be hit without a look at the heights. q1: its height above the frame's zero
// plane; base: the index of sample (ix, iz); tx, tz: where it is in that cell.
//
// THE CULL `q1 < top`, and why it never changes a bit. A hit needs gap = height - q1 > 0, and in IEEE arithmetic (subnormals kept)
// height - q1 > 0 exactly when height > q1: the comparison is on the very q1 the rule subtracts, so rot need not be orthonormal for it.
// It is therefore enough that no finite rounded `height` exceeds top. With M the largest |h| and hmax the largest h: the exact value of
// the interpolation, for the binary32 tx and tz, is a combination of three samples whose weights are >= 0 and add up to at most
// 1 + 2^-24 (the sum tx + tz that compared <= 1 was rounded), so it is <= hmax + 2^-23 M; the six roundings on the way (sx, sz, two
// products, two sums) each err by at most 2^-24 of a value no larger than 5 M, and a product that underflows by at most 2^-150 more:
// height <= hmax + 2^-19 M + 2^-140 with room to spare, and top is that sum rounded UP to binary32 (+inf when it overflows). Where a
// difference of two samples overflows, sx or sz is infinite: then height is NaN or infinite, and so are len and depth's factor 1/len = 0
// -- depth is NaN and compares false --, so such a cell never hits, culled or not. A NaN q1 compares false here and gives a NaN gap there.
__device__ __forceinline__ bool heightfield_locate(const HeightfieldArgs &H, float x, float y, float z, float &q1, int &base, float &tx, float &tz) {
    const float ex = x - H.a[0], ey = y - H.a[1], ez = z - H.a[2];
    float q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float a = ex * H.rot[3 * k], b = ey * H.rot[3 * k + 1], c = ez * H.rot[3 * k + 2];
        const float ab = a + b;
        q[k] = ab + c;
    }
    q1 = q[1];
    if (!(q1 < H.top)) return false;
    const float fx = q[0] / H.cell[0], fz = q[2] / H.cell[1];
    const float mx = (float)(H.nx - 1), mz = (float)(H.nz - 1);
    if (!(fx >= 0.0f && fx <= mx && fz >= 0.0f && fz <= mz)) return false;      // (a NaN compares false: never hit)
    int ix = (int)fx, iz = (int)fz;
    ix = ix > H.nx - 2 ? H.nx - 2 : ix;
    iz = iz > H.nz - 2 ? H.nz - 2 : iz;
    tx = fx - (float)ix;
    tz = fz - (float)iz;
    base = iz * H.nx + ix;      // (< nx nz <= 4097^2)
    return true;
}

// (hit, n, depth) from the cell's four samples. The normal -- five divisions and the square root -- only where gap > 0.
__device__ __forceinline__ bool heightfield_contact(const HeightfieldArgs &H, float q1, float tx, float tz, float h00, float h10, float h01, float h11,
                                                    float (&n)[3], float &depth) {
    const float tt = tx + tz;
    const bool lower = tt <= 1.0f;
    const float sx = lower ? h10 - h00 : h11 - h01;
    const float sz = lower ? h01 - h00 : h11 - h10;
    const float ux = lower ? tx : 1.0f - tx, uz = lower ? tz : 1.0f - tz;
    const float px = ux * sx, pz = uz * sz;
    const float lo1 = h00 + px, up1 = h11 - px;
    const float lo2 = lo1 + pz, up2 = up1 - pz;
    const float height = lower ? lo2 : up2;
    const float gap = height - q1;
    if (!(gap > 0.0f)) return false;
    const float gx = sx / H.cell[0], gz = sz / H.cell[1];
    const float gxx = gx * gx, gzz = gz * gz;
    const float g1 = gxx + 1.0f;
    const float l2 = g1 + gzz;
    const float len = sqrtf(l2);
    const float m0 = (-gx) / len, m1 = 1.0f / len, m2 = (-gz) / len;
    depth = gap * m1;
    if (!(depth < H.thickness)) return false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = m0 * H.rot[c], b = m1 * H.rot[3 + c], e = m2 * H.rot[6 + c];
        const float ab = a + b;
        n[c] = ab + e;
    }
    return true;
}

constexpr int kHeightfieldLanes = 256, kHeightfieldPerLane = 4;      // 1 024 particles per workgroup

// collide_kernel's access shape: a lane takes FOUR consecutive particles = one aligned 16-byte word of w, read first (four pinned
// particles read nothing more), and three of x; the last n mod 4 particles take one lane each, word by word. The descriptor is uniform
// (scalar registers); a lane that has a particle over the grid and under `top` gathers that particle's four samples -- the sixteen loads
// of a lane are issued together, before the first use; a particle that needs none reads sample 0's cell, which every lane of the grid
// shares -- and only a lane with a hit reads velocities. Stored are the 16-byte words a contact changed: an untouched body costs
// 12 + 4 bytes per particle and keeps every bit. The collider of 2f's response is at rest (lin = ang = 0: the products with 0 stay, they
// make the NaN the rule makes of an infinite x'). No LDS, no atomics, no scratch: a lane writes only words it read. The waves-per-SIMD
// hint is a register budget: without it the scheduler spreads the four particles' divisions over 100 VGPRs (4 waves per SIMD); with it
// the same statements take 59, still without scratch.
__global__ __launch_bounds__(kHeightfieldLanes) __attribute__((amdgpu_waves_per_eu(6))) void heightfield_kernel(float *pos, float *vel, const float *wf, int64_t n, HeightfieldArgs H, const float *__restrict__ h) {
    ColliderRec C = {};
    C.a[0] = H.a[0]; C.a[1] = H.a[1]; C.a[2] = H.a[2];
    C.friction = H.friction; C.restitution = H.restitution;
    const int64_t k = (int64_t)blockIdx.x * kHeightfieldLanes + threadIdx.x;
    const int64_t n4 = n / kHeightfieldPerLane;
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
        bool over[4];
        int base[4];
        float q1[4], tx[4], tz[4];
#pragma unroll
        for (int j = 0; j < kHeightfieldPerLane; ++j) {
            base[j] = 0; q1[j] = tx[j] = tz[j] = 0.0f;
            over[j] = w[j] > 0.0f && heightfield_locate(H, __uint_as_float(x[3 * j]), __uint_as_float(x[3 * j + 1]), __uint_as_float(x[3 * j + 2]), q1[j], base[j], tx[j], tz[j]);
        }
        if (!(over[0] || over[1] || over[2] || over[3])) return;
        float h00[4], h10[4], h01[4], h11[4];
#pragma unroll
        for (int j = 0; j < kHeightfieldPerLane; ++j) {
            const float *cell = h + (over[j] ? base[j] : 0);      // (sample 0's cell exists: nx, nz >= 2)
            h00[j] = cell[0]; h10[j] = cell[1]; h01[j] = cell[H.nx]; h11[j] = cell[H.nx + 1];
        }
        float nrm[4][3], depth[4];
        bool hit[4];
#pragma unroll
        for (int j = 0; j < kHeightfieldPerLane; ++j)
            hit[j] = over[j] && heightfield_contact(H, q1[j], tx[j], tz[j], h00[j], h10[j], h01[j], h11[j], nrm[j], depth[j]);
        if (!(hit[0] || hit[1] || hit[2] || hit[3])) return;
        uint32_t v[12];
        {
            const uint4 a = pv[0], b = pv[1], c = pv[2];
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w; v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
        }
        unsigned wrote_x = 0, wrote_v = 0;      // bit j: particle j of the lane
#pragma unroll
        for (int j = 0; j < kHeightfieldPerLane; ++j) {
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
    const int64_t p = n4 * kHeightfieldPerLane + (k - n4);
    if (p >= n) return;
    const float w = wf[p];
    if (!(w > 0.0f)) return;
    uint32_t *xs = reinterpret_cast<uint32_t *>(pos) + 3 * p, *vs = reinterpret_cast<uint32_t *>(vel) + 3 * p;
    uint32_t x[3] = {xs[0], xs[1], xs[2]};
    int base = 0;
    float q1 = 0.0f, tx = 0.0f, tz = 0.0f;
    if (!heightfield_locate(H, __uint_as_float(x[0]), __uint_as_float(x[1]), __uint_as_float(x[2]), q1, base, tx, tz)) return;
    const float *cell = h + base;
    const float h00 = cell[0], h10 = cell[1], h01 = cell[H.nx], h11 = cell[H.nx + 1];
    float nrm[3], depth;
    if (!heightfield_contact(H, q1, tx, tz, h00, h10, h01, h11, nrm, depth)) return;
    uint32_t v[3] = {vs[0], vs[1], vs[2]};
    const bool wv = collide_respond(C, nrm, depth, x, v);
    xs[0] = x[0]; xs[1] = x[1]; xs[2] = x[2];
    if (wv) { vs[0] = v[0]; vs[1] = v[1]; vs[2] = v[2]; }
}

}  // namespace sbk
