// collide_kernels.hip.hpp — collider contacts between two ticks (SPEC.md 2f): one streaming pass that pushes every particle a rank holds out
// of a list of spheres, capsules and boxes and gives it the contact's velocity response, in binary32 without FMA, in the order SPEC.md 2f
// parenthesises. Included by collide.hip alone. The record, the response and the 16-byte store are in contact_response.hip.hpp, which the
// heightfield pass (SPEC.md 2h) shares.
#pragma once
#include "contact_response.hip.hpp"

namespace sbk {

constexpr int kColliderBatch = 16;      // records per launch: 2 KiB of kernel arguments, read with scalar loads (uniform for the whole grid)
struct ColliderBatch {
    ColliderRec c[kColliderBatch];
};
constexpr uint32_t kColliderSphere = 0, kColliderCapsule = 1, kColliderBox = 2;      // SB_COLLIDER_*

// The sphere's rule about the point (cx, cy, cz): hit, outward normal, depth
__device__ __forceinline__ bool collide_round(float x, float y, float z, float cx, float cy, float cz, float radius, float (&n)[3], float &depth) {
    const float dx = x - cx, dy = y - cy, dz = z - cz;
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float xy = xx + yy;
    const float r2 = xy + zz;
    const float rr = radius * radius;
    if (!(r2 < rr)) return false;      // (a NaN or infinite position compares false)
    const float r = sqrtf(r2);
    const bool centre = r2 == 0.0f;
    const float qx = dx / r, qy = dy / r, qz = dz / r;
    n[0] = centre ? 0.0f : qx; n[1] = centre ? 1.0f : qy; n[2] = centre ? 0.0f : qz;
    depth = radius - r;
    return true;
}

// (hit, n, depth) of one point against one collider. The branch on C.shape is on a scalar: the record is uniform for the grid.
__device__ __forceinline__ bool collide_shape(const ColliderRec &C, float x, float y, float z, float (&n)[3], float &depth) {
    if (C.shape == kColliderSphere) return collide_round(x, y, z, C.a[0], C.a[1], C.a[2], C.radius, n, depth);
    if (C.shape == kColliderCapsule) {
        const float abx = C.b[0] - C.a[0], aby = C.b[1] - C.a[1], abz = C.b[2] - C.a[2];
        const float lx = abx * abx, ly = aby * aby, lz = abz * abz;
        const float lxy = lx + ly;
        const float L2 = lxy + lz;
        const float ex = x - C.a[0], ey = y - C.a[1], ez = z - C.a[2];
        const float sx = ex * abx, sy = ey * aby, sz = ez * abz;
        const float sxy = sx + sy;
        const float s = sxy + sz;
        float t = s / L2;
        t = (L2 == 0.0f || t != t) ? 0.0f : t;
        t = t < 0.0f ? 0.0f : t;
        t = t > 1.0f ? 1.0f : t;
        const float tx = t * abx, ty = t * aby, tz = t * abz;
        const float cx = C.a[0] + tx, cy = C.a[1] + ty, cz = C.a[2] + tz;
        return collide_round(x, y, z, cx, cy, cz, C.radius, n, depth);
    }
    const float ex = x - C.a[0], ey = y - C.a[1], ez = z - C.a[2];
    float q[3], dep[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float a = ex * C.rot[3 * k], b = ey * C.rot[3 * k + 1], c = ez * C.rot[3 * k + 2];
        const float ab = a + b;
        q[k] = ab + c;
        dep[k] = C.half[k] - __builtin_fabsf(q[k]);
    }
    if (!(__builtin_fabsf(q[0]) < C.half[0] && __builtin_fabsf(q[1]) < C.half[1] && __builtin_fabsf(q[2]) < C.half[2])) return false;
    // the exit face: the smallest depth, a tie keeps the lowest k
    const bool f1 = dep[1] < dep[0];
    float d = f1 ? dep[1] : dep[0], qf = f1 ? q[1] : q[0];
    float ax = f1 ? C.rot[3] : C.rot[0], ay = f1 ? C.rot[4] : C.rot[1], az = f1 ? C.rot[5] : C.rot[2];
    const bool f2 = dep[2] < d;
    d = f2 ? dep[2] : d; qf = f2 ? q[2] : qf;
    ax = f2 ? C.rot[6] : ax; ay = f2 ? C.rot[7] : ay; az = f2 ? C.rot[8] : az;
    const bool neg = qf < 0.0f;
    n[0] = neg ? -ax : ax; n[1] = neg ? -ay : ay; n[2] = neg ? -az : az;
    depth = d;
    return true;
}

constexpr int kCollideLanes = 256, kCollidePerLane = 4;      // 1 024 particles per workgroup

// place_kernel's access shape: a lane takes FOUR consecutive particles = three aligned 16-byte words of x and one of w; the last n mod 4
// particles take one lane each, word by word. What differs is what is NOT moved: velocities are read only by a lane that has a hit (at
// its first hit; they then stay in registers for the rest of the batch), and a lane stores only the 16-byte words of x and v that hold a
// component of a particle some collider wrote -- an untouched body costs 12 + 4 bytes per particle, and untouched particles keep every
// bit because nothing is written over them. The records of a batch are kernel arguments: scalar loads, one shape branch per collider on a
// scalar register. Particles are carried in registers across the colliders of the batch (the position after collider k is the input of
// collider k + 1). No LDS, no atomics: a lane writes only words it read.
__global__ __launch_bounds__(kCollideLanes) void collide_kernel(float *pos, float *vel, const float *wf, int64_t n, int count, ColliderBatch B) {
    const int64_t k = (int64_t)blockIdx.x * kCollideLanes + threadIdx.x;
    const int64_t n4 = n / kCollidePerLane;
    if (k < n4) {
        uint4 *px = reinterpret_cast<uint4 *>(pos) + 3 * k, *pv = reinterpret_cast<uint4 *>(vel) + 3 * k;
        const float4 W = reinterpret_cast<const float4 *>(wf)[k];
        const float w[4] = {W.x, W.y, W.z, W.w};
        if (!(W.x > 0.0f || W.y > 0.0f || W.z > 0.0f || W.w > 0.0f)) return;      // four pinned particles: nothing to read
        uint32_t x[12], v[12] = {};
        {
            const uint4 a = px[0], b = px[1], c = px[2];
            x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w; x[8] = c.x; x[9] = c.y; x[10] = c.z; x[11] = c.w;
        }
        bool have_v = false;
        unsigned wrote_x = 0, wrote_v = 0;      // bit j: particle j of the lane
        for (int ci = 0; ci < count; ++ci) {
            const ColliderRec &C = B.c[ci];
            float nrm[4][3], depth[4];
            bool hit[4];
#pragma unroll
            for (int j = 0; j < kCollidePerLane; ++j)
                hit[j] = w[j] > 0.0f && collide_shape(C, __uint_as_float(x[3 * j]), __uint_as_float(x[3 * j + 1]), __uint_as_float(x[3 * j + 2]), nrm[j], depth[j]);
            if (!(hit[0] || hit[1] || hit[2] || hit[3])) continue;
            if (!have_v) {
                const uint4 a = pv[0], b = pv[1], c = pv[2];
                v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w; v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
                have_v = true;
            }
#pragma unroll
            for (int j = 0; j < kCollidePerLane; ++j) {
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
        }
        // word 0 holds particles 0 and 1 (floats 0..3), word 1 particles 1 and 2, word 2 particles 2 and 3
        if (wrote_x & 0x3u) collide_store4(px, x[0], x[1], x[2], x[3]);
        if (wrote_x & 0x6u) collide_store4(px + 1, x[4], x[5], x[6], x[7]);
        if (wrote_x & 0xcu) collide_store4(px + 2, x[8], x[9], x[10], x[11]);
        // (wrote_v != 0 implies have_v: every word of v stored here was read)
        if (wrote_v & 0x3u) collide_store4(pv, v[0], v[1], v[2], v[3]);
        if (wrote_v & 0x6u) collide_store4(pv + 1, v[4], v[5], v[6], v[7]);
        if (wrote_v & 0xcu) collide_store4(pv + 2, v[8], v[9], v[10], v[11]);
        return;
    }
    const int64_t p = n4 * kCollidePerLane + (k - n4);
    if (p >= n) return;
    const float w = wf[p];
    if (!(w > 0.0f)) return;
    uint32_t *xs = reinterpret_cast<uint32_t *>(pos) + 3 * p, *vs = reinterpret_cast<uint32_t *>(vel) + 3 * p;
    uint32_t x[3] = {xs[0], xs[1], xs[2]}, v[3] = {};
    bool have_v = false, wrote_x = false, wrote_v = false;
    for (int ci = 0; ci < count; ++ci) {
        const ColliderRec &C = B.c[ci];
        float nrm[3], depth;
        if (!collide_shape(C, __uint_as_float(x[0]), __uint_as_float(x[1]), __uint_as_float(x[2]), nrm, depth)) continue;
        if (!have_v) { v[0] = vs[0]; v[1] = vs[1]; v[2] = vs[2]; have_v = true; }
        uint32_t vj[3] = {v[0], v[1], v[2]};
        wrote_x = true;
        if (collide_respond(C, nrm, depth, x, vj)) {
            wrote_v = true;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = vj[c];
        }
    }
    if (wrote_x) { xs[0] = x[0]; xs[1] = x[1]; xs[2] = x[2]; }
    if (wrote_v) { vs[0] = v[0]; vs[1] = v[1]; vs[2] = v[2]; }
}

// ---- reactions (SPEC.md 2g): what the body gives back to each collider -----------------------------------------------------------------

// One collider's slots, in 8-byte words, in the order of sb_collider_reaction (collide.hip asserts it): impulse xyz, angular impulse xyz
// about a, contact mass as doubles, then the number of contacts as int64
constexpr int kReactSlots = 8, kReactSums = 7;
constexpr int kReactRow = kColliderBatch * kReactSlots;       // a workgroup's row: 128 words = 1 KiB, valid only where its mask has the collider's bit
constexpr int kReactRowsPerGroup = 64;                         // rows one workgroup of the first final level adds up
constexpr int kReactFinalLanes = 1024, kReactFinalRuns = kReactFinalLanes / kReactRow;      // 8 runs of consecutive rows per final workgroup

__device__ __forceinline__ double collide_shfl_xor(double v, int mask) {
    return __hiloint2double(__shfl_xor(__double2hiint(v), mask, 64), __shfl_xor(__double2loint(v), mask, 64));
}

// One hit particle's terms (SPEC.md 2g), added to the lane's s[0..6]: binary64 on the binary32 values converted exactly; p = x' - a is the
// binary32 difference collide_respond itself takes. vb / va: the velocity's bits before / after the collider (equal where it was not written).
__device__ __forceinline__ void collide_react_terms(const ColliderRec &C, float w, const uint32_t (&x)[3], const uint32_t (&vb)[3], const uint32_t (&va)[3], double (&s)[kReactSums]) {
    const double m = 1.0 / (double)w;
    double j[3], p[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double dv = (double)__uint_as_float(vb[c]) - (double)__uint_as_float(va[c]);
        j[c] = m * dv;
        p[c] = (double)(__uint_as_float(x[c]) - C.a[c]);
        s[c] += j[c];
    }
    s[3] += p[1] * j[2] - p[2] * j[1];
    s[4] += p[2] * j[0] - p[0] * j[2];
    s[5] += p[0] * j[1] - p[1] * j[0];
    s[6] += m;
}

// collide_kernel's pass -- the same access shape, the same collide_shape / collide_respond statements on the same inputs, so the same bits in
// x and v -- which also reduces, per collider of the batch, the terms of the particles this rank OWNS (index < n_owned) that the collider
// hit. A lane keeps one collider's 7 sums and its count only while that collider is resolved: where any lane of the wave has such a hit
// (a ballot: the branch is wave-uniform) the wave adds them up in a butterfly and lane 0 leaves them in the wave's LDS row; a wave clear
// of the collider does nothing. The lanes of the tail take one particle each as particle 0 of a lane, so the whole wave walks ONE loop
// and no lane leaves before the barrier. Behind it the four waves' rows are added in wave order for the colliders some wave hit, and
// the workgroup writes that part of rows[blockIdx.x] and its mask of such colliders: a workgroup clear of every collider writes 4 bytes.
// No atomics; rows are overwritten by the next batch in stream order.
__global__ __launch_bounds__(kCollideLanes) void collide_react_kernel(float *pos, float *vel, const float *wf, int64_t n, int64_t n_owned, int count, ColliderBatch B,
                                                                     double *rows, uint32_t *masks) {
    __shared__ double wave_row[kCollideLanes / 64][kReactRow];
    __shared__ uint32_t wave_mask[kCollideLanes / 64];
    const int64_t k = (int64_t)blockIdx.x * kCollideLanes + threadIdx.x;
    const int64_t n4 = n / kCollidePerLane;
    const bool body = k < n4;
    const int64_t p0 = body ? k * kCollidePerLane : n4 * kCollidePerLane + (k - n4);      // the lane's first particle
    const bool tail = !body && p0 < n;
    uint4 *px = reinterpret_cast<uint4 *>(pos) + 3 * k, *pv = reinterpret_cast<uint4 *>(vel) + 3 * k;                      // body lanes
    uint32_t *xs = reinterpret_cast<uint32_t *>(pos) + 3 * p0, *vs = reinterpret_cast<uint32_t *>(vel) + 3 * p0;           // tail lanes
    float w[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t x[12] = {}, v[12] = {};
    if (body) {
        const float4 W = reinterpret_cast<const float4 *>(wf)[k];
        w[0] = W.x; w[1] = W.y; w[2] = W.z; w[3] = W.w;
    } else if (tail) w[0] = wf[p0];
    const bool live = w[0] > 0.0f || w[1] > 0.0f || w[2] > 0.0f || w[3] > 0.0f;      // (four pinned particles: nothing to read)
    if (live && body) {
        const uint4 a = px[0], b = px[1], c = px[2];
        x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w; x[8] = c.x; x[9] = c.y; x[10] = c.z; x[11] = c.w;
    } else if (live) { x[0] = xs[0]; x[1] = xs[1]; x[2] = xs[2]; }
    bool have_v = false;
    unsigned wrote_x = 0, wrote_v = 0;      // bit j: particle j of the lane
    uint32_t mask = 0;                      // bit ci: this wave left a row for collider ci (the same in every lane)
    for (int ci = 0; ci < count; ++ci) {
        const ColliderRec &C = B.c[ci];
        float nrm[4][3], depth[4];
        bool hit[4];
#pragma unroll
        for (int j = 0; j < kCollidePerLane; ++j)
            hit[j] = w[j] > 0.0f && collide_shape(C, __uint_as_float(x[3 * j]), __uint_as_float(x[3 * j + 1]), __uint_as_float(x[3 * j + 2]), nrm[j], depth[j]);
        double s[kReactSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        int32_t cnt = 0;
        if (hit[0] || hit[1] || hit[2] || hit[3]) {
            if (!have_v) {
                if (body) {
                    const uint4 a = pv[0], b = pv[1], c = pv[2];
                    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w; v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
                } else { v[0] = vs[0]; v[1] = vs[1]; v[2] = vs[2]; }
                have_v = true;
            }
#pragma unroll
            for (int j = 0; j < kCollidePerLane; ++j) {
                if (!hit[j]) continue;
                uint32_t xj[3] = {x[3 * j], x[3 * j + 1], x[3 * j + 2]}, vj[3] = {v[3 * j], v[3 * j + 1], v[3 * j + 2]};
                const uint32_t vb[3] = {vj[0], vj[1], vj[2]};
                const bool wv = collide_respond(C, nrm[j], depth[j], xj, vj);
                wrote_x |= 1u << j;
#pragma unroll
                for (int c = 0; c < 3; ++c) x[3 * j + c] = xj[c];
                if (wv) {
                    wrote_v |= 1u << j;
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[3 * j + c] = vj[c];
                }
                if (p0 + j < n_owned) {      // a ghost is its owner's to count
                    const uint32_t va[3] = {v[3 * j], v[3 * j + 1], v[3 * j + 2]};
                    collide_react_terms(C, w[j], xj, vb, va, s);
                    ++cnt;
                }
            }
        }
        if (__ballot(cnt != 0) != 0ull) {       // wave-uniform
#pragma unroll
            for (int q = 0; q < kReactSums; ++q)
                for (int msk = 32; msk >= 1; msk >>= 1) s[q] += collide_shfl_xor(s[q], msk);
            for (int msk = 32; msk >= 1; msk >>= 1) cnt += __shfl_xor(cnt, msk, 64);
            if ((threadIdx.x & 63) == 0) {
                double *row = &wave_row[threadIdx.x >> 6][kReactSlots * ci];
#pragma unroll
                for (int q = 0; q < kReactSums; ++q) row[q] = s[q];
                row[kReactSums] = __longlong_as_double((long long)cnt);
            }
            mask |= 1u << ci;
        }
    }
    if (body) {
        // word 0 holds particles 0 and 1 (floats 0..3), word 1 particles 1 and 2, word 2 particles 2 and 3
        if (wrote_x & 0x3u) collide_store4(px, x[0], x[1], x[2], x[3]);
        if (wrote_x & 0x6u) collide_store4(px + 1, x[4], x[5], x[6], x[7]);
        if (wrote_x & 0xcu) collide_store4(px + 2, x[8], x[9], x[10], x[11]);
        // (wrote_v != 0 implies have_v: every word of v stored here was read)
        if (wrote_v & 0x3u) collide_store4(pv, v[0], v[1], v[2], v[3]);
        if (wrote_v & 0x6u) collide_store4(pv + 1, v[4], v[5], v[6], v[7]);
        if (wrote_v & 0xcu) collide_store4(pv + 2, v[8], v[9], v[10], v[11]);
    } else {      // (a lane past the end has w = 0 and wrote nothing)
        if (wrote_x) { xs[0] = x[0]; xs[1] = x[1]; xs[2] = x[2]; }
        if (wrote_v) { vs[0] = v[0]; vs[1] = v[1]; vs[2] = v[2]; }
    }
    // the workgroup's row: waves 1 .. 3 onto wave 0 in that order, each only where it left something
    if ((threadIdx.x & 63) == 0) wave_mask[threadIdx.x >> 6] = mask;
    __syncthreads();
    uint32_t wm[kCollideLanes / 64], any = 0;
#pragma unroll
    for (int wv = 0; wv < kCollideLanes / 64; ++wv) { wm[wv] = wave_mask[wv]; any |= wm[wv]; }
    if (threadIdx.x == 0) masks[blockIdx.x] = any;
    if (threadIdx.x < kReactRow && ((any >> (threadIdx.x / kReactSlots)) & 1u)) {
        const int slot = threadIdx.x, ci = slot / kReactSlots;
        const bool integer = slot % kReactSlots == kReactSums;
        double t = 0.0;
        long long ti = 0;
#pragma unroll
        for (int wv = 0; wv < kCollideLanes / 64; ++wv) {
            if (!((wm[wv] >> ci) & 1u)) continue;
            const double r = wave_row[wv][slot];
            if (integer) ti += __double_as_longlong(r); else t += r;
        }
        rows[(size_t)kReactRow * blockIdx.x + slot] = integer ? __longlong_as_double(ti) : t;
    }
}

// Adds rows in a fixed order, the pattern of body_sums_final_kernel: workgroup g takes rows [g rows_per_group, (g + 1) rows_per_group) of
// n_rows, cut into 8 runs of consecutive rows; one lane per run and slot adds its run in row order, its rows fetched eight at a time
// (the additions keep their order, the loads do not wait for one another), then the 8 run sums are added in run order. A row counts
// only for the colliders in its mask. Two uses: the FIRST LEVEL (out_masks given) leaves one row and one mask per workgroup, written as
// the pass writes them; the LAST LEVEL (out_masks null, one workgroup) writes `count` colliders' slots to out_rows -- sb_collider_reaction
// records in mapped pinned memory --, zeros for a collider nothing hit. 0 rows: all zeros.
__global__ __launch_bounds__(kReactFinalLanes) void collide_react_final_kernel(const double *__restrict__ rows, const uint32_t *__restrict__ masks, int n_rows, int rows_per_group,
                                                                              double *__restrict__ out_rows, uint32_t *__restrict__ out_masks, int count) {
    constexpr int kBatch = 8;
    __shared__ double run_sum[kReactFinalRuns][kReactRow];
    __shared__ uint32_t run_mask[kReactFinalRuns];
    const int slot = threadIdx.x % kReactRow, run = threadIdx.x / kReactRow, ci = slot / kReactSlots;
    const bool integer = slot % kReactSlots == kReactSums;
    const int r0 = min(n_rows, (int)blockIdx.x * rows_per_group), r1 = min(n_rows, r0 + rows_per_group);
    const int per_run = (r1 - r0 + kReactFinalRuns - 1) / kReactFinalRuns;
    const int g0 = min(r1, r0 + run * per_run), g1 = min(r1, g0 + per_run);
    double t = 0.0;
    long long ti = 0;
    uint32_t seen = 0;
    for (int g = g0; g < g1; g += kBatch) {
        uint32_t mk[kBatch];
        double val[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) mk[j] = g + j < g1 ? masks[g + j] : 0u;
#pragma unroll
        for (int j = 0; j < kBatch; ++j) val[j] = (mk[j] >> ci) & 1u ? rows[(size_t)kReactRow * (g + j) + slot] : 0.0;
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            seen |= mk[j];
            if (!((mk[j] >> ci) & 1u)) continue;
            if (integer) ti += __double_as_longlong(val[j]); else t += val[j];
        }
    }
    run_sum[run][slot] = integer ? __longlong_as_double(ti) : t;
    if (slot == 0) run_mask[run] = seen;
    __syncthreads();
    if (threadIdx.x >= kReactRow) return;      // (behind the only barrier)
    uint32_t any = 0;
    double r = 0.0;
    long long ri = 0;
    for (int q = 0; q < kReactFinalRuns; ++q) {
        const uint32_t m = run_mask[q];
        any |= m;
        if (!((m >> ci) & 1u)) continue;
        if (integer) ri += __double_as_longlong(run_sum[q][slot]); else r += run_sum[q][slot];
    }
    const double word = integer ? __longlong_as_double(ri) : r;
    if (out_masks) {
        if (threadIdx.x == 0) out_masks[blockIdx.x] = any;
        if ((any >> ci) & 1u) out_rows[(size_t)kReactRow * blockIdx.x + slot] = word;
    } else if (ci < count) out_rows[slot] = word;
}

}  // namespace sbk
