// placement_kernels.hip.hpp — placement between two ticks (SPEC.md 2d): one streaming pass that rewrites positions and velocities of every
// particle a rank holds with one affine map, in binary32 without FMA, in the order SPEC.md 2d parenthesises. Included by placement.hip alone.
#pragma once
#include "device_math.hip.hpp"

namespace sbk {

// sb_placement without its two header words: the kernel's arguments (84 bytes, in scalar registers; the flags are template arguments)
struct PlaceMap {
    float m[9], from[3], to[3], lin[3], ang[3];
};

// SPEC.md 2d, the rule of 2c: a component that is WRITTEN and comes out NaN is stored as THE quiet NaN 0x7fc00000
__device__ __forceinline__ uint32_t place_canonical_bits(float v) { return v == v ? __float_as_uint(v) : 0x7fc00000u; }

// One particle. x, v: the stored words, in and out -- what SPEC.md 2d does not write passes through as bits (NaN payloads included);
// q: the words the map reads (x itself, or the reference pose). FROM_REFERENCE implies SET_VELOCITY (the host folds it in).
template <bool SET_VELOCITY, bool KEEP_PINNED>
__device__ __forceinline__ void place_particle(const PlaceMap &M, const uint32_t (&q)[3], float w, uint32_t (&x)[3], uint32_t (&v)[3]) {
    if (KEEP_PINNED && w == 0.0f) return;
    const float dx = __uint_as_float(q[0]) - M.from[0], dy = __uint_as_float(q[1]) - M.from[1], dz = __uint_as_float(q[2]) - M.from[2];
    float xn[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = M.m[3 * c] * dx, b = M.m[3 * c + 1] * dy, e = M.m[3 * c + 2] * dz;
        const float ab = a + b;
        const float abe = ab + e;
        xn[c] = abe + M.to[c];
        x[c] = place_canonical_bits(xn[c]);
    }
    if (!(w > 0.0f)) return;                // a pinned particle keeps its velocity's bits
    float vn[3];
    if (SET_VELOCITY) {
        // a = x' - to from the ROUNDED x' (a NaN x' gives a NaN a whatever its payload: xn serves)
        const float ax = xn[0] - M.to[0], ay = xn[1] - M.to[1], az = xn[2] - M.to[2];
        const float yz = M.ang[1] * az, zy = M.ang[2] * ay;
        const float zx = M.ang[2] * ax, xz = M.ang[0] * az;
        const float xy = M.ang[0] * ay, yx = M.ang[1] * ax;
        const float cx = yz - zy, cy = zx - xz, cz = xy - yx;
        vn[0] = M.lin[0] + cx; vn[1] = M.lin[1] + cy; vn[2] = M.lin[2] + cz;
    } else {
        const float vx = __uint_as_float(v[0]), vy = __uint_as_float(v[1]), vz = __uint_as_float(v[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float a = M.m[3 * c] * vx, b = M.m[3 * c + 1] * vy;
            const float ab = a + b;
            const float e = M.m[3 * c + 2] * vz;
            vn[c] = ab + e;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = place_canonical_bits(vn[c]);
}

// One aligned 16-byte store. Written out: left to itself the compiler re-splits a lane's 48 bytes into four 12-byte stores (one per particle,
// straight from the registers the arithmetic left them in), three of which straddle a 16-byte boundary. The statement ends with the two
// wait states a store of more than 8 bytes needs before a VALU instruction may overwrite its data registers: the compiler pads its own
// stores but not an asm statement, and frees the operands for reuse right behind it (here: for the next store's address).
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void place_store4(uint4 *p, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    const u32x4_t v = {a, b, c, d};
    asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}

constexpr int kPlaceLanes = 256, kPlacePerLane = 4;      // 1 024 particles per workgroup

// The packed xyz arrays are read and written 16 bytes at a time: a lane takes FOUR consecutive particles = 48 bytes = three aligned
// 16-byte words of each array (the arrays come from hipMalloc; 48 k is a multiple of 16), and the four inverse masses as one more. Every
// byte of every line is used; a lane's three accesses fall in at most two 128-byte lines. The last n mod 4 particles take one lane each,
// word by word (lanes n / 4 .. n / 4 + n mod 4 - 1). No LDS, no atomics: a lane writes only what it read.
// Reads that the mode does not need are not made: the reference pose replaces the positions' read unless a pinned particle keeps its
// own (KEEP_PINNED), SET_VELOCITY needs the old velocities only for a lane that holds a pinned particle.
template <bool FROM_REFERENCE, bool SET_VELOCITY, bool KEEP_PINNED>
__global__ __launch_bounds__(kPlaceLanes) void place_kernel(float *pos, float *vel, const float *ref, const float *wf, int64_t n, PlaceMap M) {
    const int64_t k = (int64_t)blockIdx.x * kPlaceLanes + threadIdx.x;
    const int64_t n4 = n / kPlacePerLane;
    if (k < n4) {
        uint4 *px = reinterpret_cast<uint4 *>(pos) + 3 * k, *pv = reinterpret_cast<uint4 *>(vel) + 3 * k;
        const float4 W = reinterpret_cast<const float4 *>(wf)[k];
        const float w[4] = {W.x, W.y, W.z, W.w};
        const bool pinned = W.x == 0.0f || W.y == 0.0f || W.z == 0.0f || W.w == 0.0f;
        const bool all_free = W.x > 0.0f && W.y > 0.0f && W.z > 0.0f && W.w > 0.0f;
        uint32_t x[12] = {}, v[12] = {}, q[12];
        const bool read_x = !FROM_REFERENCE || (KEEP_PINNED && pinned);
        const bool read_v = !SET_VELOCITY || !all_free;
        if (read_x) {
            const uint4 a = px[0], b = px[1], c = px[2];
            x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w; x[8] = c.x; x[9] = c.y; x[10] = c.z; x[11] = c.w;
        }
        if (read_v) {
            const uint4 a = pv[0], b = pv[1], c = pv[2];
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w; v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
        }
        if (FROM_REFERENCE) {
            const uint4 *pq = reinterpret_cast<const uint4 *>(ref) + 3 * k;
            const uint4 a = pq[0], b = pq[1], c = pq[2];
            q[0] = a.x; q[1] = a.y; q[2] = a.z; q[3] = a.w; q[4] = b.x; q[5] = b.y; q[6] = b.z; q[7] = b.w; q[8] = c.x; q[9] = c.y; q[10] = c.z; q[11] = c.w;
        } else {
#pragma unroll
            for (int i = 0; i < 12; ++i) q[i] = x[i];
        }
#pragma unroll
        for (int j = 0; j < kPlacePerLane; ++j) {
            const uint32_t qj[3] = {q[3 * j], q[3 * j + 1], q[3 * j + 2]};
            uint32_t xj[3] = {x[3 * j], x[3 * j + 1], x[3 * j + 2]}, vj[3] = {v[3 * j], v[3 * j + 1], v[3 * j + 2]};
            place_particle<SET_VELOCITY, KEEP_PINNED>(M, qj, w[j], xj, vj);
#pragma unroll
            for (int c = 0; c < 3; ++c) { x[3 * j + c] = xj[c]; v[3 * j + c] = vj[c]; }
        }
        // (every word of x is defined here: either read, or written by place_particle -- without KEEP_PINNED every particle's position is
        // written, with it a lane that holds a pinned particle has read; the same for v with `all_free`)
        place_store4(px, x[0], x[1], x[2], x[3]); place_store4(px + 1, x[4], x[5], x[6], x[7]); place_store4(px + 2, x[8], x[9], x[10], x[11]);
        place_store4(pv, v[0], v[1], v[2], v[3]); place_store4(pv + 1, v[4], v[5], v[6], v[7]); place_store4(pv + 2, v[8], v[9], v[10], v[11]);
        return;
    }
    const int64_t p = n4 * kPlacePerLane + (k - n4);
    if (p >= n) return;
    uint32_t *xs = reinterpret_cast<uint32_t *>(pos) + 3 * p, *vs = reinterpret_cast<uint32_t *>(vel) + 3 * p;
    const float w = wf[p];
    uint32_t x[3] = {xs[0], xs[1], xs[2]}, v[3] = {vs[0], vs[1], vs[2]}, q[3];
    const uint32_t *qs = FROM_REFERENCE ? reinterpret_cast<const uint32_t *>(ref) + 3 * p : xs;
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = FROM_REFERENCE ? qs[c] : x[c];
    place_particle<SET_VELOCITY, KEEP_PINNED>(M, q, w, x, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) { xs[c] = x[c]; vs[c] = v[c]; }
}

}  // namespace sbk
