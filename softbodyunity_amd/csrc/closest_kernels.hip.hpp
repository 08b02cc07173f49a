// closest_kernels.hip.hpp — SPEC.md §6g: closest points on a snapshot's triangles, in two launches and without atomics, after the ray cast
// of readback_kernels.hip.hpp (included first: RayBest, ray_take, ray_pack / ray_unpack, ray_reduce_wave, kRayLanes, kRayMaxGroups and
// kRayMiss are its). A candidate's squared distance dd is a sum of squares -- +0 or positive, never -0 -- so its bits order as an unsigned
// integer and the 64-bit key (bits(dd) << 32) | triangle, a miss all ones, is a total order: its minimum is exact, the triangle ids are
// distinct, so any tree delivers the sequential loop's hit, (u, v) travelling with the key. The square root is taken once, at the end.
//
// No reference counterpart exists (/root/reference/README.md:1 is the whole reference tree).
#pragma once

namespace sbk {

constexpr int kClosestTile = 4;         // queries a workgroup tests every triangle against (see closest_partial_kernel)
constexpr int kClosestBatch = 256;      // queries per pair of launches: the ray cast's buffers hold them (kRayBatch rays of 8 floats, kRayBatch hits)
static_assert(kClosestBatch <= kRayBatch, "a batch of queries lives in the buffers of a batch of rays");

// SPEC.md §6g for one triangle (corners pa, pb, pc, edges ab = pb - pa and ac = pc - pa) and one query q: the Voronoi-region chain, the
// first test that holds deciding (u, v). Every region needs at most one quotient, so the chain selects numerator and denominator and
// divides once: only the selected values are observable, and they are the chain's own operations on the chain's own operands. A NaN
// fails every predicate, falls through to the face and comes out as a NaN dd, which is no candidate. -> dd
__device__ __forceinline__ float closest_on_triangle(V3 pa, V3 pb, V3 pc, V3 ab, V3 ac, V3 q, float &u, float &v) {
    const V3 ap = sub3(q, pa), bp = sub3(q, pb), cp = sub3(q, pc);
    const float d1 = dot3(ab, ap), d2 = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    const float vc = (d1 * d4) - (d3 * d2), vb = (d5 * d2) - (d1 * d6), va = (d3 * d6) - (d5 * d4), e = d4 - d3, f = d5 - d6;
    // region 1 .. 7 of the chain; num / den is its one quotient (1 / 1 where it has none)
    int region;
    float num = 1.0f, den = 1.0f;
    if (d1 <= 0.0f && d2 <= 0.0f) region = 1;
    else if (d3 >= 0.0f && d4 <= d3) region = 2;
    else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { region = 3; num = d1; den = d1 - d3; }
    else if (d6 >= 0.0f && d5 <= d6) region = 4;
    else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { region = 5; num = d2; den = d2 - d6; }
    else if (va <= 0.0f && e >= 0.0f && f >= 0.0f) { region = 6; num = e; den = e + f; }
    else { region = 7; den = (va + vb) + vc; }
    const float w = num / den;
    u = region == 2 ? 1.0f : region == 3 ? w : region == 6 ? 1.0f - w : region == 7 ? vb * w : 0.0f;
    v = region == 4 ? 1.0f : region == 5 || region == 6 ? w : region == 7 ? vc * w : 0.0f;
    const V3 c = {pa.x + ((u * ab.x) + (v * ac.x)), pa.y + ((u * ab.y) + (v * ac.y)), pa.z + ((u * ab.z) + (v * ac.z))};
    const V3 r = sub3(q, c);
    return dot3(r, r);
}

// Grid (triangle chunks, query tiles), the launch shape of raycast_partial_kernel. Lane k of a chunk row walks triangles k, k + stride, ...:
// three indices and three 12-byte rows per triangle, gathered once, ab and ac formed once, and tested against the kClosestTile queries of
// blockIdx.y. A query's address is the same in every lane (kernel argument and blockIdx only), so its four floats arrive by scalar loads
// and stay in SGPRs, R2 = max_distance * max_distance with them. Per query one key and (u, v) in registers; at the end a wave64 butterfly,
// the four waves through LDS, and lanes 0 .. kClosestTile-1 store the workgroup's partial of one query each, 16 bytes:
// partials[query * gridDim.x + chunk]. The statements are SPEC.md §6g's, in its order (the unit is built with contraction off).
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): 70 VGPRs and 65 SGPRs at kClosestTile = 4, no spills, 7 waves per SIMD
// (fifteen of them hold pa, pb, pc, ab, ac; sixteen the four keys with their (u, v)); a tile of 8 takes 86 VGPRs and leaves 5 waves, so
// the tile stays the ray cast's.
// n_queries >= 1; gridDim.y = ceil(n_queries / kClosestTile); gridDim.x = min(ceil(m / 256), kRayMaxGroups) >= 1.
__global__ __launch_bounds__(kRayLanes) void closest_partial_kernel(const float *xyz, const int32_t *tri, int m, const float *queries, int n_queries, uint4 *partials) {
    __shared__ uint4 wave_best[kRayLanes / 64][kClosestTile];
    const int q0 = (int)blockIdx.y * kClosestTile;
    RayBest best[kClosestTile];
#pragma unroll
    for (int j = 0; j < kClosestTile; ++j) best[j] = {kRayMiss, 0.0f, 0.0f};
    const int stride = (int)gridDim.x * kRayLanes;
    for (int64_t t_id = (int64_t)blockIdx.x * kRayLanes + threadIdx.x; t_id < m; t_id += stride) {
        const size_t a = 3 * (size_t)tri[3 * t_id], b = 3 * (size_t)tri[3 * t_id + 1], c = 3 * (size_t)tri[3 * t_id + 2];
        const V3 pa = {xyz[a], xyz[a + 1], xyz[a + 2]}, pb = {xyz[b], xyz[b + 1], xyz[b + 2]}, pc = {xyz[c], xyz[c + 1], xyz[c + 2]};
        const V3 ab = sub3(pb, pa), ac = sub3(pc, pa);
#pragma unroll
        for (int j = 0; j < kClosestTile; ++j) {
            if (q0 + j >= n_queries) break;       // (the same in every lane)
            const float *qr = queries + 4 * (size_t)(q0 + j);
            const float R2 = qr[3] * qr[3];
            float u, v;
            const float dd = closest_on_triangle(pa, pb, pc, ab, ac, {qr[0], qr[1], qr[2]}, u, v);
            if (!(dd <= R2 && dd < __builtin_inff())) continue;
            ray_take(best[j], ((unsigned long long)__float_as_uint(dd) << 32) | (unsigned)t_id, u, v);
        }
    }
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < kClosestTile; ++j) {
        ray_reduce_wave(best[j]);
        if ((threadIdx.x & 63) == 0) wave_best[wave][j] = ray_pack(best[j]);
    }
    __syncthreads();
    const int j = threadIdx.x;
    if (j < kClosestTile && q0 + j < n_queries) {
        RayBest b = ray_unpack(wave_best[0][j]);
        for (int w = 1; w < kRayLanes / 64; ++w) { const RayBest o = ray_unpack(wave_best[w][j]); ray_take(b, o.key, o.u, o.v); }
        partials[(size_t)(q0 + j) * gridDim.x + blockIdx.x] = ray_pack(b);
    }
}

// Workgroup r reduces query r's n_partials partials by key and writes its sb_closest_hit -- triangle, sqrtf(dd), u, v; a miss: -1, 0, 0,
// 0 -- in one 16-byte store.
__global__ __launch_bounds__(kRayLanes) void closest_final_kernel(const uint4 *partials, int n_partials, uint4 *hits) {
    __shared__ uint4 wave_best[kRayLanes / 64];
    RayBest b = {kRayMiss, 0.0f, 0.0f};
    const uint4 *mine = partials + (size_t)blockIdx.x * n_partials;
    for (int g = threadIdx.x; g < n_partials; g += kRayLanes) { const RayBest o = ray_unpack(mine[g]); ray_take(b, o.key, o.u, o.v); }
    ray_reduce_wave(b);
    if ((threadIdx.x & 63) == 0) wave_best[threadIdx.x >> 6] = ray_pack(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kRayLanes / 64; ++w) { const RayBest o = ray_unpack(wave_best[w]); ray_take(b, o.key, o.u, o.v); }
        const float distance = sqrtf(__uint_as_float((unsigned)(b.key >> 32)));
        hits[blockIdx.x] = b.key == kRayMiss ? make_uint4(0xffffffffu, 0u, 0u, 0u) : make_uint4((unsigned)b.key, __float_as_uint(distance), __float_as_uint(b.u), __float_as_uint(b.v));
    }
}

}  // namespace sbk
