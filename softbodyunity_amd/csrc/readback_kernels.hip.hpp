// readback_kernels.hip.hpp — render readback: snapshots in caller numbering, embedded render vertices (SPEC.md §6b) and area-weighted
// vertex normals (SPEC.md §6a), vertex tangents from UVs (SPEC.md §6c)
//
// No reference counterpart exists (/root/reference/README.md:1 is the whole reference tree).
#pragma once
#include "device_math.hip.hpp"

namespace sbk {

// Render readback: owned positions (device order, float4) -> caller order, packed xyz.
__global__ __launch_bounds__(256) void snapshot_kernel(PosView pos, const int32_t *local_to_old, float *out_xyz, int n_owned) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= n_owned) return;
    const float4 p = pv_load(pos, l);
    const size_t o = 3 * (size_t)local_to_old[l];
    out_xyz[o] = p.x; out_xyz[o + 1] = p.y; out_xyz[o + 2] = p.z;
}

// Snapshot of the render set only: entry subset[k] of the caller-numbered snapshot <- particle local_of_subset[k].
__global__ __launch_bounds__(256) void snapshot_subset_kernel(PosView pos, const int32_t *subset, const int32_t *local_of_subset,
                                                             float *out_xyz, int count) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= count) return;
    const float4 p = pv_load(pos, local_of_subset[k]);
    const size_t o = 3 * (size_t)subset[k];
    out_xyz[o] = p.x; out_xyz[o + 1] = p.y; out_xyz[o + 2] = p.z;
}

// The render set of a rank of a partitioned solver (no normals there): compact entry k <- particle local_of_subset[k].
__global__ __launch_bounds__(256) void snapshot_compact_kernel(PosView pos, const int32_t *local_of_subset, float *out_xyz, int count) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= count) return;
    const float4 p = pv_load(pos, local_of_subset[k]);
    const size_t o = 3 * (size_t)k;
    out_xyz[o] = p.x; out_xyz[o + 1] = p.y; out_xyz[o + 2] = p.z;
}

// SPEC.md §6b: embedded render vertices. One lane per render vertex r: r = ((w0 x[i0] + w1 x[i1]) + w2 x[i2]) + w3 x[i3], every product
// rounded, the sums left to right (the unit is built with contraction off). src_xyz is any packed xyz array the cage indexes: the state
// or the peek array in device numbering (the solver translates the cage once), or a gathered snapshot in whole-mesh numbering (the
// group). A bandwidth-bound gather: 16 B of cage and 16 B of weights per lane, coalesced; four 12-byte reads wherever the cage points
// (neighbouring render vertices share cages, so most of them are served by the L2); 12 B out, in the caller's vertex order.
__global__ __launch_bounds__(256) void skin_kernel(const float *src_xyz, const int4 *cage, const float4 *weights, float *out_xyz, int m) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= m) return;
    const int4 c = cage[r];
    const float4 w = weights[r];
    const size_t a0 = 3 * (size_t)c.x, a1 = 3 * (size_t)c.y, a2 = 3 * (size_t)c.z, a3 = 3 * (size_t)c.w;
    const V3 x0 = {src_xyz[a0], src_xyz[a0 + 1], src_xyz[a0 + 2]};
    const V3 x1 = {src_xyz[a1], src_xyz[a1 + 1], src_xyz[a1 + 2]};
    const V3 x2 = {src_xyz[a2], src_xyz[a2 + 1], src_xyz[a2 + 2]};
    const V3 x3 = {src_xyz[a3], src_xyz[a3 + 1], src_xyz[a3 + 2]};
    const size_t o = 3 * (size_t)r;
    out_xyz[o] = ((w.x * x0.x + w.y * x1.x) + w.z * x2.x) + w.w * x3.x;
    out_xyz[o + 1] = ((w.x * x0.y + w.y * x1.y) + w.z * x2.y) + w.w * x3.y;
    out_xyz[o + 2] = ((w.x * x0.z + w.y * x1.z) + w.z * x2.z) + w.w * x3.z;
}

// SPEC.md §6a: area-weighted vertex normals on a position snapshot in caller numbering. One lane per vertex gathers its
// incident triangles in ascending order (adj lists built on the host), so the additions happen in the oracle's order.
__global__ __launch_bounds__(256) void normals_kernel(const float *snap_xyz, const int32_t *adj_off, const int32_t *adj_tri,
                                                      const int32_t *tri, float *nrm_xyz, int n, const int32_t *subset,
                                                      float *subset_pos_xyz) {
    // subset == nullptr: lane k handles particle k and writes normal k. Otherwise lane k handles particle subset[k] and
    // writes compact entry k of the normals AND of the positions (the render set travels to the host on its own).
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int v = subset ? subset[k] : k;
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    for (int q = adj_off[v]; q < adj_off[v + 1]; ++q) {
        const int t = adj_tri[q];
        const size_t a = 3 * (size_t)tri[3 * t], b = 3 * (size_t)tri[3 * t + 1], c = 3 * (size_t)tri[3 * t + 2];
        const V3 xa = {snap_xyz[a], snap_xyz[a + 1], snap_xyz[a + 2]};
        const V3 e1 = sub3({snap_xyz[b], snap_xyz[b + 1], snap_xyz[b + 2]}, xa);
        const V3 e2 = sub3({snap_xyz[c], snap_xyz[c + 1], snap_xyz[c + 2]}, xa);
        const V3 f = cross3(e1, e2);
        nx = nx + f.x; ny = ny + f.y; nz = nz + f.z;
    }
    float xx = nx * nx, yy = ny * ny, zz = nz * nz;
    float L2 = (xx + yy) + zz;
    if (L2 >= 0x1p-96f) { float L = sqrt_rn_normal(L2); nx = nx / L; ny = ny / L; nz = nz / L; }
    else { nx = 0.0f; ny = 0.0f; nz = 0.0f; }
    const size_t o = 3 * (size_t)k;
    nrm_xyz[o] = nx; nrm_xyz[o + 1] = ny; nrm_xyz[o + 2] = nz;
    if (subset) {
        const size_t sv = 3 * (size_t)v;
        subset_pos_xyz[o] = snap_xyz[sv]; subset_pos_xyz[o + 1] = snap_xyz[sv + 1]; subset_pos_xyz[o + 2] = snap_xyz[sv + 2];
    }
}

// SPEC.md §6c: the normals of §6a and per-vertex tangents from UVs in one walk. Same lanes, same subset / compact convention and, for the
// normal, the same statements as normals_kernel -- a readback delivers the same normal bits with and without UVs. The three corners of an
// incident triangle are gathered once and feed the face normal and both tangent-frame sums (tri_k: the triangle's four UV coefficients,
// one 16-byte load). A latency-bound gather: within an iteration the index, coefficient and corner loads do not depend on one another,
// and the next triangle's id is fetched one iteration ahead of its use. The 12 accumulators and 9 corner coordinates leave the lane far
// below the 64 registers full occupancy allows. No contraction (the unit is built with it off); tangent out as one 16-byte store.
__global__ __launch_bounds__(256) void normals_tangents_kernel(const float *snap_xyz, const int32_t *adj_off, const int32_t *adj_tri,
                                                               const int32_t *tri, const float4 *tri_k, float *nrm_xyz, float4 *tan_xyzw,
                                                               int n, const int32_t *subset, float *subset_pos_xyz) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int v = subset ? subset[k] : k;
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    V3 S = {0.0f, 0.0f, 0.0f}, T = {0.0f, 0.0f, 0.0f};
    int q = adj_off[v];
    const int q_end = adj_off[v + 1];
    int t = q < q_end ? adj_tri[q] : 0;
    for (; q < q_end; ++q) {
        const int t_next = q + 1 < q_end ? adj_tri[q + 1] : t;
        const size_t a = 3 * (size_t)tri[3 * t], b = 3 * (size_t)tri[3 * t + 1], c = 3 * (size_t)tri[3 * t + 2];
        const float4 kk = tri_k[t];
        const V3 xa = {snap_xyz[a], snap_xyz[a + 1], snap_xyz[a + 2]};
        const V3 e1 = sub3({snap_xyz[b], snap_xyz[b + 1], snap_xyz[b + 2]}, xa);
        const V3 e2 = sub3({snap_xyz[c], snap_xyz[c + 1], snap_xyz[c + 2]}, xa);
        const V3 f = cross3(e1, e2);
        nx = nx + f.x; ny = ny + f.y; nz = nz + f.z;
        const V3 s = {kk.x * e1.x - kk.y * e2.x, kk.x * e1.y - kk.y * e2.y, kk.x * e1.z - kk.y * e2.z};
        const V3 g = {kk.z * e2.x - kk.w * e1.x, kk.z * e2.y - kk.w * e1.y, kk.z * e2.z - kk.w * e1.z};
        S.x = S.x + s.x; S.y = S.y + s.y; S.z = S.z + s.z;
        T.x = T.x + g.x; T.y = T.y + g.y; T.z = T.z + g.z;
        t = t_next;
    }
    float xx = nx * nx, yy = ny * ny, zz = nz * nz;
    float L2 = (xx + yy) + zz;
    if (L2 >= 0x1p-96f) { float L = sqrt_rn_normal(L2); nx = nx / L; ny = ny / L; nz = nz / L; }
    else { nx = 0.0f; ny = 0.0f; nz = 0.0f; }
    const size_t o = 3 * (size_t)k;
    nrm_xyz[o] = nx; nrm_xyz[o + 1] = ny; nrm_xyz[o + 2] = nz;
    if (subset) {
        const size_t sv = 3 * (size_t)v;
        subset_pos_xyz[o] = snap_xyz[sv]; subset_pos_xyz[o + 1] = snap_xyz[sv + 1]; subset_pos_xyz[o + 2] = snap_xyz[sv + 2];
    }
    // Gram-Schmidt against the normal, handedness from the accumulated bitangent
    const V3 nn = {nx, ny, nz};
    const float d = dot3(nn, S);
    const float dx = d * nn.x, dy = d * nn.y, dz = d * nn.z;
    V3 u = {S.x - dx, S.y - dy, S.z - dz};
    const float U2 = dot3(u, u);
    if (U2 >= 0x1p-96f) { float U = sqrt_rn_normal(U2); u.x = u.x / U; u.y = u.y / U; u.z = u.z / U; }
    else { u.x = 0.0f; u.y = 0.0f; u.z = 0.0f; }
    const float h = dot3(cross3(nn, S), T);
    tan_xyzw[k] = make_float4(u.x, u.y, u.z, h < 0.0f ? -1.0f : 1.0f);
}

// SPEC.md §6d: the axis-aligned box of a set of rows, in two launches and without atomics. Minimum and maximum are exact, and after the final
// + 0.0f the box depends on the multiset of values only, so any tree gives the spec's bits. A NaN never wins a comparison: the accumulators
// start at +inf / -inf and only ever take a value that compared less / greater, so no accumulator holds a NaN and the tree needs no NaN rule.
constexpr int kBoundsLanes = 256;
constexpr int kBoundsMaxGroups = 2048;      // grid cap of bounds_partial_kernel: 8 waves per SIMD on 256 CUs; larger sets walk the grid-stride loop

struct Box6 { float lo[3], hi[3]; };

__device__ __forceinline__ void box_take(Box6 &b, float x, float y, float z) {
    if (x < b.lo[0]) b.lo[0] = x;
    if (y < b.lo[1]) b.lo[1] = y;
    if (z < b.lo[2]) b.lo[2] = z;
    if (x > b.hi[0]) b.hi[0] = x;
    if (y > b.hi[1]) b.hi[1] = y;
    if (z > b.hi[2]) b.hi[2] = z;
}
// lo against lo, hi against hi: an empty component (+inf, -inf) must not leak its +inf into hi
__device__ __forceinline__ void box_merge(Box6 &b, const float *lo_hi6) {
    for (int c = 0; c < 3; ++c) {
        if (lo_hi6[c] < b.lo[c]) b.lo[c] = lo_hi6[c];
        if (lo_hi6[3 + c] > b.hi[c]) b.hi[c] = lo_hi6[3 + c];
    }
}

// The workgroup's box in lane 0: a wave64 butterfly, then the four waves' boxes through LDS. Every lane of the 256 calls it.
__device__ __forceinline__ void box_reduce_workgroup(Box6 &b) {
    __shared__ float wave_box[kBoundsLanes / 64][6];
    for (int m = 32; m >= 1; m >>= 1)
        for (int c = 0; c < 3; ++c) {
            const float l = __shfl_xor(b.lo[c], m, 64), h = __shfl_xor(b.hi[c], m, 64);
            if (l < b.lo[c]) b.lo[c] = l;
            if (h > b.hi[c]) b.hi[c] = h;
        }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int c = 0; c < 3; ++c) { wave_box[wave][c] = b.lo[c]; wave_box[wave][3 + c] = b.hi[c]; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kBoundsLanes / 64; ++w) box_merge(b, wave_box[w]);
}

// Lane k of the grid reduces rows k, k + grid, ... of a packed xyz array: row rows[k] where a row list is given (a rank's full snapshot:
// the caller ids of the particles it owns), else row k -- neighbouring lanes then read neighbouring 12-byte rows, one 768-byte run per wave.
// Workgroup g writes partials[6g .. 6g+5] = lo.xyz, hi.xyz. The launch has min(ceil(count / 256), kBoundsMaxGroups) workgroups.
__global__ __launch_bounds__(kBoundsLanes) void bounds_partial_kernel(const float *xyz, const int32_t *rows, int count, float *partials) {
    const float inf = __builtin_inff();
    Box6 b = {{inf, inf, inf}, {-inf, -inf, -inf}};
    const int stride = (int)gridDim.x * kBoundsLanes;
    for (int64_t k = (int64_t)blockIdx.x * kBoundsLanes + threadIdx.x; k < count; k += stride) {
        const size_t o = 3 * (size_t)(rows ? rows[k] : (int32_t)k);
        box_take(b, xyz[o], xyz[o + 1], xyz[o + 2]);
    }
    box_reduce_workgroup(b);
    if (threadIdx.x == 0) {
        float *out = partials + 6 * (size_t)blockIdx.x;
        out[0] = b.lo[0]; out[1] = b.lo[1]; out[2] = b.lo[2]; out[3] = b.hi[0]; out[4] = b.hi[1]; out[5] = b.hi[2];
    }
}

// One workgroup reduces the n_partials rows of six floats (0 rows: the empty box), applies the + 0.0f that makes a zero result +0, and
// writes box8 = lo.xyz, 0, hi.xyz, 0.
__global__ __launch_bounds__(kBoundsLanes) void bounds_final_kernel(const float *partials, int n_partials, float *box8) {
    const float inf = __builtin_inff();
    Box6 b = {{inf, inf, inf}, {-inf, -inf, -inf}};
    for (int g = threadIdx.x; g < n_partials; g += kBoundsLanes) box_merge(b, partials + 6 * (size_t)g);
    box_reduce_workgroup(b);
    if (threadIdx.x == 0) {
        box8[0] = b.lo[0] + 0.0f; box8[1] = b.lo[1] + 0.0f; box8[2] = b.lo[2] + 0.0f; box8[3] = 0.0f;
        box8[4] = b.hi[0] + 0.0f; box8[5] = b.hi[1] + 0.0f; box8[6] = b.hi[2] + 0.0f; box8[7] = 0.0f;
    }
}

// SPEC.md §6e: ray casts against a snapshot's triangles, in two launches and without atomics. A candidate's distance is a non-negative float
// after its + 0.0f, so its bits order as an unsigned integer and the 64-bit key (bits(t) << 32) | triangle, a miss all ones, is a total
// order: its minimum is exact, the triangle ids are distinct, so any tree delivers the sequential loop's hit, (u, v) travelling with the key.
constexpr int kRayLanes = 256;
constexpr int kRayMaxGroups = 1024;     // grid cap of raycast_partial_kernel along the triangles; larger lists walk the grid-stride loop
constexpr int kRayTile = 4;             // rays a workgroup tests every triangle against: 4 x (key, u, v) = 16 registers beside the corners
constexpr int kRayBatch = 256;          // rays per pair of launches: the partials are kRayMaxGroups x kRayBatch x 16 bytes, whatever the count
constexpr unsigned long long kRayMiss = ~0ull;

struct RayBest { unsigned long long key; float u, v; };

__device__ __forceinline__ void ray_take(RayBest &b, unsigned long long key, float u, float v) {
    if (key < b.key) { b.key = key; b.u = u; b.v = v; }
}
__device__ __forceinline__ uint4 ray_pack(const RayBest &b) {
    return make_uint4((unsigned)b.key, (unsigned)(b.key >> 32), __float_as_uint(b.u), __float_as_uint(b.v));
}
__device__ __forceinline__ RayBest ray_unpack(uint4 q) {
    return {((unsigned long long)q.y << 32) | q.x, __uint_as_float(q.z), __uint_as_float(q.w)};
}
// the wave's minimum in every lane of it
__device__ __forceinline__ void ray_reduce_wave(RayBest &b) {
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)b.key, m, 64), hi = __shfl_xor((unsigned)(b.key >> 32), m, 64);
        const float u = __shfl_xor(b.u, m, 64), v = __shfl_xor(b.v, m, 64);
        ray_take(b, ((unsigned long long)hi << 32) | lo, u, v);
    }
}

// Grid (triangle chunks, ray tiles). Lane k of a chunk row walks triangles k, k + stride, ...: three indices and three 12-byte rows per
// triangle, gathered once and tested against the kRayTile rays of blockIdx.y. A ray's address is the same in every lane (kernel argument
// and blockIdx only), so its eight floats arrive by scalar loads and stay in SGPRs. Per ray one key and (u, v) in registers; at the end a
// wave64 butterfly, the four waves through LDS, and lanes 0 .. kRayTile-1 store the workgroup's partial of one ray each, 16 bytes:
// partials[ray * gridDim.x + chunk]. The statements are SPEC.md §6e's, in its order (the unit is built with contraction off).
// n_rays >= 1; gridDim.y = ceil(n_rays / kRayTile); gridDim.x = min(ceil(m / 256), kRayMaxGroups) >= 1.
__global__ __launch_bounds__(kRayLanes) void raycast_partial_kernel(const float *xyz, const int32_t *tri, int m, const float *rays, int n_rays, uint4 *partials) {
    __shared__ uint4 wave_best[kRayLanes / 64][kRayTile];
    const int ray0 = (int)blockIdx.y * kRayTile;
    RayBest best[kRayTile];
#pragma unroll
    for (int j = 0; j < kRayTile; ++j) best[j] = {kRayMiss, 0.0f, 0.0f};
    const int stride = (int)gridDim.x * kRayLanes;
    for (int64_t t_id = (int64_t)blockIdx.x * kRayLanes + threadIdx.x; t_id < m; t_id += stride) {
        const size_t a = 3 * (size_t)tri[3 * t_id], b = 3 * (size_t)tri[3 * t_id + 1], c = 3 * (size_t)tri[3 * t_id + 2];
        const V3 pa = {xyz[a], xyz[a + 1], xyz[a + 2]};
        const V3 e1 = sub3({xyz[b], xyz[b + 1], xyz[b + 2]}, pa);
        const V3 e2 = sub3({xyz[c], xyz[c + 1], xyz[c + 2]}, pa);
#pragma unroll
        for (int j = 0; j < kRayTile; ++j) {
            if (ray0 + j >= n_rays) break;       // (the same in every lane)
            const float *r = rays + 8 * (size_t)(ray0 + j);
            const V3 o = {r[0], r[1], r[2]}, d = {r[4], r[5], r[6]};
            const float tmax = r[3];
            const V3 P = cross3(d, e2);
            const float det = dot3(e1, P);
            if (!(det != 0.0f)) continue;
            const float inv = 1.0f / det;
            const V3 T = sub3(o, pa);
            const float u = dot3(T, P) * inv;
            if (!(u >= 0.0f && u <= 1.0f)) continue;
            const V3 Q = cross3(T, e1);
            const float v = dot3(d, Q) * inv;
            if (!(v >= 0.0f && (u + v) <= 1.0f)) continue;
            float t = dot3(e2, Q) * inv;
            if (!(t >= 0.0f && t <= tmax)) continue;
            t = t + 0.0f;
            ray_take(best[j], ((unsigned long long)__float_as_uint(t) << 32) | (unsigned)t_id, u, v);
        }
    }
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < kRayTile; ++j) {
        ray_reduce_wave(best[j]);
        if ((threadIdx.x & 63) == 0) wave_best[wave][j] = ray_pack(best[j]);
    }
    __syncthreads();
    const int j = threadIdx.x;
    if (j < kRayTile && ray0 + j < n_rays) {
        RayBest b = ray_unpack(wave_best[0][j]);
        for (int w = 1; w < kRayLanes / 64; ++w) { const RayBest o = ray_unpack(wave_best[w][j]); ray_take(b, o.key, o.u, o.v); }
        partials[(size_t)(ray0 + j) * gridDim.x + blockIdx.x] = ray_pack(b);
    }
}

// Workgroup r reduces ray r's n_partials partials by key and writes its sb_ray_hit -- triangle, t, u, v; a miss: -1, 0, 0, 0 -- in one
// 16-byte store.
__global__ __launch_bounds__(kRayLanes) void raycast_final_kernel(const uint4 *partials, int n_partials, uint4 *hits) {
    __shared__ uint4 wave_best[kRayLanes / 64];
    RayBest b = {kRayMiss, 0.0f, 0.0f};
    const uint4 *mine = partials + (size_t)blockIdx.x * n_partials;
    for (int g = threadIdx.x; g < n_partials; g += kRayLanes) { const RayBest o = ray_unpack(mine[g]); ray_take(b, o.key, o.u, o.v); }
    ray_reduce_wave(b);
    if ((threadIdx.x & 63) == 0) wave_best[threadIdx.x >> 6] = ray_pack(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kRayLanes / 64; ++w) { const RayBest o = ray_unpack(wave_best[w]); ray_take(b, o.key, o.u, o.v); }
        hits[blockIdx.x] = b.key == kRayMiss ? make_uint4(0xffffffffu, 0u, 0u, 0u) : make_uint4((unsigned)b.key, (unsigned)(b.key >> 32), __float_as_uint(b.u), __float_as_uint(b.v));
    }
}

}  // namespace sbk
