// body_state_kernels.hip.hpp — SPEC.md §6f: the mass-weighted sums behind centre of mass, momenta and the best-fit rotation, reduced over
// the particles a rank owns in two launches and without atomics (the shape of the bounds reduction in readback_kernels.hip.hpp)
#pragma once
#include "device_math.hip.hpp"

namespace sbk {

constexpr int kBodyLanes = 256;
constexpr int kBodyMaxGroups = 1024;    // grid cap of body_sums_partial_kernel: 4 waves per SIMD on 256 CUs (the f64 accumulators of a query for
                                        // both bits leave room for about five); larger sets walk the grid-stride loop
constexpr int kBodySums = 32;           // SPEC.md §6f: the slots of a row
constexpr int kBodyRow = kBodySums + 2; // a row of the partials, in 8-byte words: the sums, then the two counts (dynamic, pinned) as int64
constexpr unsigned kBodyPose = 1u, kBodyMotion = 2u;      // = SB_BODY_POSE, SB_BODY_MOTION (body_state.hip asserts it)

// Which slots a query produces (SPEC.md §6f's table); one that is not requested is never accumulated and is written as 0.
template <unsigned WHAT>
__device__ __forceinline__ constexpr bool body_slot_wanted(int k) {
    const bool p = (WHAT & kBodyPose) != 0, m = (WHAT & kBodyMotion) != 0;
    return k <= 3 ? true : k <= 6 ? p : k <= 12 ? true : k <= 21 ? p : k <= 28 ? m : false;
}

__device__ __forceinline__ double body_shfl_xor(double v, int mask) {
    return __hiloint2double(__shfl_xor(__double2hiint(v), mask, 64), __shfl_xor(__double2loint(v), mask, 64));
}

// Lane k of the grid walks rows k, k + grid, ... of the packed arrays (device order: neighbouring lanes read neighbouring 12-byte rows, one
// 768-byte run per wave and array, and 256 bytes of inverse masses): 28 bytes per particle for one bit, 40 for both. A dynamic particle
// (w > 0) enters every requested sum with m = 1 / (double)w; a pinned one is counted and nothing else of it is used (its coordinates may be
// anything). Every statement is binary64. Then the wave64 butterfly on the two halves of each double, the four waves through LDS in wave
// order, and lane 0 writes the workgroup's row: partials[kBodyRow * g ..] = 32 sums, n_dynamic, n_pinned.
template <unsigned WHAT>
__global__ __launch_bounds__(kBodyLanes) void body_sums_partial_kernel(const float *xyz, const float *vel, const float *ref, const float *wf,
                                                                       int64_t count, double *partials) {
    constexpr bool P = (WHAT & kBodyPose) != 0, M = (WHAT & kBodyMotion) != 0;
    static_assert(WHAT == kBodyPose || WHAT == kBodyMotion || WHAT == (kBodyPose | kBodyMotion), "a query asks for POSE, MOTION or both");
    double s[kBodySums];
#pragma unroll
    for (int k = 0; k < kBodySums; ++k) s[k] = 0.0;
    int32_t n_dyn = 0, n_pin = 0;
    const int64_t stride = (int64_t)gridDim.x * kBodyLanes;
    for (int64_t k = (int64_t)blockIdx.x * kBodyLanes + threadIdx.x; k < count; k += stride) {
        const size_t o = 3 * (size_t)k;
        const float w = wf[k];
        const float fx = xyz[o], fy = xyz[o + 1], fz = xyz[o + 2];
        float qx = 0.0f, qy = 0.0f, qz = 0.0f, ux = 0.0f, uy = 0.0f, uz = 0.0f;
        if (P) { qx = ref[o]; qy = ref[o + 1]; qz = ref[o + 2]; }
        if (M) { ux = vel[o]; uy = vel[o + 1]; uz = vel[o + 2]; }
        if (!(w > 0.0f)) { ++n_pin; continue; }
        ++n_dyn;
        const double m = 1.0 / (double)w;
        const double x = (double)fx, y = (double)fy, z = (double)fz;
        const double mx = m * x, my = m * y, mz = m * z;
        s[0] += m;
        s[1] += mx; s[2] += my; s[3] += mz;
        s[7] += mx * x; s[8] += my * y; s[9] += mz * z; s[10] += mx * y; s[11] += mx * z; s[12] += my * z;
        if (P) {
            const double a = (double)qx, b = (double)qy, c = (double)qz;
            s[4] += m * a; s[5] += m * b; s[6] += m * c;
            s[13] += mx * a; s[14] += mx * b; s[15] += mx * c;
            s[16] += my * a; s[17] += my * b; s[18] += my * c;
            s[19] += mz * a; s[20] += mz * b; s[21] += mz * c;
        }
        if (M) {
            const double a = (double)ux, b = (double)uy, c = (double)uz;
            const double ma = m * a, mb = m * b, mc = m * c;
            s[22] += ma; s[23] += mb; s[24] += mc;
            s[25] += my * c - mz * b; s[26] += mz * a - mx * c; s[27] += mx * b - my * a;
            s[28] += (ma * a + mb * b) + mc * c;
        }
    }
    // the workgroup's row: butterfly inside each wave, then waves 1 .. 3 onto wave 0 in that order
    __shared__ double wave_sum[kBodyLanes / 64][kBodySums];
    __shared__ int32_t wave_cnt[kBodyLanes / 64][2];
#pragma unroll
    for (int k = 0; k < kBodySums; ++k) {
        if (!body_slot_wanted<WHAT>(k)) continue;
        for (int msk = 32; msk >= 1; msk >>= 1) s[k] += body_shfl_xor(s[k], msk);
    }
    for (int msk = 32; msk >= 1; msk >>= 1) { n_dyn += __shfl_xor(n_dyn, msk, 64); n_pin += __shfl_xor(n_pin, msk, 64); }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < kBodySums; ++k) wave_sum[wave][k] = s[k];
        wave_cnt[wave][0] = n_dyn; wave_cnt[wave][1] = n_pin;
    }
    __syncthreads();
    if (threadIdx.x < kBodyRow) {
        double *row = partials + (size_t)kBodyRow * blockIdx.x;
        const int k = threadIdx.x;
        if (k < kBodySums) {
            double t = wave_sum[0][k];
            for (int wv = 1; wv < kBodyLanes / 64; ++wv) t += wave_sum[wv][k];
            row[k] = t;
        } else {
            int64_t t = 0;
            for (int wv = 0; wv < kBodyLanes / 64; ++wv) t += wave_cnt[wv][k - kBodySums];
            row[k] = __longlong_as_double((long long)t);
        }
    }
}

// One workgroup adds the n_partials rows in a fixed order -- 32 runs of consecutive rows, each added in index order by one lane per slot,
// then the 32 run sums in run order -- and writes 32 doubles and the two counts to out34 (mapped pinned memory). 0 rows: all zeros.
// A run's rows are fetched eight at a time before they are added: the additions keep their order, the loads do not wait for one another
// (one dependent load per row made this kernel a third of a query's time at 256^3).
constexpr int kBodyFinalLanes = 1024;
__global__ __launch_bounds__(kBodyFinalLanes) void body_sums_final_kernel(const double *__restrict__ partials, int n_partials, double *__restrict__ out34) {
    constexpr int kRuns = kBodyFinalLanes / kBodySums;      // 32
    constexpr int kBatch = 8;
    __shared__ double run_sum[kRuns][kBodySums];
    __shared__ long long run_cnt[kBodyFinalLanes / 64][2];
    const int slot = threadIdx.x % kBodySums, run = threadIdx.x / kBodySums;
    const int per_run = (n_partials + kRuns - 1) / kRuns;
    const int g0 = run * per_run, g1 = min(n_partials, g0 + per_run);
    double t = 0.0;
    for (int g = g0; g < g1; g += kBatch) {
        double v[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) v[j] = g + j < g1 ? partials[(size_t)kBodyRow * (g + j) + slot] : 0.0;
#pragma unroll
        for (int j = 0; j < kBatch; ++j) if (g + j < g1) t += v[j];
    }
    run_sum[run][slot] = t;
    // the counts: integers, any order
    long long nd = 0, np = 0;
    for (int g = threadIdx.x; g < n_partials; g += kBodyFinalLanes) {
        nd += __double_as_longlong(partials[(size_t)kBodyRow * g + kBodySums]);
        np += __double_as_longlong(partials[(size_t)kBodyRow * g + kBodySums + 1]);
    }
    for (int msk = 32; msk >= 1; msk >>= 1) {
        nd += __double_as_longlong(body_shfl_xor(__longlong_as_double(nd), msk));
        np += __double_as_longlong(body_shfl_xor(__longlong_as_double(np), msk));
    }
    if ((threadIdx.x & 63) == 0) { run_cnt[threadIdx.x >> 6][0] = nd; run_cnt[threadIdx.x >> 6][1] = np; }
    __syncthreads();
    if (threadIdx.x < kBodySums) {
        double r = run_sum[0][threadIdx.x];
        for (int q = 1; q < kRuns; ++q) r += run_sum[q][threadIdx.x];
        out34[threadIdx.x] = r;
    } else if (threadIdx.x < kBodyRow) {
        const int c = threadIdx.x - kBodySums;
        long long r = 0;
        for (int wv = 0; wv < kBodyFinalLanes / 64; ++wv) r += run_cnt[wv][c];
        out34[threadIdx.x] = __longlong_as_double(r);
    }
}

}  // namespace sbk
