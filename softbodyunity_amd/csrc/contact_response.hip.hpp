// contact_response.hip.hpp — what the contact passes between two ticks share: the collider record, the response of SPEC.md 2f for a particle
// that is hit, the canonical NaN of a written component and the 16-byte store. Included by collide_kernels.hip.hpp (SPEC.md 2f, 2g) and
// heightfield_kernels.hip.hpp (SPEC.md 2h); the statements are the ones collide_kernels.hip.hpp held, moved here unchanged, so the collider
// kernels' code objects are what they were.
#pragma once
#include "device_math.hip.hpp"

namespace sbk {

// sb_collider as the kernel reads it (collide.hip asserts the two layouts equal): 128 bytes
struct ColliderRec {
    uint32_t shape, flags;
    float a[3], b[3], rot[9], half[3], radius, lin[3], ang[3], friction, restitution;
    int32_t reserved[3];
};

// SPEC.md 2f, the rule of 2c and 2d: a component that is WRITTEN and comes out NaN is stored as THE quiet NaN 0x7fc00000
__device__ __forceinline__ uint32_t collide_canonical_bits(float v) { return v == v ? __float_as_uint(v) : 0x7fc00000u; }

// The response of SPEC.md 2f for a particle that is hit. x: in and out (always written); v: in, and out when the function returns true
// (the particle approaches the collider); a separating particle's velocity is not written and keeps its bits.
__device__ __forceinline__ bool collide_respond(const ColliderRec &C, const float (&n)[3], float depth, uint32_t (&x)[3], uint32_t (&v)[3]) {
    float xn[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float push = depth * n[c];
        xn[c] = __uint_as_float(x[c]) + push;
        x[c] = collide_canonical_bits(xn[c]);
    }
    const float px = xn[0] - C.a[0], py = xn[1] - C.a[1], pz = xn[2] - C.a[2];
    const float yz = C.ang[1] * pz, zy = C.ang[2] * py;
    const float zx = C.ang[2] * px, xz = C.ang[0] * pz;
    const float xy = C.ang[0] * py, yx = C.ang[1] * px;
    const float cx = yz - zy, cy = zx - xz, cz = xy - yx;
    const float vc[3] = {C.lin[0] + cx, C.lin[1] + cy, C.lin[2] + cz};
    const float ux = __uint_as_float(v[0]) - vc[0], uy = __uint_as_float(v[1]) - vc[1], uz = __uint_as_float(v[2]) - vc[2];
    const float a = ux * n[0], b = uy * n[1], e = uz * n[2];
    const float ab = a + b;
    const float un = ab + e;
    if (!(un < 0.0f)) return false;
    const float jn = -un;
    const float ox = un * n[0], oy = un * n[1], oz = un * n[2];
    float t[3] = {ux - ox, uy - oy, uz - oz};
    const float txx = t[0] * t[0], tyy = t[1] * t[1], tzz = t[2] * t[2];
    const float txy = txx + tyy;
    const float t2 = txy + tzz;
    const float tl = sqrtf(t2);
    const float lim = C.friction * jn;
    const bool slip = t2 > 0.0f && tl > lim;
    const float ratio = lim / tl;
    const float scale = 1.0f - ratio;
    const float un2 = C.restitution * jn;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float st = scale * t[c];
        const float tc = slip ? st : 0.0f;
        const float nc = un2 * n[c];
        const float tn = tc + nc;
        v[c] = collide_canonical_bits(vc[c] + tn);
    }
    return true;
}

// One aligned 16-byte store, as placement's (placement_kernels.hip.hpp has the reasons: the compiler re-splits a lane's 48 bytes into
// 12-byte stores; the statement ends with the two wait states a store of more than 8 bytes needs before its data registers are reused).
typedef uint32_t collide_u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void collide_store4(uint4 *p, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    const collide_u32x4_t v = {a, b, c, d};
    asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}

}  // namespace sbk
