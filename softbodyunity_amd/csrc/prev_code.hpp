// prev_code.hpp — a previous position as 8 bytes, coded against the position x it is stored beside: the encoder (the tile kernels' final
// store) and the decoder (their prologue). Plain C++ for g++ and for device code, like stream_codec.hpp.
//
// No reference counterpart exists (/root/reference/README.md:1 is the whole reference tree).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SB_PREV_FN __host__ __device__ __forceinline__
#else
#define SB_PREV_FN inline
#endif

namespace sbk {

// Between two tile kernels a particle's previous position P differs from its position x by about h v, so per component the difference of
// the two BIT PATTERNS, k = bits(P) - bits(x) in uint32_t wrap-around arithmetic, is small. bits(P) = bits(x) + k holds for every pair of
// patterns -- signs, zeros, denormals, infinities, NaN payloads: no rounding is involved anywhere -- and a component fits when k, read
// as a signed number, lies in [-2^20, 2^20). The 64 bits: kx in bits 0-20, ky in 21-41, kz in 42-62, bit 63 = escape: some component
// does not fit, the particle's full 12-byte P stands at its usual place in the full-width array and the three fields mean nothing.
constexpr int kPrevFieldBits = 21;
constexpr uint32_t kPrevFieldMask = (1u << kPrevFieldBits) - 1u, kPrevHalf = 1u << (kPrevFieldBits - 1);
constexpr uint64_t kPrevEscape = 1ull << 63;

struct Bits3 { uint32_t x, y, z; };                     // the bit patterns of three floats
struct PrevCode { uint64_t code; bool fits; };

SB_PREV_FN bool prev_delta_fits(uint32_t k) { return k + kPrevHalf < 2u * kPrevHalf; }      // k as signed in [-2^20, 2^20)
SB_PREV_FN bool prev_is_escape(uint64_t code) { return (code >> 63) != 0; }
SB_PREV_FN bool prev_hi_is_escape(uint32_t code_hi) { return (code_hi >> 31) != 0; }        // the same on the upper dword alone
SB_PREV_FN PrevCode prev_encode(Bits3 P, Bits3 x) {
    const uint32_t kx = P.x - x.x, ky = P.y - x.y, kz = P.z - x.z;
    const bool fits = prev_delta_fits(kx) && prev_delta_fits(ky) && prev_delta_fits(kz);
    const uint64_t f = (uint64_t)(kx & kPrevFieldMask) | ((uint64_t)(ky & kPrevFieldMask) << kPrevFieldBits) | ((uint64_t)(kz & kPrevFieldMask) << (2 * kPrevFieldBits));
    return {fits ? f : kPrevEscape, fits};
}
// field -> k: sign extension of 21 bits without a signed type
SB_PREV_FN uint32_t prev_field_delta(uint32_t f) { return (f ^ kPrevHalf) - kPrevHalf; }
SB_PREV_FN Bits3 prev_decode(uint64_t code, Bits3 x) {
    const uint32_t fx = (uint32_t)code & kPrevFieldMask, fy = (uint32_t)(code >> kPrevFieldBits) & kPrevFieldMask, fz = (uint32_t)(code >> (2 * kPrevFieldBits)) & kPrevFieldMask;
    return {x.x + prev_field_delta(fx), x.y + prev_field_delta(fy), x.z + prev_field_delta(fz)};
}

}  // namespace sbk
