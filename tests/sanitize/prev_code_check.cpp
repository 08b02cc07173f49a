// prev_code_check.cpp — csrc/prev_code.hpp (previous positions as 8-byte codes against x) and the rule that decides who uses them
// (csrc/launch_shape.hpp use_prev_codes), on a machine without a GPU (tests/test_prev_code.py). Built with -fsanitize=address,undefined:
// the codec promises to do without signed subtraction and without a shift of a negative value.
//
//   (a) fits  <=>  every wrapped difference bits(P) - bits(x), read as a signed number, lies in [-2^20, 2^20) -- computed here in int64_t,
//       not with the header's expression;
//   (b) whenever fits, prev_decode(prev_encode(P, x).code, x) == P bit for bit and the escape bit is clear; whenever not, the code is the
//       escape bit alone;
//   (c) the decision function over its inputs.
// Prints "pairs N", "fitting N", "decisions N"; any violation is reported on stderr and makes the exit status 1.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "launch_shape.hpp"
#include "prev_code.hpp"

namespace {

long bad = 0, pairs = 0, fitting = 0;

uint32_t bits_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

bool want_fit(uint32_t p, uint32_t x) {
    const uint32_t k = p - x;                                          // wrap-around
    const int64_t sk = k < 0x80000000u ? (int64_t)k : (int64_t)k - ((int64_t)1 << 32);
    return sk >= -((int64_t)1 << 20) && sk < ((int64_t)1 << 20);
}

void check(sbk::Bits3 P, sbk::Bits3 x) {
    ++pairs;
    const bool want = want_fit(P.x, x.x) && want_fit(P.y, x.y) && want_fit(P.z, x.z);
    const sbk::PrevCode e = sbk::prev_encode(P, x);
    bool ok = e.fits == want && sbk::prev_is_escape(e.code) == !want && sbk::prev_hi_is_escape((uint32_t)(e.code >> 32)) == !want;
    if (want) {
        ++fitting;
        const sbk::Bits3 q = sbk::prev_decode(e.code, x);
        ok = ok && q.x == P.x && q.y == P.y && q.z == P.z;
    } else ok = ok && e.code == sbk::kPrevEscape;
    if (!ok) {
        ++bad;
        if (bad < 20) std::fprintf(stderr, "P %08x %08x %08x x %08x %08x %08x: fits %d (want %d) code %016llx\n", P.x, P.y, P.z, x.x, x.y, x.z, (int)e.fits, (int)want, (unsigned long long)e.code);
    }
}

}  // namespace

int main() {
    // ---- hand-picked bit patterns: every one as x, against x + d for the boundary differences, in every component
    const uint32_t xs[] = {
        0x00000000u, 0x80000000u,                               // +0, -0
        0x00000001u, 0x80000001u, 0x007fffffu, 0x807fffffu,     // denormals
        0x00800000u, 0x3f800000u, 0xbf800000u, 0x42c80000u,     // smallest normal, +-1, 100
        0x000fffffu, 0x80000005u,                               // a difference that crosses zero: the sign changes
        0x7f800000u, 0xff800000u,                               // +-inf
        0x7fc00000u, 0xffc00001u, 0x7f800001u, 0x7fffffffu, 0xffffffffu, 0x7fc12345u,     // NaNs with payloads
        0x7f7fffffu, 0xff7fffffu, 0xfff00000u, 0x000fffffu,     // largest finite; patterns whose sums wrap around 2^32
    };
    const uint32_t ds[] = {0u, 1u, 0xffffffffu, (1u << 20) - 1u, 1u << 20, (1u << 20) + 1u, 0u - (1u << 20), 0u - ((1u << 20) - 1u), 0u - ((1u << 20) + 1u),
                           0x80000000u, 0x7fffffffu, 0x00345678u, 0u - 0x00345678u, 0x000abcdeu, 0u - 0x000abcdeu};
    for (uint32_t x : xs) for (uint32_t d : ds) {
        const uint32_t p = x + d;
        check({p, x, x}, {x, x, x}); check({x, p, x}, {x, x, x}); check({x, x, p}, {x, x, x});
        check({p, p, p}, {x, x, x});
        for (uint32_t d2 : ds) check({p, x + d2, x - d}, {x, x, x});            // mixed components: one that does not fit makes the particle escape
    }
    // a sign change between floats proper: P = -1e-40f, x = +1e-40f and the like (equal inputs are the d = 0 cases above)
    const float fs[] = {0.0f, -0.0f, 1e-40f, -1e-40f, 1e-38f, 1.0f, 1.0000001f, -3.5f, 255.75f, 255.75002f, 1e30f};
    for (float a : fs) for (float b : fs) check({bits_of(a), bits_of(b), bits_of(a)}, {bits_of(b), bits_of(a), bits_of(a)});
    // ---- random pairs: arbitrary patterns (nearly all escape), and patterns near each other (nearly all fit, both sides of the boundary)
    std::mt19937_64 rng(20240611u);
    for (int n = 0; n < 400000; ++n) {
        const uint64_t a = rng(), b = rng(), c = rng();
        check({(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b}, {(uint32_t)(b >> 32), (uint32_t)c, (uint32_t)(c >> 32)});
    }
    for (int n = 0; n < 1200000; ++n) {
        const uint64_t a = rng(), b = rng(), c = rng();
        const sbk::Bits3 x{(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b};
        const uint32_t span = (n & 3) == 0 ? 23 : 21;            // differences of 21 bits always fit, of 23 bits mostly do not
        auto d = [&](uint64_t r) { return (uint32_t)(r & ((1u << span) - 1u)) - (1u << (span - 1)); };
        check({x.x + d(b >> 32), x.y + d(c), x.z + d(c >> 32)}, x);
    }
    // ---- the decision function (launch_shape.hpp): on for a single-rank spring lattice whose every launch is 128 x 4 with palette masses
    long decisions = 0;
    sbt::TilingScalars narrow;       // a lane-packed spring tiling: 128-lane workgroups in every launch
    narrow.n_tiles = 20000; narrow.max_local = 512; narrow.has_quads = false; narrow.packed_lanes = 128;
    sbt::PrevCodeInputs on;
    on.world = 1; on.halo_slots = 0; on.tile_lanes = 0; on.w_palette = true; on.steps_between_tiles = 0; on.n_local = 1 << 24;
    auto expect = [&](bool want, const sbt::TilingScalars &T0, const sbt::TilingScalars &T1, const sbt::PrevCodeInputs &in, const char *what) {
        ++decisions;
        if (sbt::use_prev_codes(T0, T1, in) != want) { ++bad; std::fprintf(stderr, "use_prev_codes: %s: expected %d\n", what, (int)want); }
    };
    expect(true, narrow, narrow, on, "the headline");
    { auto in = on; in.world = 2; expect(false, narrow, narrow, in, "world 2"); }
    { auto in = on; in.world = 8; expect(false, narrow, narrow, in, "world 8"); }
    { auto in = on; in.halo_slots = 1; expect(false, narrow, narrow, in, "halo slots (loopback)"); }
    { auto in = on; in.w_palette = false; expect(false, narrow, narrow, in, "float masses"); }
    { auto in = on; in.steps_between_tiles = 1; expect(false, narrow, narrow, in, "a T2 layer or a global colour between the tile kernels"); }
    { auto in = on; in.n_local = sbt::kPrevCodeMaxParticles + 1; expect(false, narrow, narrow, in, "beyond the particle limit"); }
    { auto in = on; in.n_local = sbt::kPrevCodeMaxParticles; expect(true, narrow, narrow, in, "at the particle limit"); }
    { auto q = narrow; q.has_quads = true; q.packed_lanes = 0; expect(false, q, narrow, on, "quads in T0"); expect(false, narrow, q, on, "quads in T1");
      auto in = on; in.tile_lanes = 128; expect(false, q, narrow, in, "quads in T0, 128 lanes forced"); }
    { auto w = narrow; w.packed_lanes = 256; expect(false, w, narrow, on, "wide-packed T0"); expect(false, narrow, w, on, "wide-packed T1"); }
    { auto u = narrow; u.packed_lanes = 0;       // not packed: the width follows the launch size unless tile_lanes forces it
      expect(false, u, narrow, on, "unpacked T0, width by launch size"); expect(false, narrow, u, on, "unpacked T1, width by launch size");
      for (int tl : {128, 256, 512}) { auto in = on; in.tile_lanes = tl; expect(tl == 128, u, u, in, "unpacked tilings, tile_lanes forced"); } }
    { auto big = narrow; big.max_local = 1024; big.packed_lanes = 0; auto in = on; in.tile_lanes = 128; expect(false, big, narrow, in, "large tiles"); }
    { sbt::TilingScalars none; expect(true, narrow, none, on, "one tiling only"); expect(false, none, none, on, "no tiles at all"); }
    // the rule agrees with the launch shape: wherever codes are on, every launch size gets the 128 x 4 spring shape
    for (int packed : {0, 128}) for (int tl : {0, 128}) for (int n : {1, 768, 769, 10239, 10240, 40000}) {
        auto T = narrow; T.packed_lanes = packed;
        auto in = on; in.tile_lanes = tl;
        ++decisions;
        if (!sbt::use_prev_codes(T, T, in)) continue;
        const sbt::LaunchShape sh = sbt::tile_launch_shape(T, tl, 512, 10240, n, false);
        if (!(sbt::same_width(sh, sbt::kShapeNarrow) && !sh.quads)) { ++bad; std::fprintf(stderr, "codes on, but a launch of %d tiles is %d x %d\n", n, sh.threads, sh.ppt); }
    }
    std::printf("pairs %ld\nfitting %ld\ndecisions %ld\n", pairs, fitting, decisions);
    return bad ? 1 : 0;
}
