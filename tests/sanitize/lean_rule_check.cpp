// lean_rule_check.cpp — csrc/launch_shape.hpp use_lean_coded, the rule that gives a solver the lean coded tile kernels, on a machine
// without a GPU (tests/test_lean_rule.py). The lean kernels hold the register-resident engine alone and read a tile's slots only from
// the lane's own 16-byte word: a solver that ran them on a tile that is not lane-packed would decode a window that was never loaded.
// Checks, over a cross product of tiling scalars and solver inputs:
//   (a) lean implies use_prev_codes, at every point;
//   (b) lean == codes && every device tile of both tilings lane-packed && the longest program within kRegRoundsNarrow, spelled out here;
//   (c) from the headline's configuration each of these switches it off: one unpacked tile in T0, one in T1, a program above
//       kRegRoundsNarrow, a halo slot, world > 1, a T2 layer, float masses, a packed width other than 128; an empty T1 keeps it on;
//   (d) the LDS a lean launch asks for: positions + palette + 16 bytes, never more than the tiling's own.
// Prints "points N" and "lean K"; any violation is reported on stderr and makes the exit status 1.
#include <cstdio>

#include "launch_shape.hpp"

namespace {

long bad = 0;
void expect(bool ok, const char *what) {
    if (!ok) { ++bad; std::fprintf(stderr, "violated: %s\n", what); }
}

sbt::TilingScalars tiling(int n_tiles, long n_packed, int packed_lanes, int max_rounds, int max_local = 512) {
    sbt::TilingScalars D;
    D.n_tiles = n_tiles; D.n_packed_tiles = n_packed; D.packed_lanes = packed_lanes; D.max_local = max_local;
    D.rounds_dwords = (max_rounds + 3) & ~3; D.pal_dwords = 4; D.win_dwords = 4;
    D.lds_bytes = (size_t)D.max_local * 16 + (size_t)D.rounds_dwords * 4 + (size_t)D.pal_dwords * 4 + (size_t)D.win_dwords * 4 + 16;      // tables_host.cpp tiling_limits
    return D;
}

}  // namespace

int main() {
    static_assert(sbk::kLanePackDecodable, "the product build decodes lane-packed tiles");
    const int over = ((sbk::kRegRoundsNarrow + 3) & ~3) + 1;      // a program the padded round count cannot hide
    long points = 0, lean = 0;
    for (int n0 : {1, 7, 32768}) for (int n1 : {0, 1, 32778}) for (int miss0 : {0, 1}) for (int miss1 : {0, 1})
    for (int lanes0 : {0, 128, 256}) for (int lanes1 : {0, 128, 256}) for (int rounds : {1, sbk::kRegRoundsNarrow, over, 40})
    for (int world : {1, 2}) for (int halo : {0, 1}) for (int between : {0, 1}) for (int wpal : {0, 1}) for (int tile_lanes : {0, 128, 256}) {
        if (miss1 && n1 == 0) continue;
        ++points;
        const sbt::TilingScalars T0 = tiling(n0, lanes0 ? n0 - miss0 : 0, lanes0, rounds), T1 = tiling(n1, lanes1 ? n1 - miss1 : 0, lanes1, rounds);
        sbt::PrevCodeInputs in;
        in.world = world; in.halo_slots = halo; in.steps_between_tiles = between; in.w_palette = wpal != 0; in.tile_lanes = tile_lanes; in.n_local = 4096;
        const bool codes = sbt::use_prev_codes(T0, T1, in), got = sbt::use_lean_coded(T0, T1, in);
        const bool packed0 = lanes0 == 128 && !miss0, packed1 = n1 == 0 || (lanes1 == 128 && !miss1);
        // (the tiling records its longest program padded to four round words; a lane-packed tile holds at most kLanePackRounds by construction)
        const bool want = codes && packed0 && packed1 && ((rounds + 3) & ~3) <= ((sbk::kRegRoundsNarrow + 3) & ~3);
        expect(!got || codes, "(a) lean without codes");
        expect(got == want, "(b) the rule, spelled out");
        lean += got;
    }
    // (c) the headline: 256^3 at tile 512, both tilings all lane-packed, three rounds, one rank, palette masses
    const sbt::TilingScalars H0 = tiling(32768, 32768, 128, 3), H1 = tiling(32778, 32778, 128, 3);
    sbt::PrevCodeInputs in;
    in.w_palette = true; in.n_local = 16777216;
    expect(sbt::use_lean_coded(H0, H1, in), "(c) the headline runs the lean kernels");
    expect(!sbt::use_lean_coded(tiling(32768, 32767, 128, 3), H1, in), "(c) one unpacked tile in T0");
    expect(!sbt::use_lean_coded(H0, tiling(32778, 32777, 128, 3), in), "(c) one unpacked tile in T1");
    expect(!sbt::use_lean_coded(H0, tiling(32778, 0, 0, 3), in), "(c) a tiling without packed slots");
    expect(!sbt::use_lean_coded(tiling(32768, 32768, 128, over), H1, in), "(c) a program above kRegRoundsNarrow");
    expect(!sbt::use_lean_coded(tiling(32768, 32768, 256, 3), H1, in), "(c) 8-byte wide-packed slots");
    expect(sbt::use_lean_coded(H0, tiling(0, 0, 0, 0), in), "(c) an empty second tiling");
    { sbt::PrevCodeInputs q = in; q.halo_slots = 1; expect(!sbt::use_lean_coded(H0, H1, q), "(c) a halo slot"); }
    { sbt::PrevCodeInputs q = in; q.world = 2; expect(!sbt::use_lean_coded(H0, H1, q), "(c) world > 1"); }
    { sbt::PrevCodeInputs q = in; q.steps_between_tiles = 1; expect(!sbt::use_lean_coded(H0, H1, q), "(c) a T2 layer"); }
    { sbt::PrevCodeInputs q = in; q.w_palette = false; expect(!sbt::use_lean_coded(H0, H1, q), "(c) float masses"); }
    { sbt::PrevCodeInputs q = in; q.n_local = sbt::kPrevCodeMaxParticles + 1; expect(!sbt::use_lean_coded(H0, H1, q), "(c) beyond the coded size"); }
    // (d)
    for (int max_local : {1, 100, 512}) {
        const sbt::TilingScalars D = tiling(8, 8, 128, 3, max_local);
        expect(sbt::lean_lds_bytes(D) == (size_t)max_local * 16 + 4 * 4 + 16, "(d) positions + palette + 16 bytes");
        expect(sbt::lean_lds_bytes(D) <= D.lds_bytes, "(d) never more than the tiling's");
    }
    std::printf("points %ld\nlean %ld\n", points, lean);
    return bad ? 1 : 0;
}
