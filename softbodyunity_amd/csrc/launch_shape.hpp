// launch_shape.hpp — which tile_kernel instantiation a launch runs (the template arguments THREADS, PPT, QUADS), as a pure function of the
// tiling's scalars, three tuning values and the number of tiles in the launch. Host only, compiled with g++ like tables_host.cpp: no HIP
// runtime call, no solver object. schedule.hip launch_tile dispatches on the answer; tests/sanitize/launch_shape_check.cpp walks the rule.
// The rule is a CONTRACT: tables_host.cpp choose_packed_lanes packs slots only where every launch of the tiling runs workgroups of
// packed_lanes lanes, and the kernel takes its fast paths only if kTileThreads == 64 * item_waves or td.packed_lanes == kTileThreads -- a
// tile launched at another width decodes a window that was never staged: wrong bits, not an error.
#pragma once
#include "kernel_types.hpp"
#include "tables_host.hpp"

namespace sbt {

struct LaunchShape { int threads, ppt; bool quads; };      // lanes per tile, particles per lane, tiles with four-lane constraints
inline bool same_width(const LaunchShape &a, const LaunchShape &b) { return a.threads == b.threads && a.ppt == b.ppt; }

// The five (THREADS, PPT) pairs the kernels are built for (THREADS x PPT = the capacity kSmallTile or kLargeTile); `quads` is set per launch.
constexpr LaunchShape kShapeNarrow{sbk::kNarrowTileThreads, sbk::kSmallTile / sbk::kNarrowTileThreads, false};     // 128 x 4
constexpr LaunchShape kShapeWide{sbk::kWideTileThreads, sbk::kSmallTile / sbk::kWideTileThreads, false};           // 256 x 2
constexpr LaunchShape kShapeWideLarge{sbk::kWideTileThreads, sbk::kLargeTile / sbk::kWideTileThreads, false};      // 256 x 4
constexpr LaunchShape kShapeEight{sbk::kQuadTileThreads, sbk::kSmallTile / sbk::kQuadTileThreads, false};          // 512 x 1
constexpr LaunchShape kShapeEightLarge{sbk::kQuadTileThreads, sbk::kLargeTile / sbk::kQuadTileThreads, false};     // 512 x 2 (with quads only)

// tile_lanes, quad_lanes, narrow_min_tiles: sb_solver's tuning fields of those names; n_tiles_in_launch: of THIS launch (a boundary /
// interior split, a T2 layer, the peek's subset), not of the tiling; ghosts: the launch reads its ghosts from the receive buffer.
inline LaunchShape tile_launch_shape(const TilingScalars &D, int tile_lanes, int quad_lanes, int narrow_min_tiles, int n_tiles_in_launch, bool ghosts) {
    const bool small = D.max_local <= sbk::kSmallTile;   // every tile <= 512 particles
    // narrow (2-wave) workgroups once the launch oversubscribes the chip; wide ones while every tile is resident at once
    // (a tiling with lane-packed slots runs 128-lane workgroups in EVERY launch, also the peek's subset of its tiles)
    // (a tiling with 8-byte wide-packed slots likewise runs 256-lane workgroups in every launch)
    const bool narrow = small && (D.packed_lanes ? D.packed_lanes == sbk::kLanePackLanes : (tile_lanes ? tile_lanes == sbk::kNarrowTileThreads : n_tiles_in_launch >= narrow_min_tiles));
    // tiles with tets / hinges: optionally 8 waves, so that a group's wave slots (16 four-lane constraints or 64 springs each) fit one row
    const bool quad8 = D.has_quads && quad_lanes == sbk::kQuadTileThreads;
    // spring-only small tiles on 8 waves (one particle per lane in the load / MARK / store phases; the rounds use half the lanes) while
    // every workgroup of the launch is resident even at that width (4 per compute unit): 64^3 0.1244 -> 0.1213, 48^3 0.1027 -> 0.1005 ms
    // per tick; 96^3 (1 728 tiles) 0.206 -> 0.230, so only launches of at most kWide8MaxTiles (profiles/r03o_lanes512_small_cubes.txt)
    const bool wide8 = small && !D.has_quads && !D.packed_lanes && (tile_lanes ? tile_lanes == sbk::kQuadTileThreads : n_tiles_in_launch <= sbk::kWide8MaxTiles);
    const bool quads = ghosts ? false : D.has_quads;     // (the ghost-reading kernels exist for spring-only tilings)
    LaunchShape sh = quads && quad8 ? (small ? kShapeEight : kShapeEightLarge) : wide8 ? kShapeEight : narrow ? kShapeNarrow : small ? kShapeWide : kShapeWideLarge;
    sh.quads = quads;            // (wide8 implies !has_quads: that shape is spring-only by itself)
    return sh;
}

// ---- previous positions as 8-byte codes (prev_code.hpp) ---------------------------------------------------------------------------------
// Decided once per solver (sb_finalize), not per launch: a code is written by one tile kernel and read by the next, so either every tile
// launch of the tick runs a coded kernel or none does. The coded kernels are built for 128 x 4 spring-only launches with palette masses.
// every launch of the tiling is 128 x 4 without quads, whatever its number of tiles (the tiling-level part of `narrow` above; wide8 is off then)
inline bool tiling_always_narrow(const TilingScalars &D, int tile_lanes) {
    if (D.n_tiles == 0) return true;       // (a plan with one tiling: the other one is never launched)
    return D.max_local <= sbk::kSmallTile && !D.has_quads && (D.packed_lanes ? D.packed_lanes == sbk::kLanePackLanes : tile_lanes == sbk::kNarrowTileThreads);
}
// The 512^3 check of tests/test_gpu_full_size.py holds sb_stats.launch_bytes of that lattice to the full-width format (> 7e9 B per launch); until
// that figure is recorded anew, lattices beyond this many local particles keep the full-width path. No property of the code sets the limit.
constexpr int64_t kPrevCodeMaxParticles = (int64_t)1 << 26;
struct PrevCodeInputs {
    int world = 1;
    int halo_slots = 0;              // active halo slots (a loopback solver has world 1 and halo slots)
    int tile_lanes = 0;              // sb_solver's tuning field
    bool w_palette = false;          // the kernels read palette masses (WPAL)
    int steps_between_tiles = 0;     // T2 layers + global colours: they move x between two tile kernels, and a code is relative to the x stored beside it
    int64_t n_local = 0;
};
inline bool use_prev_codes(const TilingScalars &T0, const TilingScalars &T1, const PrevCodeInputs &in) {
    if (in.world != 1 || in.halo_slots != 0) return false;                    // ghosts, halo pack / unpack and peer push read full-width previous positions
    if (!in.w_palette) return false;                                          // the float-mass kernels have no registers left for it
    if (in.steps_between_tiles != 0) return false;
    if (T0.n_tiles == 0 || in.n_local > kPrevCodeMaxParticles) return false;
    return tiling_always_narrow(T0, in.tile_lanes) && tiling_always_narrow(T1, in.tile_lanes);
}

// ---- the lean coded kernels (tile_kernel LEAN) --------------------------------------------------------------------------------------------
// Decided with use_prev_codes, once per solver: every tile launch of the tick runs a lean kernel or none does. A lean kernel holds the
// register-resident engine alone and reads a tile's slots only from the lane's own 16-byte word, so EVERY device tile of both tilings must
// be lane-packed -- which, with palette masses, also makes it dictionary-coded (tables_host.cpp pack_form) -- and its program must fit the
// registers of a 128-lane workgroup. A coded lattice with one rim pack that zips into more rounds keeps the general coded kernels.
inline bool tiling_all_lane_packed(const TilingScalars &D) {
    if (D.n_tiles == 0) return true;       // (a plan with one tiling: the other one is never launched)
    return D.packed_lanes == sbk::kLanePackLanes && D.n_packed_tiles == (int64_t)D.n_tiles &&
           D.rounds_dwords <= ((sbk::kRegRoundsNarrow + 3) & ~3);      // (rounds_dwords: the tiling's longest program, padded to 4)
}
inline bool use_lean_coded(const TilingScalars &T0, const TilingScalars &T1, const PrevCodeInputs &in) {
    if (!use_prev_codes(T0, T1, in) || !sbk::kLanePackDecodable) return false;
    return tiling_all_lane_packed(T0) && tiling_all_lane_packed(T1);
}
// LDS of a lean launch: positions, the palette, the 16 spare bytes -- no round words, no window (the tiling's lds_bytes holds both)
inline size_t lean_lds_bytes(const TilingScalars &D) { return (size_t)D.max_local * sizeof(float4) + (size_t)D.pal_dwords * 4 + 16; }

}  // namespace sbt
