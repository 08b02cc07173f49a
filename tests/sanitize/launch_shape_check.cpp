// launch_shape_check.cpp — csrc/launch_shape.hpp against the rule it replaced, on a machine without a GPU (tests/test_launch_shape.py).
//
// Walks the whole cross product of tiling scalars, tuning values and launch sizes given below and checks at every point
//   (a) equality with the parent's rule: the five boolean lines, the block size and the branch order of launch_tile / SB_LAUNCH_TILE as
//       they stood in csrc/schedule.hip at commit 1cb47a8, transcribed here -- the reference; it is not derived from the new header;
//   (b) the contract with the table builder and the kernel (launch_shape.hpp);
//   (c) coverage: every shape the kernels are built for, with and without quads where that is legal, is returned somewhere.
// Prints "points N" and "shapes K"; any violation is reported on stderr and makes the exit status 1.
#include <cstdio>
#include <set>
#include <tuple>

#include "launch_shape.hpp"

namespace {

struct Ref { int threads, ppt; bool quads; int block; bool narrow; };

// schedule.hip at 1cb47a8, launch_tile: `s` is the solver, D the tiling, the launch covers tiles [tile_begin, tile_end)
struct SolverFields { int tile_lanes, quad_lanes, narrow_min_tiles; };
Ref parent_rule(const SolverFields *s, const sbt::TilingScalars &D, int tile_begin, int tile_end, bool ghosts) {
    const bool small = D.max_local <= sbk::kSmallTile;   // every tile <= 512 particles
    const bool narrow = small && (D.packed_lanes ? D.packed_lanes == sbk::kLanePackLanes : (s->tile_lanes ? s->tile_lanes == sbk::kNarrowTileThreads : tile_end - tile_begin >= s->narrow_min_tiles));
    const bool quad8 = D.has_quads && s->quad_lanes == sbk::kQuadTileThreads;
    constexpr int kWide8MaxTiles = sbk::kWide8MaxTiles;
    const bool wide8 = small && !D.has_quads && !D.packed_lanes && (s->tile_lanes ? s->tile_lanes == 512 : tile_end - tile_begin <= kWide8MaxTiles);
    const int block(quad8 || wide8 ? sbk::kQuadTileThreads : (narrow ? sbk::kNarrowTileThreads : sbk::kWideTileThreads));
    // SB_LAUNCH_TILE(Q, W, G): a ghost-reading launch expands it with Q = false, every other one with Q = D.has_quads
    const bool Q = ghosts ? false : D.has_quads;
    if (Q && quad8) {
        if (small) return Ref{sbk::kQuadTileThreads, sbk::kSmallTile / sbk::kQuadTileThreads, true, block, narrow};
        else return Ref{sbk::kQuadTileThreads, sbk::kLargeTile / sbk::kQuadTileThreads, true, block, narrow};
    } else if (wide8) return Ref{sbk::kQuadTileThreads, sbk::kSmallTile / sbk::kQuadTileThreads, false, block, narrow};
    else if (narrow) return Ref{sbk::kNarrowTileThreads, sbk::kSmallTile / sbk::kNarrowTileThreads, Q, block, narrow};
    else if (small) return Ref{sbk::kWideTileThreads, sbk::kSmallTile / sbk::kWideTileThreads, Q, block, narrow};
    else return Ref{sbk::kWideTileThreads, sbk::kLargeTile / sbk::kWideTileThreads, Q, block, narrow};
}

}  // namespace

int main() {
    const int legal[5][2] = {{128, 4}, {256, 2}, {256, 4}, {512, 1}, {512, 2}};
    std::set<std::tuple<int, int, bool>> seen;
    long points = 0, bad = 0;
    for (int max_local : {1, 512, 513, 1024}) for (int has_quads : {0, 1}) for (int packed_lanes : {0, 128, 256})
    for (int tile_lanes : {0, 128, 256, 512}) for (int quad_lanes : {256, 512}) for (int nmt : {1, 769, 10240})
    for (int n : {1, 768, 769, nmt - 1, nmt, 40000}) for (int ghosts : {0, 1}) {
        if (packed_lanes && !(max_local <= 512 && !has_quads)) continue;      // what the builder can produce
        if (n <= 0 || (ghosts && has_quads)) continue;
        ++points;
        sbt::TilingScalars D;
        D.max_local = max_local; D.has_quads = has_quads != 0; D.packed_lanes = packed_lanes;
        const SolverFields S{tile_lanes, quad_lanes, nmt};
        const Ref want = parent_rule(&S, D, 0, n, ghosts != 0);
        const sbt::LaunchShape got = sbt::tile_launch_shape(D, tile_lanes, quad_lanes, nmt, n, ghosts != 0);
        bool is_legal = false;
        for (const auto &p : legal) is_legal = is_legal || (got.threads == p[0] && got.ppt == p[1]);
        const bool ok =
            got.threads == want.threads && got.ppt == want.ppt && got.quads == want.quads && got.threads == want.block &&      // (a)
            is_legal && got.threads * got.ppt >= max_local &&                                                                   // (b)
            (!packed_lanes || got.threads == packed_lanes) && (!ghosts || !got.quads) &&
            (!(has_quads && quad_lanes == 512 && !ghosts) || got.threads == 512) &&
            (!(has_quads && quad_lanes == 256 && !ghosts && !want.narrow) || got.threads == 256);
        if (!ok) {
            ++bad;
            std::fprintf(stderr, "max_local %d has_quads %d packed_lanes %d tile_lanes %d quad_lanes %d narrow_min_tiles %d n %d ghosts %d: got (%d, %d, %d), parent (%d, %d, %d) block %d\n",
                         max_local, has_quads, packed_lanes, tile_lanes, quad_lanes, nmt, n, ghosts, got.threads, got.ppt, (int)got.quads,
                         want.threads, want.ppt, (int)want.quads, want.block);
        }
        seen.insert({got.threads, got.ppt, got.quads});
    }
    for (const auto &p : legal) for (bool q : {false, true}) {      // (c): 512 x 2 is built with quads only
        if (p[0] == 512 && p[1] == 2 && !q) continue;
        if (!seen.count({p[0], p[1], q})) { ++bad; std::fprintf(stderr, "shape (%d, %d, %d) is never returned\n", p[0], p[1], (int)q); }
    }
    std::printf("points %ld\nshapes %zu\n", points, seen.size());
    return bad ? 1 : 0;
}
