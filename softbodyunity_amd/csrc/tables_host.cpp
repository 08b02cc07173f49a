// tables_host.cpp — see tables_host.hpp. Host arithmetic only: what tables.hip uploads byte for byte.
//
// No reference counterpart exists (/root/reference/README.md:1 is the whole reference tree).
//
// Map of the file (a stage reads its arguments and writes its result; nothing else is shared):
//   helpers            float_bits, layer_of, pack_field, xcd_position (the stream's bit fields: stream_codec.hpp)
//   build_state        pack_state, mass_palette
//   build_tiling       boundary_order          T0 boundary tiles first, T1 boundary tiles last (world > 1)
//                      pack_tiles              best fit of under-full tiles into workgroups, by layer / boundary class
//                      t2_layer_ranges         device-tile range of every T2 layer
//                      choose_packed_lanes     may this tiling hold lane-packed (128) or wide-packed (256) slots
//                      build_pack              one pack: pack_descriptor (runs), zip_rounds (program), rest_dictionary,
//                                              emit_wave_items, then ONE of emit_lane_packed / emit_wide_packed / emit_slots
//                      place_pieces            the host threads' pieces laid end to end, offsets re-based
//                      share_programs          one copy of every distinct program, shared ones first
//                      cost_order              heavy tiles first inside small launches, through the kernel's XCD remap
//                      tiling_limits           LDS carve and the counts sb_stats reports
//   build_gcolours
//   build_halos        halo_lists, fused_unpack_ok, mailbox_layout
#include "tables_host.hpp"

#include <algorithm>
#include <atomic>
#include <climits>
#include <cstring>
#include <stdexcept>

#include "../../include/softbody_debug.h"

namespace sbt {
namespace {

uint32_t float_bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// the T2 layer a plan tile of T[2] belongs to
int layer_of(const sbp::Plan &P, int32_t plan_tile) {
    int ly = 0;
    while (ly + 1 < (int)P.t2_layers.size() && plan_tile >= P.t2_layers[ly].second) ++ly;
    return ly;
}

// the 21-bit field of the lane-packed and the wide-packed words for the index pair `idx`
uint32_t pack_field(uint32_t idx, uint32_t pal_index, const char *what) {
    const sbk::IndexPair p = sbk::decode_index_pair(idx);
    if (!sbk::pack_field_fits(p.i, p.j, pal_index)) throw std::runtime_error(what);
    return sbk::encode_pack_field(p.i, p.j, pal_index);
}

// The tile that workgroup `wg` of a launch of `n` workgroups reads. Must match the XCD remap at the head of tile_kernel
// (tile_kernel.hip.hpp, `tile_index`): workgroups are dealt round-robin over 8 XCDs, each XCD gets a contiguous range of tiles.
int32_t xcd_position(int32_t wg, int32_t n) {
    const int32_t xq = n >> 3, xr = n & 7, xcd = wg & 7;
    return (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (wg >> 3);
}

// ---- particle state -----------------------------------------------------------------------------------------------------------------------

void pack_state(const TableInput &in, HostTables &H) {
    const sbp::LocalPlan &L = *in.local;
    H.n_owned = L.n_owned;
    H.n_local = (int64_t)L.local_to_old.size();
    H.pos3.assign((size_t)H.n_local * 3, 0.0f); H.vel.assign((size_t)H.n_local * 3, 0.0f); H.wf.assign((size_t)H.n_local, 0.0f);
    sbp::parallel_for_chunks(H.n_local, 1 << 18, [&](int64_t, int64_t lb, int64_t le) {
        for (int64_t l = lb; l < le; ++l) {
            const int32_t o = L.local_to_old[l];
            for (int c = 0; c < 3; ++c) { H.pos3[3 * (size_t)l + c] = in.pos[3 * (size_t)o + c]; H.vel[3 * (size_t)l + c] = in.vel[3 * (size_t)o + c]; }
            H.wf[l] = in.invm[o];
        }
    });
}

// one byte per particle instead of four when the mesh uses few distinct masses (the usual case)
void mass_palette(const TableOptions &opt, HostTables &H) {
    const std::vector<float> &hw = H.wf;
    std::vector<uint32_t> vals(hw.size());
    for (size_t l = 0; l < hw.size(); ++l) vals[l] = float_bits(hw[l]);
    std::vector<uint32_t> uniq;           // sorted distinct bit patterns, given up beyond the palette size
    bool few = true;
    {
        uint32_t last = 0; bool have_last = false;
        for (uint32_t v : vals) {
            if (have_last && v == last) continue;
            last = v; have_last = true;
            auto it = std::lower_bound(uniq.begin(), uniq.end(), v);
            if (it != uniq.end() && *it == v) continue;
            if ((int)uniq.size() == sbk::kMaxMassPalette) { few = false; break; }
            uniq.insert(it, v);
        }
    }
    H.wpal.assign(sbk::kMaxMassPalette, 0.0f);
    H.w8.clear(); H.w_palette = H.w_uniform = false;
    if (!few || (opt.tune_flags & SB_TUNE_NO_MASS_PALETTE)) return;
    H.w8.resize(hw.size());
    sbp::parallel_for_chunks((int64_t)hw.size(), 1 << 20, [&](int64_t, int64_t lb, int64_t le) {
        for (int64_t l = lb; l < le; ++l) H.w8[(size_t)l] = (uint8_t)(std::lower_bound(uniq.begin(), uniq.end(), vals[(size_t)l]) - uniq.begin());
    });
    for (size_t k = 0; k < uniq.size(); ++k) std::memcpy(&H.wpal[k], &uniq[k], 4);
    H.w_palette = true;
    H.w_uniform = uniq.size() == 1 && !(opt.tune_flags & SB_TUNE_NO_UNIFORM_MASS);
}

// ---- a tiling: which plan tiles share a workgroup, in which order -------------------------------------------------------------------------

// world > 1: T0 launches run the tiles that hold sent particles FIRST, T1 launches run the tiles that hold a ghost or a sent
// particle LAST: the ghost exchange between a T0 and the following T1 kernel can then travel beside the T0 interior tiles and
// the T1 interior tiles, which touch none of the particles the pack kernel reads or the unpack kernel writes (enqueue_substeps,
// overlapped schedule). Re-orders LT; returns, per tile of the re-ordered LT, whether it is a boundary tile (empty: no re-ordering).
std::vector<uint8_t> boundary_order(const sbp::LocalPlan &L, int tl, int64_t n_owned, int64_t n_local, sbp::LocalTiling &LT) {
    std::vector<uint8_t> tile_is_b;
    if (!((tl == 0 || tl == 1) && L.world > 1 && L.halo.size() > 1)) return tile_is_b;
    std::vector<uint8_t> sent((size_t)n_local, 0);
    for (const auto &lst : L.halo[1].send_idx) for (int32_t li : lst) sent[li] = 1;
    std::vector<int32_t> order(LT.tile_ids.size());
    std::vector<uint8_t> is_b(LT.tile_ids.size(), 0);
    for (size_t ci = 0; ci < LT.tile_ids.size(); ++ci) {
        order[ci] = (int32_t)ci;
        for (int32_t r = LT.run_begin[ci]; r < LT.run_begin[ci + 1] && !is_b[ci]; ++r) {
            if (tl == 1 && (int64_t)LT.runs[r].start + LT.runs[r].len > n_owned) { is_b[ci] = 1; break; }   // a ghost run
            for (int32_t q = 0; q < LT.runs[r].len; ++q) if (sent[LT.runs[r].start + q]) { is_b[ci] = 1; break; }
        }
    }
    if (tl == 0) std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return is_b[a] > is_b[b]; });
    else std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return is_b[a] < is_b[b]; });
    sbp::LocalTiling R;
    R.run_begin.push_back(0);
    for (int32_t ci : order) {
        R.tile_ids.push_back(LT.tile_ids[ci]);
        for (int32_t r = LT.run_begin[ci]; r < LT.run_begin[ci + 1]; ++r) R.runs.push_back(LT.runs[r]);
        R.run_begin.push_back((int32_t)R.runs.size());
        tile_is_b.push_back(is_b[ci]);
    }
    LT = R;
    return tile_is_b;
}

// Packing: a tile is only a set of particles whose own constraints are projected in LDS, so several under-full plan tiles (the
// rim of the shifted grid, surface cells of an irregular mesh) can share one workgroup: their particles are staged side by side
// and round r of the pack is the union of the members' next rounds of one type. Members share no particle and keep their own
// round order, so the result is bit-identical to running them one after the other (the published order); only the number of
// workgroups changes. Returns the packs (members = indices into LT.tile_ids, in execution order) and how many hold boundary tiles.
std::vector<std::vector<int32_t>> pack_tiles(const sbp::Plan &P, const sbp::Tiling &G, const sbp::LocalTiling &LT, int tl,
                                             const std::vector<uint8_t> &tile_is_b, bool enabled, int32_t &n_boundary_packs) {
    const size_t n_plan_tiles = LT.tile_ids.size();
    const int capacity = sbk::kSmallTile;         // packs stay small tiles; plan tiles above that size are left alone
    // only tiles with short programs share a workgroup (the rim of a lattice: 3-4 rounds): zipping long programs of
    // an irregular mesh (40+ rounds per tile) lengthens them, and such launches do not fill the chip anyway
    constexpr int kPackMaxRounds = 8;     // (16: -0.2 %, 32: +0.7 %, 64: +11 % on the 100 k surrogate, profiles/r02zq_pack_rounds.json)
    std::vector<int32_t> pack_of(n_plan_tiles, -1), cand;
    // a pack never mixes T2 layers, nor boundary with interior tiles
    auto cls = [&](int32_t ci) { return tl == 2 ? layer_of(P, LT.tile_ids[ci]) : (tile_is_b.empty() ? 0 : (int)tile_is_b[(size_t)ci]); };
    auto size_of = [&](int32_t ci) { return G.tiles[LT.tile_ids[ci]].n_local; };
    auto runs_of = [&](int32_t ci) { return LT.run_begin[ci + 1] - LT.run_begin[ci]; };
    if (enabled)
        for (size_t ci = 0; ci < n_plan_tiles; ++ci)
            if (size_of((int32_t)ci) < capacity && runs_of((int32_t)ci) <= sbk::kInlineRuns &&
                G.tiles[LT.tile_ids[ci]].n_rounds <= kPackMaxRounds) cand.push_back((int32_t)ci);
    std::sort(cand.begin(), cand.end(), [&](int32_t a, int32_t b) {
        if (cls(a) != cls(b)) return cls(a) < cls(b);
        if (size_of(a) != size_of(b)) return size_of(a) > size_of(b);
        return a < b;
    });
    struct Bin { int32_t fill, runs, members; };
    std::vector<Bin> bins;
    std::vector<std::vector<int32_t>> open((size_t)capacity + 1);   // open[r]: bins of the current class with r free slots
    int cur_cls = -1;
    for (int32_t ci : cand) {     // best fit, largest first
        if (cls(ci) != cur_cls) { for (auto &o : open) o.clear(); cur_cls = cls(ci); }
        int32_t chosen = -1;
        for (int r = size_of(ci); r <= capacity && chosen < 0; ++r)
            for (size_t k = open[r].size(); k-- > 0;) {
                const Bin &B = bins[open[r][k]];
                if (B.runs + runs_of(ci) <= sbk::kInlineRuns && B.members < 16) {
                    chosen = open[r][k];
                    open[r].erase(open[r].begin() + (std::ptrdiff_t)k);
                    break;
                }
            }
        if (chosen < 0) { chosen = (int32_t)bins.size(); bins.push_back({0, 0, 0}); }
        Bin &B = bins[chosen];
        B.fill += size_of(ci); B.runs += runs_of(ci); ++B.members;
        open[capacity - B.fill].push_back(chosen);
        pack_of[ci] = chosen;
    }
    std::vector<std::vector<int32_t>> packs;
    std::vector<int32_t> slot_of_bin(bins.size(), -1);
    n_boundary_packs = 0;
    for (size_t ci = 0; ci < n_plan_tiles; ++ci) {
        if (pack_of[ci] < 0) { packs.push_back({(int32_t)ci}); }
        else if (slot_of_bin[pack_of[ci]] < 0) { slot_of_bin[pack_of[ci]] = (int32_t)packs.size(); packs.push_back({(int32_t)ci}); }
        else { packs[slot_of_bin[pack_of[ci]]].push_back((int32_t)ci); continue; }
        if (!tile_is_b.empty() && tile_is_b[ci]) ++n_boundary_packs;
    }
    return packs;
}

std::vector<std::pair<int32_t, int32_t>> t2_layer_ranges(const sbp::Plan &P, const sbp::LocalTiling &LT, const std::vector<std::vector<int32_t>> &packs) {
    std::vector<std::pair<int32_t, int32_t>> ranges(P.t2_layers.size(), {0, 0});
    for (size_t pk = 0; pk < packs.size(); ++pk) {
        auto &rg = ranges[(size_t)layer_of(P, LT.tile_ids[packs[pk][0]])];
        if (rg.second == rg.first) rg.first = (int32_t)pk;
        rg.second = (int32_t)pk + 1;
    }
    return ranges;
}

// Lane-packed slots (kernel_types.hpp kLanePack*): only where every launch of the tiling is known to run 128-lane workgroups -- its
// launches oversubscribe the chip (launch_tile: narrow) -- and the mesh has springs only. A packed tiling forces its width on every
// launch, the boundary / interior pieces of the overlapped schedule included. The 8-byte form for 256-lane workgroups (kWidePack*)
// serves tilings between the 512-lane and the 128-lane regimes: 128^3 on one GPU, a rank's 4 096 tiles of 256^3 on 8. Which TILES
// then qualify is decided tile by tile (build_pack).
int32_t choose_packed_lanes(const TableInput &in, const TableOptions &opt, const sbp::Tiling &G, const sbp::LocalTiling &LT, int tl, int64_t n_packs) {
    bool all_small = true;       // (a tiling with a tile above 512 particles launches the 1 024-particle kernels)
    for (int32_t id : LT.tile_ids) all_small = all_small && G.tiles[id].n_local <= sbk::kSmallTile;
    const bool packable = tl < 2 && all_small && in.n_vol == 0 && in.n_bend == 0 && !(opt.tune_flags & SB_TUNE_NO_PALETTE);
    if (packable && !(opt.tune_flags & SB_TUNE_NO_LANE_PACK) && (opt.tile_lanes == 0 || opt.tile_lanes == sbk::kLanePackLanes) &&
        n_packs >= (int64_t)opt.narrow_min_tiles)
        return sbk::kLanePackLanes;
    if (packable && !(opt.tune_flags & SB_TUNE_NO_WIDE_SLOTS) && (opt.tile_lanes == 0 || opt.tile_lanes == sbk::kWidePackLanes) &&
        n_packs > (int64_t)sbk::kWide8MaxTiles && n_packs < (int64_t)opt.narrow_min_tiles && sbk::kRegRoundsWide >= sbk::kLanePackRounds)
        return sbk::kWidePackLanes;
    return 0;
}

// ---- one pack -----------------------------------------------------------------------------------------------------------------------------

struct TilingEnv {               // what every pack of one tiling is built from; read-only while the host threads run
    const TableInput &in;
    const sbp::Tiling &G;
    const sbp::LocalTiling &LT;
    int tl;
    bool no_palette, emit_items, w_palette;
    int item_waves;
    int32_t packed_lanes;        // of the tiling (choose_packed_lanes)
    const sbp::Tile &tile(int32_t member) const { return G.tiles[LT.tile_ids[member]]; }
};
// Packs are independent: chunks of packs build their pieces of the tables side by side on host threads, the pieces are then
// laid end to end in pack order (place_pieces), exactly as a pack-by-pack loop would fill them.
struct Piece {
    std::vector<sbk::TileDesc> tiles;     // s_begin, run_overflow, gather_begin relative to the piece
    std::vector<int2> overflow;
    std::vector<uint32_t> stream;
    std::vector<int32_t> gather;
    int32_t max_local = 0, max_pal = 0, max_rounds = 0;
    uint32_t max_data = 4;
    int64_t n_packed_tiles = 0;
    bool has_quads = false;
};
struct Part { int32_t member; int32_t cnt[3]; int64_t first_d, first_q; };   // a member's group inside a pack group
struct PackRound { int32_t cnt[3]; std::vector<Part> parts; };                 // constraints per type (distance, volume, bending)
struct PackCounts { int64_t n_dist = 0, n_cons = 0; };

void pad16(std::vector<uint32_t> &stream, size_t s0) { while ((stream.size() - s0) & 3) stream.push_back(0); }

// the pack's run table (inline runs, overflow) or particle list (T2), its members' first tile-local indices (base)
PackCounts pack_descriptor(const TilingEnv &E, const std::vector<int32_t> &members, Piece &Q, sbk::TileDesc &td, std::vector<int32_t> &base) {
    const sbp::LocalTiling &LT = E.LT;
    PackCounts n;
    td.run_overflow = (int32_t)Q.overflow.size();
    base.resize(members.size());
    int32_t lstart = 0, n_runs = 0;
    for (size_t m = 0; m < members.size(); ++m) {
        const int32_t ci = members[m];
        const sbp::Tile &T = E.tile(ci);
        base[m] = lstart;
        if (E.tl == 2) {
            if (m == 0) td.gather_begin = (int32_t)Q.gather.size();
            for (int32_t q = LT.gather_begin[ci]; q < LT.gather_begin[ci + 1]; ++q) Q.gather.push_back(LT.gather[q]);
            lstart += LT.gather_begin[ci + 1] - LT.gather_begin[ci];
        }
        for (int32_t r = LT.run_begin[ci]; r < LT.run_begin[ci + 1]; ++r, ++n_runs) {
            const sbp::Run &rn = LT.runs[r];
            if (n_runs < sbk::kInlineRuns) td.runs[n_runs] = make_int2(rn.start, lstart);
            else Q.overflow.push_back(make_int2(rn.start, lstart));
            lstart += rn.len;
        }
        if (lstart - base[m] != T.n_local) throw std::runtime_error("internal: tile run lengths do not add up");
        n.n_dist += T.d_end - T.d_begin;
        n.n_cons += (T.d_end - T.d_begin) + (T.q_end - T.q_begin);
    }
    td.n_local = lstart;
    td.run_count = n_runs;
    for (int32_t r = n_runs; r < sbk::kInlineRuns; ++r) td.runs[r] = make_int2(0, INT32_MAX);   // never selected
    if (lstart > sbk::kLargeTile) throw std::runtime_error("internal: packed tile too large");
    return n;
}

// the pack's program: group r of the pack = the members' next groups, as many as fit (<= 256 constraints per type)
void zip_rounds(const TilingEnv &E, const std::vector<int32_t> &members, std::vector<PackRound> &prog) {
    prog.clear();
    std::vector<int32_t> next(members.size(), 0);
    std::vector<int64_t> dk(members.size()), qk(members.size());
    for (size_t m = 0; m < members.size(); ++m) { dk[m] = E.tile(members[m]).d_begin; qk[m] = E.tile(members[m]).q_begin; }
    for (;;) {
        PackRound R{{0, 0, 0}, {}};
        for (size_t m = 0; m < members.size(); ++m) {
            const sbp::Tile &T = E.tile(members[m]);
            if (next[m] >= T.n_rounds) continue;
            const sbk::GroupWord gw = sbk::decode_group_word(E.G.rounds[T.round_begin + next[m]]);      // (the plan's round words have the stream's layout)
            const int32_t c[3] = {(int32_t)gw.n_dist, (int32_t)gw.n_vol, (int32_t)gw.n_bend};
            if (R.cnt[0] + c[0] > sbp::kRoundThreads || R.cnt[1] + c[1] > sbp::kRoundThreads || R.cnt[2] + c[2] > sbp::kRoundThreads) continue;
            R.parts.push_back({(int32_t)m, {c[0], c[1], c[2]}, dk[m], qk[m]});
            dk[m] += c[0]; qk[m] += c[1] + c[2];
            for (int t = 0; t < 3; ++t) R.cnt[t] += c[t];
            ++next[m];
        }
        if (R.parts.empty()) break;
        prog.push_back(std::move(R));
    }
    for (size_t m = 0; m < members.size(); ++m)
        if (dk[m] != E.tile(members[m]).d_end || qk[m] != E.tile(members[m]).q_end) throw std::runtime_error("internal: tile stream does not match its rounds");
}

// dictionary-code the rest lengths of the pack's distance constraints when few values repeat: the sorted distinct bit patterns,
// or empty (full slots)
std::vector<uint32_t> rest_dictionary(const TilingEnv &E, const std::vector<int32_t> &members, int64_t n_dist, int32_t n_local) {
    std::vector<uint32_t> vals;
    if (E.no_palette || n_dist <= 0) return vals;
    vals.reserve((size_t)n_dist);
    for (int32_t ci : members) {
        const sbp::Tile &T = E.tile(ci);
        for (int64_t k = T.d_begin; k < T.d_end; ++k) vals.push_back(float_bits(E.in.dist_rest[E.G.t_dist_id[k]]));
    }
    std::sort(vals.begin(), vals.end());
    vals.erase(std::unique(vals.begin(), vals.end()), vals.end());
    if (!((int)vals.size() <= sbk::kMaxPalette && n_local <= sbk::kCompactMaxLocal)) vals.clear();
    return vals;
}
uint32_t palette_index(const std::vector<uint32_t> &pal, uint32_t rest_bits) { return (uint32_t)(std::lower_bound(pal.begin(), pal.end(), rest_bits) - pal.begin()); }

// Wave items (kernel_types.hpp kItem*): the work of every group dealt to the waves of a tile, one dword per wave and step.
// Slots of a group: its hinges (4 per wave slot: a hinge takes a row of 16 lanes, tile_kernel.hip.hpp project_bending_row), its
// tets (16), its springs (64); rows of item_waves slots, dealt boustrophedon (the wave that took a hinge slot in one row takes the
// cheapest of the next). Appended to the tile's header unless an offset does not fit its 21 bits.
void emit_wave_items(const TilingEnv &E, const std::vector<PackRound> &prog, bool compact, size_t s0, sbk::TileDesc &td, std::vector<uint32_t> &stream) {
    const int item_waves = E.item_waves;
    std::vector<uint32_t> it[8];
    uint32_t off = 0;                       // dwords from the start of the tile's data
    bool fits = true;
    for (const PackRound &R : prog) {
        const uint32_t nd = (uint32_t)R.cnt[0], nv = (uint32_t)R.cnt[1], nb = (uint32_t)R.cnt[2];
        const uint32_t dsize = sbk::group_data_dwords(nd, compact), qoff = off + dsize;
        const int n_wb = (int)((nb + 3) >> 2), n_wv = (int)((nv + 15) >> 4), n_wd = (int)((nd + 63) >> 6);
        const int n_slots = n_wb + n_wv + n_wd, rows = std::max(1, (n_slots + item_waves - 1) / item_waves);
        for (int row = 0; row < rows; ++row)
            for (int wave = 0; wave < item_waves; ++wave) {
                const int sw = row * item_waves + ((row & 1) ? item_waves - 1 - wave : wave);
                uint32_t type = sbk::kItemIdle, cnt = 0, o = 0;
                if (sw < n_wb) { type = sbk::kItemBending; cnt = std::min(4u, nb - 4u * (uint32_t)sw); o = qoff + 4u * (nv + 4u * (uint32_t)sw); }
                else if (sw < n_wb + n_wv) { const uint32_t c0 = 16u * (uint32_t)(sw - n_wb); type = sbk::kItemVolume; cnt = std::min(16u, nv - c0); o = qoff + 4u * c0; }
                else if (sw < n_slots) {
                    const uint32_t c0 = 64u * (uint32_t)(sw - n_wb - n_wv);
                    type = compact ? sbk::kItemDistCompact : sbk::kItemDistFull; cnt = std::min(64u, nd - c0); o = off + (compact ? c0 : 2u * c0);
                }
                if (!sbk::item_offset_fits(o)) fits = false;
                it[wave].push_back(sbk::encode_item(type, cnt, row + 1 == rows, o));
            }
        off += sbk::group_dwords(nd, nv + nb, compact);
    }
    if (!fits) return;
    td.n_steps = (int32_t)it[0].size();
    td.s_items = (uint32_t)(stream.size() - s0);
    for (int wave = 0; wave < item_waves; ++wave) stream.insert(stream.end(), it[wave].begin(), it[wave].end());
    pad16(stream, s0);
}

// ---- the three slot encodings -----------------------------------------------------------------------------------------------------------------

struct PackSlots {               // what the emitters read of a pack
    const std::vector<PackRound> &prog;
    const std::vector<int32_t> &base;       // first tile-local index of every member
    const std::vector<uint32_t> &pal;       // empty: full slots
    bool compact() const { return !pal.empty(); }
};
// calls f(round, position in the round, {i | j << 16} tile-local indices, rest-length bits) for every distance slot of the pack
template <class F>
void for_each_distance_slot(const TilingEnv &E, const PackSlots &S, F &&f) {
    for (size_t r = 0; r < S.prog.size(); ++r) {
        int32_t c = 0;
        for (const Part &pt : S.prog[r].parts) {
            const uint32_t b2 = sbk::index_pair_offset((uint32_t)S.base[pt.member]);
            for (int64_t k = pt.first_d; k < pt.first_d + pt.cnt[0]; ++k, ++c) f((int)r, c, E.G.t_dist[k] + b2, float_bits(E.in.dist_rest[E.G.t_dist_id[k]]));
        }
    }
}

// one 16-byte word per lane: six 21-bit fields, field 2 r + u = slot lane + 128 u of round r; full slots keep their rest lengths behind
void emit_lane_packed(const TilingEnv &E, const PackSlots &S, std::vector<uint32_t> &stream) {
    const bool compact = S.compact();
    std::vector<uint32_t> words(compact ? sbk::kLanePackDwordsCompact : sbk::kLanePackDwordsFull, 0u);
    for_each_distance_slot(E, S, [&](int r, int32_t c, uint32_t idx, uint32_t rb) {
        const uint32_t f = pack_field(idx, compact ? palette_index(S.pal, rb) : 0u, "internal: lane-packed slot out of range");
        const int lane = c % sbk::kLanePackLanes, u = c / sbk::kLanePackLanes, fld = 2 * r + u;
        sbk::set_lane_word_field(&words[(size_t)sbk::kLaneWordDwords * (size_t)lane], fld, f);
        // the slot's rest length: fields 0..3 in the second 16-byte sweep, 4 and 5 in the 8-byte one
        if (!compact) words[sbk::lane_pack_rest_dword((uint32_t)lane, (uint32_t)fld)] = rb;
    });
    stream.insert(stream.end(), words.begin(), words.end());
}

// one 8-byte word per lane: three 21-bit fields, field r = slot `lane` of round r
void emit_wide_packed(const TilingEnv &E, const PackSlots &S, std::vector<uint32_t> &stream) {
    std::vector<uint32_t> words(sbk::kWidePackDwords, 0u);
    for_each_distance_slot(E, S, [&](int r, int32_t c, uint32_t idx, uint32_t rb) {
        if (c >= sbk::kWidePackLanes) throw std::runtime_error("internal: wide-packed slot out of range");
        sbk::set_wide_word_field(&words[(size_t)sbk::kWideWordDwords * (size_t)c], r, pack_field(idx, palette_index(S.pal, rb), "internal: wide-packed slot out of range"));
    });
    stream.insert(stream.end(), words.begin(), words.end());
}

// a group's data: its distance slots (4 bytes dictionary-coded, else 8; padded to 4 dwords), then its volume slots, then its bending slots
void emit_slots(const TilingEnv &E, const PackSlots &S, size_t s0, std::vector<uint32_t> &stream, bool &has_quads) {
    const sbp::Tiling &G = E.G;
    for (const PackRound &R : S.prog) {
        for (const Part &pt : R.parts) {
            const uint32_t b2 = sbk::index_pair_offset((uint32_t)S.base[pt.member]);
            for (int64_t k = pt.first_d; k < pt.first_d + pt.cnt[0]; ++k) {
                const uint32_t idx = G.t_dist[k] + b2, rb = float_bits(E.in.dist_rest[G.t_dist_id[k]]);
                const sbk::IndexPair p = sbk::decode_index_pair(idx);
                if (S.compact()) stream.push_back(sbk::encode_compact_slot(p.i, p.j, palette_index(S.pal, rb)));
                else { stream.push_back(idx); stream.push_back(rb); }
            }
        }
        pad16(stream, s0);
        for (int t = 1; t < 3; ++t)
            for (const Part &pt : R.parts) {
                const uint32_t b2 = sbk::index_pair_offset((uint32_t)S.base[pt.member]);
                const int64_t kb = pt.first_q + (t == 2 ? pt.cnt[1] : 0);      // a member's group lists its tets, then its hinges
                for (int64_t k = kb; k < kb + pt.cnt[t]; ++k) {
                    if (G.t_quad_type[k] != t) throw std::runtime_error("internal: group layout");
                    has_quads = true;
                    stream.push_back(G.t_quad[2 * k] + b2); stream.push_back(G.t_quad[2 * k + 1] + b2);
                    const int32_t id = G.t_quad_id[k];
                    if (t == 1) { volatile float r6 = 6.0f * E.in.vol_rest[id]; stream.push_back(float_bits(r6)); stream.push_back(0); }
                    else { stream.push_back(float_bits(E.in.bend_rest[2 * (size_t)id])); stream.push_back(float_bits(E.in.bend_rest[2 * (size_t)id + 1])); }
                }
            }
    }
}

// which packed form a pack takes, if its tiling allows one: 0, kLanePackLanes or kWidePackLanes
uint32_t pack_form(const TilingEnv &E, const PackSlots &S, int32_t n_local, int64_t n_dist) {
    const std::vector<PackRound> &prog = S.prog;
    if (n_local > sbk::kSmallTile || prog.empty() || (int)prog.size() > sbk::kLanePackRounds) return 0;
    for (const PackRound &R : prog) if (R.cnt[1] != 0 || R.cnt[2] != 0) return 0;
    if (E.packed_lanes == sbk::kLanePackLanes && sbk::kLanePackDecodable) {
        // (dictionary-coded tiles with a palette of at most 8; tiles with per-spring rest lengths where the kernels read float inverse
        // masses -- the WPAL = false instantiations carry the loads for that form)
        bool ok = S.compact() ? (int)S.pal.size() <= sbk::kLanePackMaxPalette : (sbk::kRegFullSlots && !E.w_palette && n_dist > 0);
        for (const PackRound &R : prog) ok = ok && R.cnt[0] <= 2 * sbk::kLanePackLanes;
        return ok ? (uint32_t)sbk::kLanePackLanes : 0u;
    }
    if (E.packed_lanes == sbk::kWidePackLanes && S.compact() && (int)S.pal.size() <= sbk::kLanePackMaxPalette) {
        // (the packed form is 2 KiB whatever the tile holds: only where that is LESS than 4 bytes per slot -- full-size tiles, not rim packs)
        uint32_t unpacked = 0;
        for (const PackRound &R : prog) { if (R.cnt[0] > sbk::kWidePackLanes) return 0; unpacked += sbk::group_data_dwords((uint32_t)R.cnt[0], true); }
        return unpacked > sbk::kWidePackDwords ? (uint32_t)sbk::kWidePackLanes : 0u;
    }
    return 0;
}

// one pack: descriptor and stream [group words][dictionary][wave items] [slots], appended to the piece
void build_pack(const TilingEnv &E, const std::vector<int32_t> &members, Piece &Q, std::vector<PackRound> &prog, std::vector<int32_t> &base) {
    std::vector<uint32_t> &stream = Q.stream;
    sbk::TileDesc td{};
    const PackCounts n = pack_descriptor(E, members, Q, td, base);
    Q.max_local = std::max(Q.max_local, td.n_local);
    zip_rounds(E, members, prog);
    td.n_rounds = (int32_t)prog.size();
    if (stream.size() > 0xfffffff0ull - 4ull * (size_t)n.n_cons - 48ull * prog.size() - 1024ull)      // (group word + up to 40 wave items per group)
        throw std::runtime_error("tile constraint stream exceeds 2^32 dwords");
    td.s_begin = (uint32_t)stream.size();
    const size_t s0 = stream.size();
    const std::vector<uint32_t> pal = rest_dictionary(E, members, n.n_dist, td.n_local);
    const bool compact = !pal.empty();
    for (const PackRound &R : prog) stream.push_back(sbk::encode_group_word((uint32_t)R.cnt[0], (uint32_t)R.cnt[1], (uint32_t)R.cnt[2], compact));
    pad16(stream, s0);
    if (stream.size() == s0) stream.insert(stream.end(), 4, 0u);   // empty program: keep 16 readable bytes
    td.n_pal = (int32_t)pal.size();
    stream.insert(stream.end(), pal.begin(), pal.end());
    pad16(stream, s0);
    Q.max_pal = std::max(Q.max_pal, td.n_pal);
    Q.max_rounds = std::max(Q.max_rounds, td.n_rounds);
    if (E.emit_items && !prog.empty()) emit_wave_items(E, prog, compact, s0, td, stream);
    td.s_hdr = (uint32_t)(stream.size() - s0);
    const PackSlots S{prog, base, pal};
    td.packed_lanes = pack_form(E, S, td.n_local, n.n_dist);
    if (td.packed_lanes == (uint32_t)sbk::kLanePackLanes) emit_lane_packed(E, S, stream);
    else if (td.packed_lanes == (uint32_t)sbk::kWidePackLanes) emit_wide_packed(E, S, stream);
    else emit_slots(E, S, s0, stream, Q.has_quads);
    td.s_len = (uint32_t)(stream.size() - s0);
    if (td.packed_lanes) ++Q.n_packed_tiles;
    else Q.max_data = std::max(Q.max_data, td.s_len - td.s_hdr);     // (lane-packed tiles never use the LDS window)
    Q.tiles.push_back(td);
}

// ---- the whole tiling -------------------------------------------------------------------------------------------------------------------------

struct PieceMaxima { int32_t max_local = 0, max_pal = 0, max_rounds = 0; uint32_t max_data = 4; };

// place the pieces: stream / overflow / gather offsets of a descriptor are relative to its piece until now
PieceMaxima place_pieces(std::vector<Piece> &pieces, HostTiling &D) {
    PieceMaxima M;
    size_t nt = 0, no = 0, ns = 0, ng = 0;
    for (const Piece &Q : pieces) { nt += Q.tiles.size(); no += Q.overflow.size(); ns += Q.stream.size(); ng += Q.gather.size(); }
    if (ns > 0xfffffff0ull) throw std::runtime_error("tile constraint stream exceeds 2^32 dwords");
    D.tiles.clear(); D.runs_overflow.clear(); D.stream.clear(); D.gather.clear();
    D.tiles.reserve(nt); D.runs_overflow.reserve(no); D.stream.reserve(ns); D.gather.reserve(ng);
    D.has_quads = false; D.n_packed_tiles = 0;
    for (Piece &Q : pieces) {
        for (sbk::TileDesc td : Q.tiles) {
            td.s_begin += (uint32_t)D.stream.size();
            td.run_overflow += (int32_t)D.runs_overflow.size();
            td.gather_begin += (int32_t)D.gather.size();
            D.tiles.push_back(td);
        }
        D.runs_overflow.insert(D.runs_overflow.end(), Q.overflow.begin(), Q.overflow.end());
        D.stream.insert(D.stream.end(), Q.stream.begin(), Q.stream.end());
        D.gather.insert(D.gather.end(), Q.gather.begin(), Q.gather.end());
        M.max_local = std::max(M.max_local, Q.max_local); M.max_pal = std::max(M.max_pal, Q.max_pal);
        M.max_rounds = std::max(M.max_rounds, Q.max_rounds); M.max_data = std::max(M.max_data, Q.max_data);
        D.has_quads |= Q.has_quads;
        D.n_packed_tiles += Q.n_packed_tiles;
        std::vector<sbk::TileDesc>().swap(Q.tiles); std::vector<uint32_t>().swap(Q.stream);
    }
    return M;
}

// Content-addressed programs. A tile's program (round words, palette, wave items, slots) is written in tile-local numbering, so
// tiles of the same shape run byte-identical programs: every interior tile of a lattice, and the face, edge and corner tiles of
// each kind. Keep ONE copy of each distinct program and point every descriptor that uses it at that copy; the descriptors keep
// their own s_hdr, s_len, n_rounds, n_pal and wave items, and the kernels and the validator reach a program only through
// s_begin. Programs used by more than one tile go first: the few KiB a launch then reads over and over stay in the L2 of every
// XCD, and a launch reads from HBM little more than the particle state. Only with every piece placed in one stream can
// programs built by different host threads be compared. Returns the number of programs kept.
int64_t share_programs(std::vector<sbk::TileDesc> &tiles, std::vector<uint32_t> &stream) {
    const size_t nt = tiles.size();
    std::vector<uint64_t> key(nt);
    sbp::parallel_for_chunks((int64_t)nt, 1024, [&](int64_t, int64_t tb, int64_t te) {
        for (int64_t t = tb; t < te; ++t) {     // FNV-1a over the header fields and the program's dwords
            const sbk::TileDesc &td = tiles[(size_t)t];
            if (td.s_len & 3u) throw std::runtime_error("internal: tile stream not 16-byte aligned");
            uint64_t h = fnv1a(fnv1a(kFnvBasis, td.s_hdr), td.s_len);
            const uint32_t *w = stream.data() + td.s_begin;
            for (uint32_t k = 0; k < td.s_len; ++k) h = fnv1a(h, w[k]);
            key[(size_t)t] = h;
        }
    });
    std::vector<int32_t> by_key(nt);
    for (size_t t = 0; t < nt; ++t) by_key[t] = (int32_t)t;
    std::sort(by_key.begin(), by_key.end(), [&](int32_t a, int32_t b) { return key[(size_t)a] != key[(size_t)b] ? key[(size_t)a] < key[(size_t)b] : a < b; });
    auto same = [&](int32_t a, int32_t b) {      // the hash only proposes: the bytes decide
        const sbk::TileDesc &x = tiles[(size_t)a], &y = tiles[(size_t)b];
        return x.s_hdr == y.s_hdr && x.s_len == y.s_len &&
               std::memcmp(stream.data() + x.s_begin, stream.data() + y.s_begin, (size_t)x.s_len * 4) == 0;
    };
    std::vector<int32_t> rep(nt), uses(nt, 0);      // rep[t] = the first tile (in tile order) with t's program
    std::vector<int32_t> reps;
    for (size_t g0 = 0, g1; g0 < nt; g0 = g1) {
        for (g1 = g0 + 1; g1 < nt && key[(size_t)by_key[g1]] == key[(size_t)by_key[g0]]; ++g1) {}
        reps.clear();                               // distinct programs of this hash value (one, unless the hash collides)
        for (size_t q = g0; q < g1; ++q) {
            const int32_t t = by_key[q];
            int32_t r = t;
            for (int32_t c : reps) if (same(c, t)) { r = c; break; }
            if (r == t) reps.push_back(t);
            rep[(size_t)t] = r; ++uses[(size_t)r];
        }
    }
    std::vector<uint32_t> shared;
    std::vector<uint32_t> at(nt, 0u);
    int64_t n_programs = 0;
    for (int pass = 0; pass < 2; ++pass)            // the shared programs first, then the tiles' own, each in tile order
        for (size_t t = 0; t < nt; ++t)
            if (rep[t] == (int32_t)t && (uses[t] > 1) == (pass == 0)) {
                at[t] = (uint32_t)shared.size();
                const uint32_t *w = stream.data() + tiles[t].s_begin;
                shared.insert(shared.end(), w, w + tiles[t].s_len);
                ++n_programs;
            }
    for (size_t t = 0; t < nt; ++t) tiles[t].s_begin = at[(size_t)rep[t]];
    stream.swap(shared);
    return n_programs;
}

// a tile's cost: steps its longest wave runs, from its group words
int32_t tile_cost(const sbk::TileDesc &td, const std::vector<uint32_t> &stream, bool has_quads, int32_t item_waves) {
    int32_t c = 0;
    for (int32_t r = 0; r < td.n_rounds; ++r) {
        const sbk::GroupWord g = sbk::decode_group_word(stream[(size_t)td.s_begin + (size_t)r]);
        const int32_t nd = (int32_t)g.n_dist, nv = (int32_t)g.n_vol, nb = (int32_t)g.n_bend;
        if (has_quads) {       // rows of wave slots (as dealt for the wave items), a step with a hinge counts double
            const int nw = std::max(1, (int)item_waves ? (int)item_waves : 4);
            c += std::max(1, (((nd + 63) >> 6) + ((nv + 15) >> 4) + ((nb + 3) >> 2) + nw - 1) / nw) + (nb > 0 ? 1 : 0);
        }
        else c += std::max(1, (nd + sbk::kRoundSlots - 1) / sbk::kRoundSlots);
    }
    return c;
}

// Cost order inside a launch (`ranges`: the tile ranges launched on their own). Tiles of one launch share no particle, so their
// order is free; workgroups are dispatched in index order, and a launch of a few hundred tiles puts the first 256 on a compute
// unit each and the rest beside them. On an irregular mesh the launch lasts as long as its longest tile (40+ groups against a
// mean of 29): run the long tiles first, so that none of them starts late or beside another long one. The position of the w-th
// heaviest tile is the one workgroup w reads (xcd_position). Large launches (a lattice: equal tiles, placed for L2 locality)
// and launches of equal tiles are left alone.
void cost_order(const std::vector<std::pair<int32_t, int32_t>> &ranges, HostTiling &D) {
    constexpr int32_t kCostOrderMaxTiles = 2048;
    for (const auto &rg : ranges) {
        const int32_t nr = rg.second - rg.first;
        if (nr < 2 || nr > kCostOrderMaxTiles) continue;
        std::vector<int32_t> cost((size_t)nr), idx((size_t)nr);
        for (int32_t k = 0; k < nr; ++k) { cost[(size_t)k] = tile_cost(D.tiles[(size_t)(rg.first + k)], D.stream, D.has_quads, D.item_waves); idx[(size_t)k] = k; }
        const auto mm = std::minmax_element(cost.begin(), cost.end());
        if ((int64_t)*mm.second * 4 <= (int64_t)*mm.first * 5) continue;       // equal within 25 %
        std::stable_sort(idx.begin(), idx.end(), [&](int32_t a, int32_t b) { return cost[(size_t)a] > cost[(size_t)b]; });
        std::vector<sbk::TileDesc> placed((size_t)nr);
        for (int32_t w = 0; w < nr; ++w) placed[(size_t)xcd_position(w, nr)] = D.tiles[(size_t)(rg.first + idx[(size_t)w])];
        std::copy(placed.begin(), placed.end(), D.tiles.begin() + rg.first);
    }
}

// the tile ranges of a tiling that are launched on their own
std::vector<std::pair<int32_t, int32_t>> launch_ranges(const TableOptions &opt, int tl, const HostTables &H) {
    const HostTiling &D = H.T[tl];
    const int32_t n = (int32_t)D.tiles.size();
    if (tl == 2) return H.t2_layer_range;
    // (only the overlapped schedule launches the boundary and the interior tiles separately -- SB_SCHEDULE_AUTO's calibration runs ticks
    // of BOTH eager schedules on these tables: a whole-tiling launch of the serialised ticks then merely finds its tiles placed for two
    // launches; otherwise a launch of the whole tiling remaps with its own workgroup count, so the placement is made for that launch)
    if (opt.split_launches && D.n_boundary > 0 && D.n_boundary < n) {
        const int32_t cut = tl == 0 ? D.n_boundary : n - D.n_boundary;
        return {{0, cut}, {cut, n}};
    }
    return {{0, n}};
}

void tiling_limits(const TableOptions &opt, const sbp::Tiling &G, const sbp::LocalTiling &LT, const PieceMaxima &M, HostTiling &D) {
    D.n_tiles = (int32_t)D.tiles.size();
    D.max_local = std::max(M.max_local, 1);
    D.win_dwords = (int32_t)std::min<uint32_t>(M.max_data, 8192u);     // <= 32 KiB of LDS; >= one round (4 KiB)
    if (opt.win_dwords_cap > 0) D.win_dwords = std::max(1024, std::min(D.win_dwords, opt.win_dwords_cap) & ~3);   // tuning experiments (sb_tuning.win_dwords)
    D.pal_dwords = (M.max_pal + 3) & ~3;
    D.rounds_dwords = std::min(sbk::kMaxRoundsLds, (M.max_rounds + 3) & ~3);
    D.lds_bytes = (size_t)D.max_local * sizeof(float4) + (size_t)D.rounds_dwords * 4 + (size_t)D.pal_dwords * 4 + (size_t)D.win_dwords * 4 + 16;
    D.n_slots = 0;
    for (int32_t id : LT.tile_ids) D.n_slots += (G.tiles[id].d_end - G.tiles[id].d_begin) + (G.tiles[id].q_end - G.tiles[id].q_begin);
    D.staged_particles = 0;
    for (const sbk::TileDesc &td : D.tiles) D.staged_particles += td.n_local;
}

// ---- halo lists, fused unpack, mailbox ----------------------------------------------------------------------------------------------------

void halo_lists(const sbp::LocalPlan &L, HostTables &H) {
    H.halos.clear();
    H.send_floats = H.recv_floats = 0;
    for (size_t slot = 0; slot < L.halo.size(); ++slot) {
        const sbp::HaloSlot &S = L.halo[slot];
        HostHalo D;
        D.send_off.push_back(0); D.recv_off.push_back(0);
        for (int peer = 0; peer < L.world; ++peer) {
            if (S.send_idx[peer].empty() && S.recv_idx[peer].empty()) continue;
            D.peers.push_back(peer);
            D.send_idx.insert(D.send_idx.end(), S.send_idx[peer].begin(), S.send_idx[peer].end());
            D.recv_idx.insert(D.recv_idx.end(), S.recv_idx[peer].begin(), S.recv_idx[peer].end());
            D.send_off.push_back((int32_t)D.send_idx.size()); D.recv_off.push_back((int32_t)D.recv_idx.size());
        }
        H.send_floats = std::max(H.send_floats, D.send_idx.size() * ghost_floats(slot));
        H.recv_floats = std::max(H.recv_floats, D.recv_idx.size() * ghost_floats(slot));
        H.halos.push_back(std::move(D));
    }
}

// Fused unpack. Ownership is contiguous in the planner's numbering and a rank's ghosts are numbered in that order, so when the
// exchange before the T1 kernels is the plan's ONLY exchange (lattice-type plans: no T2 layers, no global colours) its
// receive buffer -- peers in rank order, each peer's ghosts in its own order -- IS the ghost range [n_owned, n_local) in
// order. The T1 kernels then read ghost k at 6 k floats into the buffer (tile_kernel GHOSTS) and the unpack launch is dropped.
bool fused_unpack_ok(const TableInput &in, const TableOptions &opt, const HostTables &H) {
    const sbp::Plan &P = *in.plan;
    const sbp::LocalPlan &L = *in.local;
    if (!(L.world > 1 && !opt.peer_enabled && P.tiling && P.gcolours.empty() && P.t2_layers.empty() && !H.T[1].has_quads &&
          H.halos.size() > 1 && !(opt.tune_flags & SB_TUNE_NO_FUSED_UNPACK))) return false;
    std::vector<int32_t> ridx;
    for (int peer = 0; peer < L.world; ++peer) ridx.insert(ridx.end(), L.halo[1].recv_idx[(size_t)peer].begin(), L.halo[1].recv_idx[(size_t)peer].end());
    bool identity = (int64_t)ridx.size() == H.n_local - H.n_owned && !ridx.empty();
    for (size_t k = 0; identity && k < ridx.size(); ++k) identity = ridx[k] == (int32_t)(H.n_owned + (int64_t)k);
    return identity;
}

HostMailbox mailbox_layout(const sbp::LocalPlan &L, const TableOptions &opt, const std::vector<HostHalo> &halos) {
    HostMailbox M;
    const int W = L.world;
    if (W > sbk::kMaxPeers + 1) throw std::runtime_error("peer transport: at most 9 ranks");
    M.n_slots = (int)halos.size();
    M.off_table = mailbox_slot_base(M.n_slots, W);
    const size_t hdr_words = M.off_table + (size_t)M.n_slots * W;
    M.data_off_words = (hdr_words + 63) & ~(size_t)63;
    M.header.assign(M.data_off_words, 0u);
    M.header[0] = (uint32_t)opt.plan_hash; M.header[1] = (uint32_t)(opt.plan_hash >> 32);      // compared by the neighbours (peer_link)
    M.header[2] = opt.sharded ? 1u : 0u;
    M.header[3] = opt.plan_shape;                 // compared by the neighbours too: the mailbox LAYOUT follows the number of halo slots
    for (int r = 0; r < W; ++r) { const uint64_t ph = L.pair_hash[(size_t)r]; M.header[4 + 2 * (size_t)r] = (uint32_t)ph; M.header[5 + 2 * (size_t)r] = (uint32_t)(ph >> 32); }
    M.my_off.assign((size_t)M.n_slots, std::vector<uint32_t>((size_t)W, 0u));
    size_t words = M.data_off_words;
    for (int slot = 0; slot < M.n_slots; ++slot) {
        const HostHalo &D = halos[(size_t)slot];
        for (size_t k = 0; k < D.peers.size(); ++k) {          // one 16-byte aligned segment per sending neighbour
            M.my_off[(size_t)slot][(size_t)D.peers[k]] = (uint32_t)words;
            M.header[M.off_table + (size_t)slot * W + (size_t)D.peers[k]] = (uint32_t)words;
            words += 2 * ((ghost_floats((size_t)slot) * (size_t)(D.recv_off[k + 1] - D.recv_off[k]) + 3) & ~(size_t)3);      // two buffers, used alternately
        }
        words = (words + 63) & ~(size_t)63;
    }
    M.bytes = words * 4;
    return M;
}

}  // namespace

// ---- the stages tables.hip uploads one after the other ------------------------------------------------------------------------------------

void build_state(const TableInput &in, const TableOptions &opt, HostTables &H) {
    pack_state(in, H);
    mass_palette(opt, H);
}

// re-base this rank's tiles of tiling tl onto compact arrays
void build_tiling(const TableInput &in, const TableOptions &opt, int tl, HostTables &H) {
    const sbp::Plan &P = *in.plan;
    const sbp::LocalPlan &L = *in.local;
    const sbp::Tiling &G = P.T[tl];
    sbp::LocalTiling LT = L.T[tl];     // copy: T0 and T1 are re-ordered
    HostTiling &D = H.T[tl];
    const std::vector<uint8_t> tile_is_b = boundary_order(L, tl, H.n_owned, H.n_local, LT);
    const std::vector<std::vector<int32_t>> packs = pack_tiles(P, G, LT, tl, tile_is_b, opt.pack_tiles, D.n_boundary);
    if (tl == 2) H.t2_layer_range = t2_layer_ranges(P, LT, packs);
    // meshes with tets / hinges: per-wave step lists beside the group words (springs-only meshes never run the kernels that read them)
    const bool emit_items = (in.n_vol > 0 || in.n_bend > 0) && !(opt.tune_flags & SB_TUNE_NO_WAVE_ITEMS);
    D.item_waves = emit_items ? opt.quad_lanes / 64 : 0;
    D.packed_lanes = choose_packed_lanes(in, opt, G, LT, tl, (int64_t)packs.size());
    const TilingEnv E{in, G, LT, tl, (opt.tune_flags & SB_TUNE_NO_PALETTE) != 0, emit_items, H.w_palette, opt.quad_lanes / 64, D.packed_lanes};
    constexpr int64_t kPacksPerChunk = 128;
    std::vector<Piece> pieces((size_t)(((int64_t)packs.size() + kPacksPerChunk - 1) / kPacksPerChunk));
    sbp::parallel_for_chunks((int64_t)packs.size(), kPacksPerChunk, [&](int64_t chunk, int64_t pk_begin, int64_t pk_end) {
        std::vector<PackRound> prog;
        std::vector<int32_t> base;
        for (int64_t pk = pk_begin; pk < pk_end; ++pk) build_pack(E, packs[(size_t)pk], pieces[(size_t)chunk], prog, base);
    });
    const PieceMaxima M = place_pieces(pieces, D);
    // stream_bytes stays what the tiles READ (the sum of s_len x 4: the compulsory-bytes model of sb_stats.launch_bytes); what is
    // uploaded is stream.size()
    D.stream_bytes = (int64_t)D.stream.size() * 4;
    D.n_programs = (int64_t)D.tiles.size();
    if (!(opt.tune_flags & SB_TUNE_NO_SHARED_PROGRAMS) && D.tiles.size() > 1) D.n_programs = share_programs(D.tiles, D.stream);
    if (!(opt.tune_flags & SB_TUNE_NO_COST_ORDER)) cost_order(launch_ranges(opt, tl, H), D);
    tiling_limits(opt, G, LT, M, D);
}

void build_gcolours(const TableInput &in, HostTables &H) {
    H.gcolours.clear();
    for (const sbp::LocalGColour &LG : in.local->gcolours) {
        HostGColour D;
        D.type = LG.type; D.count = (int32_t)LG.id.size();
        if (LG.type == 0) {
            D.ij.resize(LG.id.size()); D.rest.resize(LG.id.size());
            for (size_t k = 0; k < LG.id.size(); ++k) { D.ij[k] = make_int2(LG.idx[2 * k], LG.idx[2 * k + 1]); D.rest[k] = in.dist_rest[LG.id[k]]; }
        } else {
            D.quad.resize(LG.id.size()); D.rest2.resize(LG.id.size());
            for (size_t k = 0; k < LG.id.size(); ++k) {
                D.quad[k] = make_int4(LG.idx[4 * k], LG.idx[4 * k + 1], LG.idx[4 * k + 2], LG.idx[4 * k + 3]);
                const int32_t id = LG.id[k];
                if (LG.type == 1) { volatile float r6 = 6.0f * in.vol_rest[id]; D.rest2[k] = make_float2(r6, 0.0f); }
                else D.rest2[k] = make_float2(in.bend_rest[2 * (size_t)id], in.bend_rest[2 * (size_t)id + 1]);
            }
        }
        H.gcolours.push_back(std::move(D));
    }
}

void build_halos(const TableInput &in, const TableOptions &opt, HostTables &H) {
    halo_lists(*in.local, H);
    H.fused_unpack = fused_unpack_ok(in, opt, H);
    H.mailbox = (opt.peer_enabled && in.local->world > 1) ? mailbox_layout(*in.local, opt, H.halos) : HostMailbox();
}

void build_tables(const TableInput &in, const TableOptions &opt, HostTables &H) {
    build_state(in, opt, H);
    for (int tl = 0; tl < 3; ++tl) build_tiling(in, opt, tl, H);
    build_gcolours(in, H);
    build_halos(in, opt, H);
}

}  // namespace sbt
