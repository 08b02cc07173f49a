// tables_host.hpp — from the planner's output to the tables the kernels read, on the host: particle state, tile descriptors and
// constraint streams, global colours, halo lists, the peer mailbox layout. Pure C++ (compiled with g++ like plan.cpp): no HIP runtime
// call, no solver object. tables.hip uploads what this unit builds; tests/sanitize/tables_digest.cpp pins it on a machine without a GPU.
//
// No reference counterpart exists (/root/reference/README.md:1 is the whole reference tree).
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "kernel_types.hpp"
#include "plan.hpp"

namespace sbt {

static_assert(sizeof(sbk::TileDesc) == 128, "the kernels read 128-byte tile descriptors");

// 64-bit FNV-1a, one word at a time (the plan hash of tables.hip, the program keys of share_programs)
constexpr uint64_t kFnvBasis = 1469598103934665603ull, kFnvPrime = 1099511628211ull;
inline uint64_t fnv1a(uint64_t h, uint64_t word) { return (h ^ word) * kFnvPrime; }

// floats per ghost a halo slot carries: slot 1 (before the T1 kernels) also carries previous positions
inline size_t ghost_floats(size_t slot) { return slot == 1 ? 6 : 3; }

// first header word of a halo slot's flags in a peer mailbox: [4 words][2 per rank: pair hashes][per slot: data flags, ack flags, 3 words]
inline size_t mailbox_slot_base(int slot, int world) { return 4 + 2 * (size_t)world + (size_t)slot * (2 * (size_t)world + 3); }

// The solver fields that shape the tables (sb_solver's names; SB_TUNE_* bits of softbody_debug.h in tune_flags).
struct TableOptions {
    uint32_t tune_flags = 0;
    int tile_lanes = 0, quad_lanes = 512, narrow_min_tiles = 10240;
    bool pack_tiles = true;
    int win_dwords_cap = 0;
    bool split_launches = false;     // the boundary and the interior tiles of T0 / T1 are launched separately (overlapped schedule, or its calibration)
    bool peer_enabled = false, sharded = false;
    uint64_t plan_hash = 0;          // mailbox header words 0-1
    uint32_t plan_shape = 0;         // mailbox header word 3
};

struct TableInput {
    const sbp::Plan *plan;
    const sbp::LocalPlan *local;
    const float *pos, *vel, *invm;                      // caller numbering, as authored
    const float *dist_rest, *vol_rest, *bend_rest;      // per constraint (bending: 2 floats)
    int64_t n_vol, n_bend;                              // four-vertex constraints authored (0: a springs-only mesh)
};

struct TilingScalars {           // what the launches need to know about a tiling beside its four arrays
    int32_t n_tiles = 0;
    size_t lds_bytes = 0;
    int64_t n_slots = 0;         // constraints stored in the tile streams
    int64_t staged_particles = 0;   // sum of n_local over the device tiles
    int64_t stream_bytes = 0;    // bytes of the tile streams (round words, palettes, slots) the tiles read: sum of s_len x 4, shared programs counted per tile
    int64_t n_programs = 0;      // distinct programs held in `stream` (tiles with identical programs share one copy; stream.count x 4 = bytes uploaded)
    int32_t max_local = 0, win_dwords = 4, pal_dwords = 0, rounds_dwords = 0;
    int32_t n_boundary = 0;      // world > 1: T0 -- the FIRST n_boundary tiles hold every particle some peer needs; T1 -- the LAST
                                 // n_boundary tiles hold every ghost and every sent particle
    bool has_quads = false;
    int32_t item_waves = 0;      // waves per tile the wave items were dealt for (0 = the streams hold none)
    int32_t packed_lanes = 0;    // 128: tiles of this tiling may hold lane-packed slots (kernel_types.hpp kLanePack*): EVERY launch of it runs 128-lane workgroups
    int64_t n_packed_tiles = 0;
};

struct HostTiling : TilingScalars {
    std::vector<sbk::TileDesc> tiles;
    std::vector<int2> runs_overflow;
    std::vector<uint32_t> stream;     // per tile: [round words][rest-length dictionary][round data], see kernel_types.hpp
    std::vector<int32_t> gather;      // T2: particle lists of the tiles (local numbering)
    void release_arrays() {          // frees the storage, keeps the scalars
        std::vector<sbk::TileDesc>().swap(tiles); std::vector<int2>().swap(runs_overflow); std::vector<uint32_t>().swap(stream); std::vector<int32_t>().swap(gather);
    }
};

struct HostGColour {
    int type = 0;
    int32_t count = 0;
    std::vector<int2> ij;             // type 0
    std::vector<float> rest;
    std::vector<int4> quad;           // types 1, 2
    std::vector<float2> rest2;
};

struct HostHalo {                // one halo slot: who we talk to and which particles travel
    std::vector<int> peers;
    std::vector<int32_t> send_off, recv_off;      // per peer (+1), in particles
    std::vector<int32_t> send_idx, recv_idx;
};

struct HostMailbox {             // header words, then one segment per (halo slot, sending rank) in slot order, ranks increasing
    int n_slots = 0;
    size_t off_table = 0, data_off_words = 0, bytes = 0;
    std::vector<uint32_t> header;                 // data_off_words of them
    std::vector<std::vector<uint32_t>> my_off;    // [slot][rank]: first word of rank's segment
};

struct HostTables {
    int64_t n_owned = 0, n_local = 0;
    std::vector<float> pos3, vel, wf;             // device numbering: packed xyz, packed xyz, inverse mass
    std::vector<uint8_t> w8;                      // palette index of the inverse mass (w_palette)
    std::vector<float> wpal;                      // kMaxMassPalette entries
    bool w_palette = false, w_uniform = false;
    HostTiling T[3];
    std::vector<std::pair<int32_t, int32_t>> t2_layer_range;   // device-tile ranges of T[2], one per T2 layer
    std::vector<HostGColour> gcolours;
    std::vector<HostHalo> halos;                  // indexed by halo slot
    size_t send_floats = 0, recv_floats = 0;      // the largest slot's buffers
    bool fused_unpack = false;
    HostMailbox mailbox;                          // peer_enabled and world > 1 only
};

// The stages, in the order build_device uploads them (each reads what the earlier ones left in H). A caller may release a
// stage's vectors once it has uploaded them: later stages read only scalars of earlier ones (and the halos' offsets).
void build_state(const TableInput &in, const TableOptions &opt, HostTables &H);
void build_tiling(const TableInput &in, const TableOptions &opt, int tl, HostTables &H);
void build_gcolours(const TableInput &in, HostTables &H);
void build_halos(const TableInput &in, const TableOptions &opt, HostTables &H);       // + buffer sizes, fused unpack, mailbox layout
void build_tables(const TableInput &in, const TableOptions &opt, HostTables &H);      // all of the above

}  // namespace sbt
