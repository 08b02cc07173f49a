// stream_codec.hpp — the bit layout of the tile constraint stream, written once: every form's constants, its encoder (the table builder,
// tables_host.cpp) and its decoder (tile_kernel.hip.hpp, validate_kernels.hip.hpp, validate.hip). Plain C++ for g++ and for device code.
//
// No reference counterpart exists (/root/reference/README.md:1 is the whole reference tree).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SB_CODEC_FN __host__ __device__ __forceinline__
#else
#define SB_CODEC_FN inline
#endif

namespace sbk {

// A tile's constraint stream lives at stream[TileDesc::s_begin ...], 16-byte aligned, in dwords:
//   [group words, padded to 4] [rest-length palette, padded to 4] [wave items, padded to 4] | [the groups' data]
// (the bar = TileDesc::s_hdr). A group's constraints share no particle (one barrier per group). Its data: the distance slots -- full,
// or dictionary-coded when a tile's distance constraints use at most kMaxPalette distinct rest lengths (regular meshes), the values
// then stand in the tile's palette -- padded to 4 dwords; then the volume slots, then the bending slots (four-vertex slots).

// ---- group word: distance | volume << 10 | bending << 20 constraint counts (each <= kRoundSlots), bit 30 = dictionary-coded distance slots
constexpr int kGroupCountBits = 10, kGroupCompactBit = 30;
constexpr uint32_t kGroupCountMask = (1u << kGroupCountBits) - 1u;
// (Every form has single-field accessors and a decoder that returns a plain struct built from them. Device code on the hot path uses
// the accessors: a struct decoder is optimised on its own before it is inlined, which reorders the instructions of the tile kernels.)
struct GroupWord { uint32_t n_dist, n_vol, n_bend, compact; };      // (compact: 0 or 1)
SB_CODEC_FN uint32_t encode_group_word(uint32_t n_dist, uint32_t n_vol, uint32_t n_bend, bool compact) {
    return n_dist | (n_vol << kGroupCountBits) | (n_bend << (2 * kGroupCountBits)) | (compact ? 1u << kGroupCompactBit : 0u);
}
SB_CODEC_FN uint32_t group_dist_count(uint32_t w) { return w & kGroupCountMask; }
SB_CODEC_FN uint32_t group_vol_count(uint32_t w) { return (w >> kGroupCountBits) & kGroupCountMask; }
SB_CODEC_FN uint32_t group_bend_count(uint32_t w) { return (w >> (2 * kGroupCountBits)) & kGroupCountMask; }
SB_CODEC_FN uint32_t group_is_compact(uint32_t w) { return (w >> kGroupCompactBit) & 1u; }
SB_CODEC_FN GroupWord decode_group_word(uint32_t w) { return {group_dist_count(w), group_vol_count(w), group_bend_count(w), group_is_compact(w)}; }
// dwords of a group's distance slots, padded to 16 bytes (one dword per dictionary-coded slot, two per full slot), and of the whole group
SB_CODEC_FN uint32_t compact_data_dwords(uint32_t n_dist) { return (n_dist + 3u) & ~3u; }
SB_CODEC_FN uint32_t full_data_dwords(uint32_t n_dist) { return (2u * n_dist + 3u) & ~3u; }
SB_CODEC_FN uint32_t group_data_dwords(uint32_t n_dist, bool compact) { return compact ? compact_data_dwords(n_dist) : full_data_dwords(n_dist); }
SB_CODEC_FN uint32_t group_dwords(uint32_t n_dist, uint32_t n_quads, bool compact) { return group_data_dwords(n_dist, compact) + 4u * n_quads; }

// ---- a pair of tile-local indices {i | j << 16}: the first dword of a full distance slot, each of the first two of a four-vertex slot
constexpr int kPairShift = 16;
constexpr uint32_t kPairMask = 0xffffu;
struct IndexPair { uint32_t i, j; };
SB_CODEC_FN uint32_t encode_index_pair(uint32_t i, uint32_t j) { return i | (j << kPairShift); }
SB_CODEC_FN uint32_t pair_i(uint32_t w) { return w & kPairMask; }
SB_CODEC_FN uint32_t pair_j(uint32_t w) { return w >> kPairShift; }
SB_CODEC_FN IndexPair decode_index_pair(uint32_t w) { return {pair_i(w), pair_j(w)}; }
// the same offset added to both indices of a pair (a pack's members are renumbered by their base)
SB_CODEC_FN uint32_t index_pair_offset(uint32_t base) { return base | (base << kPairShift); }

// ---- full distance slot {i | j << 16, rest length}: 2 dwords; four-vertex slot {i0 | i1 << 16, i2 | i3 << 16, rest.x, rest.y}: 4 dwords
constexpr int kFullSlotDwords = 2, kQuadSlotDwords = 4;
struct QuadIndices { uint32_t i[4]; };
SB_CODEC_FN QuadIndices decode_quad_indices(uint32_t e0, uint32_t e1) { return {{pair_i(e0), pair_j(e0), pair_i(e1), pair_j(e1)}}; }

// ---- dictionary-coded distance slot {i:12 | j:12 | palette:8}: 1 dword
constexpr int kCompactIndexBits = 12, kCompactPaletteShift = 24;
constexpr uint32_t kCompactIndexMask = (1u << kCompactIndexBits) - 1u;
constexpr int kMaxPalette = 1 << (32 - kCompactPaletteShift);     // rest-length dictionary entries per tile
constexpr int kCompactMaxLocal = 1 << kCompactIndexBits;          // tile-local indices the form can hold
struct CompactSlot { uint32_t i, j, pal; };
SB_CODEC_FN uint32_t encode_compact_slot(uint32_t i, uint32_t j, uint32_t pal) { return i | (j << kCompactIndexBits) | (pal << kCompactPaletteShift); }
SB_CODEC_FN uint32_t compact_slot_i(uint32_t e) { return e & kCompactIndexMask; }
SB_CODEC_FN uint32_t compact_slot_j(uint32_t e) { return (e >> kCompactIndexBits) & kCompactIndexMask; }
SB_CODEC_FN uint32_t compact_slot_pal(uint32_t e) { return e >> kCompactPaletteShift; }
SB_CODEC_FN CompactSlot decode_compact_slot(uint32_t e) { return {compact_slot_i(e), compact_slot_j(e), compact_slot_pal(e)}; }
// a full slot's index pair as a dictionary-coded slot without a palette index (tiles of at most kCompactMaxLocal particles)
SB_CODEC_FN uint32_t compact_slot_of_pair(uint32_t pair) { return (pair & kCompactIndexMask) | ((pair >> kPairShift) << kCompactIndexBits); }

// ---- wave items (meshes with tets / hinges, 4-wave tiles). The host deals every group's work to the waves ahead of time -- hinges
// first, then tets (16 four-lane constraints per wave), then springs (64 per wave), boustrophedon over the rows of a group -- and
// stores for every wave one dword per STEP (= one row of one group): what to project, how many, where the slots lie in the tile's
// data, and whether the group ends here (workgroup barrier). The kernel's loop over a list is then a v_readlane, three bit-field
// extracts and one uniform branch per step instead of decoding the group word, the window test and the slot arithmetic (90 scalar
// instructions and a dozen branches per group on the critical path of every group).
// One item = type:3 | count:7 | barrier:1 | dword offset:21 (from the start of the tile's data).
constexpr int kItemWaves = 4;        // dealt for 4-wave tiles (8 with SB_QUAD_LANES=512)
constexpr uint32_t kItemIdle = 0, kItemDistCompact = 1, kItemDistFull = 2, kItemVolume = 3, kItemBending = 4;
constexpr int kItemCountShift = 3, kItemBarrierBit = 10, kItemOffsetShift = 11;
constexpr uint32_t kItemTypeMask = (1u << kItemCountShift) - 1u, kItemCountMask = (1u << (kItemBarrierBit - kItemCountShift)) - 1u;
struct WaveItem { uint32_t type, count, offset, barrier; };      // (barrier: nonzero = the group ends with this step)
SB_CODEC_FN bool item_offset_fits(uint32_t offset) { return offset < (1u << (32 - kItemOffsetShift)); }
SB_CODEC_FN uint32_t encode_item(uint32_t type, uint32_t count, bool barrier, uint32_t offset) {
    return type | (count << kItemCountShift) | (barrier ? 1u << kItemBarrierBit : 0u) | (offset << kItemOffsetShift);
}
SB_CODEC_FN uint32_t item_type(uint32_t it) { return it & kItemTypeMask; }
SB_CODEC_FN uint32_t item_count(uint32_t it) { return (it >> kItemCountShift) & kItemCountMask; }
SB_CODEC_FN uint32_t item_offset(uint32_t it) { return it >> kItemOffsetShift; }
SB_CODEC_FN uint32_t item_barrier(uint32_t it) { return it & (1u << kItemBarrierBit); }
SB_CODEC_FN WaveItem decode_item(uint32_t it) { return {item_type(it), item_count(it), item_offset(it), item_barrier(it)}; }
// dwords of one slot of an item's type
SB_CODEC_FN uint32_t item_slot_dwords(uint32_t type) { return type == kItemDistCompact ? 1u : (type == kItemDistFull ? (uint32_t)kFullSlotDwords : (uint32_t)kQuadSlotDwords); }

// ---- lane-packed slots. A register-resident spring tile run by 128-lane workgroups gives every lane two slots in each of its (at
// most three) rounds and keeps them in registers for both passes; the slots need 9 + 9 bits of tile-local indices and a palette index.
// Stored as ONE 16-byte word per lane -- six 21-bit fields {i:9 | j:9 | palette:3}, field 2 r + u = the lane's slot u of round r
// (constraint lane + 128 u of that round; beyond the round's count the field is 0) -- the tile's data is 2 KiB instead of 3 KiB
// (4 bytes per slot), it arrives in the lane's first window load and never touches LDS. The host decides per tile (tables_host.cpp pack_form).
// A tile whose slots are NOT dictionary-coded (per-spring rest lengths) packs the same way with its rest values behind the index words:
// [128 x 16 B index word][128 x 16 B: rest of fields 0..3][128 x 8 B: rest of fields 4, 5] = 40 bytes per lane instead of 48
// (n_pal == 0 marks this form; only in the kernels that read inverse masses as floats, WPAL = false -- the host packs accordingly).
constexpr int kLanePackLanes = 128, kLanePackRounds = 3, kLanePackFieldBits = 21, kLanePackMaxPalette = 8;
constexpr int kLanePackIndexBits = 9;
constexpr uint32_t kLanePackDwordsCompact = 4 * kLanePackLanes, kLanePackDwordsFull = 10 * kLanePackLanes;
constexpr uint32_t kLanePackFieldMask = (1u << kLanePackFieldBits) - 1u, kLanePackIndexMask = (1u << kLanePackIndexBits) - 1u;
// The same for 256-lane workgroups: a lane has ONE slot per round, so three 21-bit fields = ONE 8-byte word per lane, field r = the
// lane's slot of round r (constraint `lane` of that round) -- again 2 KiB per 512-particle tile instead of 3 KiB, loaded by the lane
// itself with the first batch, never staged in LDS. Dictionary-coded tiles only. For the launches between the 512-lane and the 128-lane
// regimes: mid-size meshes (128^3: 4 096 tiles) and the ranks of a partitioned solver (256^3 on 8 ranks: 4 096 tiles each).
constexpr int kWidePackLanes = 256;
constexpr uint32_t kWidePackDwords = 2 * kWidePackLanes;
constexpr int kLaneWordDwords = 4, kWideWordDwords = 2;

SB_CODEC_FN bool pack_field_fits(uint32_t i, uint32_t j, uint32_t pal) { return i <= kLanePackIndexMask && j <= kLanePackIndexMask && pal < (uint32_t)kLanePackMaxPalette; }
SB_CODEC_FN uint32_t encode_pack_field(uint32_t i, uint32_t j, uint32_t pal) { return i | (j << kLanePackIndexBits) | (pal << (2 * kLanePackIndexBits)); }
SB_CODEC_FN uint32_t pack_field_i(uint32_t f) { return f & kLanePackIndexMask; }
SB_CODEC_FN uint32_t pack_field_j(uint32_t f) { return (f >> kLanePackIndexBits) & kLanePackIndexMask; }
SB_CODEC_FN uint32_t pack_field_pal(uint32_t f) { return f >> (2 * kLanePackIndexBits); }
SB_CODEC_FN CompactSlot decode_pack_field(uint32_t f) { return {pack_field_i(f), pack_field_j(f), pack_field_pal(f)}; }
// a field as the dictionary-coded slot word of the same constraint
SB_CODEC_FN uint32_t compact_slot_of_pack_field(uint32_t f) {
    return (f & kLanePackIndexMask) | (((f >> kLanePackIndexBits) & kLanePackIndexMask) << kCompactIndexBits) | ((f >> (2 * kLanePackIndexBits)) << kCompactPaletteShift);
}
// where field f lies in a lane's word: first dword, shift inside it, and whether it runs on into the next dword
struct FieldPos { uint32_t dword, shift; bool straddles; };
SB_CODEC_FN FieldPos pack_field_pos(uint32_t f) {
    const uint32_t bit = (uint32_t)kLanePackFieldBits * f;
    return {bit >> 5, bit & 31u, (bit & 31u) + (uint32_t)kLanePackFieldBits > 32u};
}
// field f of a lane's word w[0 .. word_dwords) in memory: kLaneWordDwords (fields 0..5) or kWideWordDwords (fields 0..2)
SB_CODEC_FN uint32_t packed_word_field(const uint32_t *w, uint32_t word_dwords, uint32_t f) {
    const FieldPos p = pack_field_pos(f);
    const uint64_t two = (uint64_t)w[p.dword] | ((uint64_t)(p.dword + 1 < word_dwords ? w[p.dword + 1] : 0u) << 32);
    return (uint32_t)(two >> p.shift) & kLanePackFieldMask;
}
SB_CODEC_FN void set_lane_word_field(uint32_t *w, uint32_t f, uint32_t field) {
    const FieldPos p = pack_field_pos(f);
    w[p.dword] |= field << p.shift;
    if (p.straddles) w[p.dword + 1] |= field >> (32u - p.shift);
}
// field r of an 8-byte wide word {lo, hi} held in registers (fields 0..2)
SB_CODEC_FN uint32_t wide_word_field(uint32_t lo, uint32_t hi, uint32_t r) {
    return (uint32_t)(((uint64_t)lo | ((uint64_t)hi << 32)) >> ((uint32_t)kLanePackFieldBits * r)) & kLanePackFieldMask;
}
SB_CODEC_FN void set_wide_word_field(uint32_t *w, uint32_t r, uint32_t field) {
    const uint64_t f = (uint64_t)field << ((uint32_t)kLanePackFieldBits * r);
    w[0] |= (uint32_t)f;
    w[1] |= (uint32_t)(f >> 32);
}
// full form: dword (from the start of the tile's data) of the rest length of field f of `lane`
SB_CODEC_FN uint32_t lane_pack_rest_dword(uint32_t lane, uint32_t f) {
    return f < 4u ? 4u * (uint32_t)kLanePackLanes + 4u * lane + f : 8u * (uint32_t)kLanePackLanes + 2u * lane + (f - 4u);
}

}  // namespace sbk
