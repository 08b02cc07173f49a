// stream_codec_check.cpp — csrc/stream_codec.hpp on a machine without a GPU (tests/test_stream_codec.py).
//
// For every form of the tile constraint stream, at the corners of its fields:
//   (a) decode(encode(x)) == x, through the struct decoder and through the single-field accessors;
//   (b) the encoder gives the word the table builder wrote before the codec existed, and the decoder reads what the kernels read: the
//       expressions of csrc/tables_host.cpp, csrc/tile_kernel.hip.hpp and csrc/validate_kernels.hip.hpp at commit d969b55, transcribed
//       here as parent_* -- the reference; it is not derived from the new header.
// Prints "points N"; any violation is reported on stderr and makes the exit status 1.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "stream_codec.hpp"

namespace {

long points = 0, bad = 0;
void check(bool ok, const char *what, uint32_t a = 0, uint32_t b = 0, uint32_t c = 0, uint32_t d = 0) {
    if (!ok) { ++bad; std::fprintf(stderr, "%s: %u %u %u %u\n", what, a, b, c, d); }
}

// ---- the parent's expressions ------------------------------------------------------------------------------------------------------------
uint32_t parent_group_word(uint32_t nd, uint32_t nv, uint32_t nb, bool compact) { return nd | (nv << 10) | (nb << 20) | (compact ? 1u << 30 : 0u); }
uint32_t parent_group_data_dwords(uint32_t n_dist, bool compact) { return compact ? ((n_dist + 3u) & ~3u) : ((2u * n_dist + 3u) & ~3u); }
uint32_t parent_compact_slot(uint32_t idx, uint32_t pal) { return (idx & 0xffffu) | ((idx >> 16) << 12) | (pal << 24); }
uint32_t parent_item(uint32_t type, uint32_t cnt, bool last_row, uint32_t o) { return type | (cnt << 3) | (last_row ? 1u << 10 : 0u) | (o << 11); }
uint64_t parent_slot_field(uint32_t idx, uint32_t pal_index, bool &fits) {
    const uint32_t i = idx & 0xffffu, j = idx >> 16;
    fits = !(i > 511u || j > 511u || pal_index > 7u);
    return (uint64_t)(i | (j << 9) | (pal_index << 18));
}
void parent_put_lane_field(uint32_t *wd, int fld, uint64_t f) {
    const int bit = 21 * fld, w0 = bit >> 5, sh = bit & 31;
    wd[w0] |= (uint32_t)(f << sh);
    if (sh + 21 > 32) wd[w0 + 1] |= (uint32_t)(f >> (32 - sh));
}
uint32_t parent_get_lane_field(const uint32_t *wv, int fld) {      // tile_kernel's decode
    const int bit = 21 * fld, w0 = bit >> 5, sh = bit & 31;
    const uint32_t lo = wv[w0] >> sh;
    const uint32_t hi = (sh + 21 > 32) ? (wv[w0 + 1 < 4 ? w0 + 1 : 3] << ((32 - sh) & 31)) : 0u;
    return (lo | hi) & ((1u << 21) - 1u);
}
uint32_t parent_get_lane_field_validator(const uint32_t *wd, uint32_t fld, uint32_t lane_dwords) {      // validate_tiles_kernel's decode, both widths
    const uint32_t bit = 21u * fld, w0 = bit >> 5, sh = bit & 31u;
    const uint64_t two = (uint64_t)wd[w0] | ((uint64_t)(w0 + 1 < lane_dwords ? wd[w0 + 1] : 0u) << 32);
    return (uint32_t)(two >> sh) & ((1u << 21) - 1u);
}
void parent_put_wide_field(uint32_t *wd, int r, uint64_t field) {
    const uint64_t f = field << (21 * r);
    wd[0] |= (uint32_t)f;
    wd[1] |= (uint32_t)(f >> 32);
}
uint32_t parent_get_wide_field(uint32_t x, uint32_t y, int r) {
    const uint64_t two = (uint64_t)x | ((uint64_t)y << 32);
    return (uint32_t)(two >> (21 * r)) & ((1u << 21) - 1u);
}
uint32_t parent_field_as_slot(uint32_t f) { return (f & 511u) | (((f >> 9) & 511u) << 12) | ((f >> 18) << 24); }
uint32_t parent_rest_dword(uint32_t lane, uint32_t fld) { return fld < 4 ? 4u * 128u + 4u * lane + fld : 8u * 128u + 2u * lane + (fld - 4u); }

}  // namespace

int main() {
    using namespace sbk;
    const uint32_t counts[4] = {0, 1, 256, 1023}, locals[4] = {0, 511, 4095, 65535}, pals[3] = {0, 7, 255};

    // group word
    for (uint32_t nd : counts) for (uint32_t nv : counts) for (uint32_t nb : counts) for (int compact = 0; compact < 2; ++compact) {
        ++points;
        const uint32_t w = encode_group_word(nd, nv, nb, compact != 0);
        const GroupWord g = decode_group_word(w);
        check(w == parent_group_word(nd, nv, nb, compact != 0), "group word differs from the parent's", nd, nv, nb, (uint32_t)compact);
        check(g.n_dist == nd && g.n_vol == nv && g.n_bend == nb && g.compact == (uint32_t)compact, "group word round trip", nd, nv, nb, (uint32_t)compact);
        check(group_dist_count(w) == (w & 1023u) && group_vol_count(w) == ((w >> 10) & 1023u) && group_bend_count(w) == ((w >> 20) & 1023u) &&
              group_is_compact(w) == ((w >> 30) & 1u), "group word accessors", w);
        check(group_data_dwords(nd, compact != 0) == parent_group_data_dwords(nd, compact != 0) &&
              (compact ? compact_data_dwords(nd) : full_data_dwords(nd)) == parent_group_data_dwords(nd, compact != 0) &&
              group_dwords(nd, nv + nb, compact != 0) == parent_group_data_dwords(nd, compact != 0) + 4u * (nv + nb), "group data dwords", nd, nv, nb, (uint32_t)compact);
    }
    // dictionary-coded distance slot: 12-bit indices, 8-bit palette index
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) for (uint32_t pal : pals) {
        ++points;
        const uint32_t i = locals[a], j = locals[b], e = encode_compact_slot(i, j, pal);
        const CompactSlot s = decode_compact_slot(e);
        check(e == parent_compact_slot(i | (j << 16), pal), "compact slot differs from the parent's", i, j, pal);
        check(s.i == i && s.j == j && s.pal == pal, "compact slot round trip", i, j, pal);
        check(compact_slot_i(e) == (e & 0xfffu) && compact_slot_j(e) == ((e >> 12) & 0xfffu) && compact_slot_pal(e) == (e >> 24), "compact slot accessors", e);
    }
    // index pair = first dword of a full distance slot
    for (uint32_t i : locals) for (uint32_t j : locals) {
        ++points;
        const uint32_t e = encode_index_pair(i, j);
        const IndexPair p = decode_index_pair(e);
        check(e == (i | (j << 16)), "index pair differs from the parent's", i, j);
        check(p.i == i && p.j == j && pair_i(e) == (e & 0xffffu) && pair_j(e) == (e >> 16), "index pair round trip", i, j);
        check(compact_slot_of_pair(e) == ((e & 0xfffu) | ((e >> 16) << 12)), "full slot as compact slot", i, j);
        check(e + index_pair_offset(5) == ((i + 5) | ((j + 5) << 16)) || i == 65535 || j == 65535, "index pair offset", i, j);
    }
    // four-vertex slot
    for (uint32_t i0 : locals) for (uint32_t i1 : locals) for (uint32_t i2 : locals) for (uint32_t i3 : locals) {
        ++points;
        const uint32_t e0 = encode_index_pair(i0, i1), e1 = encode_index_pair(i2, i3);
        const QuadIndices q = decode_quad_indices(e0, e1);
        check(q.i[0] == i0 && q.i[1] == i1 && q.i[2] == i2 && q.i[3] == i3, "quad slot round trip", i0, i1, i2, i3);
        check(q.i[0] == (e0 & 0xffffu) && q.i[1] == (e0 >> 16) && q.i[2] == (e1 & 0xffffu) && q.i[3] == (e1 >> 16), "quad slot differs from the parent's decode", e0, e1);
    }
    // wave item
    for (uint32_t type = 0; type < 5; ++type) for (uint32_t cnt : {0u, 1u, 64u, 127u}) for (int barrier = 0; barrier < 2; ++barrier)
    for (uint32_t o : {0u, (1u << 21) - 1u}) {
        ++points;
        const uint32_t it = encode_item(type, cnt, barrier != 0, o);
        const WaveItem d = decode_item(it);
        check(item_offset_fits(o) && it == parent_item(type, cnt, barrier != 0, o), "wave item differs from the parent's", type, cnt, (uint32_t)barrier, o);
        check(d.type == type && d.count == cnt && (d.barrier != 0) == (barrier != 0) && d.offset == o, "wave item round trip", type, cnt, (uint32_t)barrier, o);
        check(item_type(it) == (it & 7u) && item_count(it) == ((it >> 3) & 127u) && item_offset(it) == (it >> 11) && item_barrier(it) == (it & (1u << 10)), "wave item accessors", it);
    }
    ++points;
    check(!item_offset_fits(1u << 21) && ((1u << 21) >= (1u << (32 - 11))) && item_offset_fits((1u << 21) - 1u), "item offset 2^21 must not fit");
    check(item_slot_dwords(kItemDistCompact) == 1 && item_slot_dwords(kItemDistFull) == 2 && item_slot_dwords(kItemVolume) == 4 && item_slot_dwords(kItemBending) == 4, "item slot dwords");
    // 21-bit lane-pack field
    for (uint32_t i : {0u, 511u}) for (uint32_t j : {0u, 511u}) for (uint32_t pal : {0u, 7u}) {
        ++points;
        bool fits;
        const uint64_t want = parent_slot_field(i | (j << 16), pal, fits);
        const uint32_t f = encode_pack_field(i, j, pal);
        const CompactSlot d = decode_pack_field(f);
        check(fits && pack_field_fits(i, j, pal) && (uint64_t)f == want, "pack field differs from the parent's", i, j, pal);
        check(d.i == i && d.j == j && d.pal == pal && pack_field_i(f) == (f & 511u) && pack_field_j(f) == ((f >> 9) & 511u) && pack_field_pal(f) == (f >> 18), "pack field round trip", i, j, pal);
        check(compact_slot_of_pack_field(f) == parent_field_as_slot(f) && compact_slot_of_pack_field(f) == encode_compact_slot(i, j, pal), "pack field as compact slot", i, j, pal);
    }
    for (int k = 0; k < 3; ++k) {      // range check: one field past its width
        ++points;
        const uint32_t i = k == 0 ? 512u : 0u, j = k == 1 ? 512u : 0u, pal = k == 2 ? 8u : 0u;
        bool fits;
        parent_slot_field(i | (j << 16), pal, fits);
        check(!fits && !pack_field_fits(i, j, pal), "pack field range check", i, j, pal);
    }
    // 16-byte lane word: six fields, three of them across a dword boundary
    const uint32_t field_values[2] = {encode_pack_field(511, 511, 7), encode_pack_field(0x155, 0x0aa, 5)};
    for (uint32_t f = 0; f < 6; ++f) for (uint32_t v : field_values) {
        ++points;
        uint32_t w[4] = {0, 0, 0, 0}, pw[4] = {0, 0, 0, 0};
        set_lane_word_field(w, f, v);
        parent_put_lane_field(pw, (int)f, v);
        const FieldPos p = pack_field_pos(f);
        check(w[0] == pw[0] && w[1] == pw[1] && w[2] == pw[2] && w[3] == pw[3], "lane word differs from the parent's", f, v);
        check(p.dword == (21u * f) >> 5 && p.shift == ((21u * f) & 31u) && p.straddles == (f == 1 || f == 3 || f == 4) &&
              p.straddles == (21u * f == 21u || 21u * f == 63u || 21u * f == 84u), "field position", f);
        for (uint32_t o = 0; o < 6; ++o) {
            const uint32_t want = o == f ? v : 0u;
            check(packed_word_field(w, 4, o) == want && parent_get_lane_field(w, (int)o) == want && parent_get_lane_field_validator(w, o, 4) == want, "lane word round trip", f, o, v);
        }
    }
    {
        ++points;
        uint32_t w[4] = {0, 0, 0, 0}, pw[4] = {0, 0, 0, 0};
        for (uint32_t f = 0; f < 6; ++f) { set_lane_word_field(w, f, encode_pack_field(100 + f, 200 + f, f)); parent_put_lane_field(pw, (int)f, encode_pack_field(100 + f, 200 + f, f)); }
        check(w[0] == pw[0] && w[1] == pw[1] && w[2] == pw[2] && w[3] == pw[3], "full lane word differs from the parent's");
        for (uint32_t f = 0; f < 6; ++f) {
            const CompactSlot d = decode_pack_field(packed_word_field(w, 4, f));
            check(d.i == 100 + f && d.j == 200 + f && d.pal == f && packed_word_field(w, 4, f) == parent_get_lane_field(w, (int)f), "full lane word round trip", f);
        }
    }
    // 8-byte wide word: three fields
    for (uint32_t r = 0; r < 3; ++r) for (uint32_t v : field_values) {
        ++points;
        uint32_t w[2] = {0, 0}, pw[2] = {0, 0};
        set_wide_word_field(w, r, v);
        parent_put_wide_field(pw, (int)r, v);
        check(w[0] == pw[0] && w[1] == pw[1], "wide word differs from the parent's", r, v);
        for (uint32_t o = 0; o < 3; ++o) {
            const uint32_t want = o == r ? v : 0u;
            check(wide_word_field(w[0], w[1], o) == want && packed_word_field(w, 2, o) == want && parent_get_wide_field(w[0], w[1], (int)o) == want && parent_get_lane_field_validator(w, o, 2) == want, "wide word round trip", r, o, v);
        }
    }
    {
        ++points;
        uint32_t w[2] = {0, 0};
        for (uint32_t r = 0; r < 3; ++r) set_wide_word_field(w, r, encode_pack_field(300 + r, 400 + r, 7 - r));
        for (uint32_t r = 0; r < 3; ++r) {
            const CompactSlot d = decode_pack_field(wide_word_field(w[0], w[1], r));
            check(d.i == 300 + r && d.j == 400 + r && d.pal == 7 - r, "full wide word round trip", r);
        }
    }
    // rest lengths of the full lane-packed form
    for (uint32_t f = 0; f < 6; ++f) for (uint32_t lane : {0u, 127u}) {
        ++points;
        check(lane_pack_rest_dword(lane, f) == parent_rest_dword(lane, f) && lane_pack_rest_dword(lane, f) < kLanePackDwordsFull, "rest length dword", lane, f);
    }
    check(kLanePackDwordsCompact == 512 && kLanePackDwordsFull == 1280 && kWidePackDwords == 512 && kMaxPalette == 256 && kCompactMaxLocal == 4096, "layout sizes");
    std::printf("points %ld\n", points);
    return bad ? 1 : 0;
}
