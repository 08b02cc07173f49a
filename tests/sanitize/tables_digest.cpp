// Digest driver for the host table builder (softbodyunity_amd/csrc/tables_host.cpp): for every case of a fixed corpus it plans the mesh,
// builds the tables of EVERY rank and prints `<case> <64-bit digest>` over everything in HostTables -- every vector with its length, every
// scalar of every tiling, the mailbox layout -- and over the device bytes this driver sums from their sizes (tables.hip's own accounting
// is not run here; the parent build digests build_device's dev_bytes in that place). tests/test_tables_digest.py compares
// the lines with tests/golden/tables_digests.json. CPU only; links no HIP runtime.
//
//   tables_digest              the fixed corpus
//   tables_digest --paths      ... and on stderr, per case, `paths <case> <name> ...`: the branches of the builder the case reached
//   tables_digest --corpus F   the entries of a corpus file in plan_corpus_san.cpp's format instead (differential runs)
//
// -DTABLES_DIGEST_PARENT builds the same driver over a build_device that uploads as it goes (the tables.hip this unit was split out
// of): that tables.hip is compiled for the host with the HIP memory calls renamed to the stand-ins below (-DhipMalloc=sb_host_malloc
// ...), an sb_solver is filled by hand, and what its DevBufs then point at is digested. That is where the golden file comes from.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#ifdef TABLES_DIGEST_PARENT
#include "solver_internal.hpp"
#else
#include "tables_host.hpp"
#include "../../include/softbody_debug.h"
#endif
#include "plan_meshes.hpp"

namespace {

using namespace meshes;

struct Digest {                 // as plan_digest.cpp: FNV-style, one 64-bit word at a time
    uint64_t h = 1469598103934665603ull;
    void u64(uint64_t v) { h = (h ^ v) * 1099511628211ull; h ^= h >> 29; }
    void i(int64_t v) { u64((uint64_t)v); }
    void str(const char *s) { for (; *s; ++s) u64((uint8_t)*s); u64(0x100); }
    template <class T> void ints(const std::vector<T> &v) { i((int64_t)v.size()); for (const T &x : v) i((int64_t)x); }
};

struct Span {                   // an uploaded array: elements of `elem` bytes (1, or a multiple of 4)
    const void *p = nullptr; size_t n = 0, elem = 4;
    template <class T> static Span of(const std::vector<T> &v) { return {v.data(), v.size(), sizeof(T)}; }
    template <class T> static Span of(const T *p, size_t n) { return {p, n, sizeof(T)}; }
    size_t bytes() const { return n * elem; }
};
void add(Digest &d, const Span &s) {
    d.i((int64_t)s.n);
    if (s.elem == 1) { for (size_t k = 0; k < s.n; ++k) d.u64(((const uint8_t *)s.p)[k]); return; }
    for (size_t k = 0; k < s.bytes() / 4; ++k) { uint32_t w; std::memcpy(&w, (const char *)s.p + 4 * k, 4); d.u64(w); }
}

// What a rank's solver holds once its tables are built, whoever built them.
struct View {
    int64_t n_owned = 0, n_local = 0, dev_bytes = 0;
    Span pos3, vel, wf, w8, wpal;
    bool w_palette = false, w_uniform = false, fused_unpack = false;
    struct Tiling {
        int64_t scalars[14];
        Span tiles, overflow, stream, gather;
        const sbk::TileDesc *td(size_t t) const { return (const sbk::TileDesc *)tiles.p + t; }
        const uint32_t *words() const { return (const uint32_t *)stream.p; }
    } T[3];
    std::vector<std::pair<int32_t, int32_t>> t2_layer_range;
    struct GColour { int type; int32_t count; Span ij, rest, quad, rest2; };
    std::vector<GColour> gcolours;
    struct Halo { std::vector<int> peers; std::vector<int32_t> send_off, recv_off; Span send_idx, recv_idx; };
    std::vector<Halo> halos;
    size_t send_floats = 0, recv_floats = 0;
    bool has_mailbox = false;
    int64_t mb_slots = 0, mb_off_table = 0, mb_data_off = 0, mb_bytes = 0;
    Span mb_header;
    std::vector<std::vector<uint32_t>> mb_my_off;
};
template <class S> void copy_scalars(View::Tiling &t, const S &s) {       // S: the scalar block of a tiling (DevTiling's own fields)
    const int64_t v[14] = {s.n_tiles, (int64_t)s.lds_bytes, s.n_slots, s.staged_particles, s.stream_bytes, s.n_programs, s.max_local, s.win_dwords,
                           s.pal_dwords, s.rounds_dwords, s.n_boundary, s.has_quads, s.item_waves * 1000 + s.packed_lanes, s.n_packed_tiles};
    std::memcpy(t.scalars, v, sizeof(v));
}
void add(Digest &d, const View &v) {
    d.i(v.n_owned); d.i(v.n_local); d.i(v.dev_bytes); d.i(v.w_palette); d.i(v.w_uniform); d.i(v.fused_unpack);
    add(d, v.pos3); add(d, v.vel); add(d, v.wf); add(d, v.w8); add(d, v.wpal);
    for (const View::Tiling &t : v.T) {
        for (int64_t s : t.scalars) d.i(s);
        add(d, t.tiles); add(d, t.overflow); add(d, t.stream); add(d, t.gather);
    }
    d.i((int64_t)v.t2_layer_range.size());
    for (const auto &r : v.t2_layer_range) { d.i(r.first); d.i(r.second); }
    d.i((int64_t)v.gcolours.size());
    for (const View::GColour &g : v.gcolours) { d.i(g.type); d.i(g.count); add(d, g.ij); add(d, g.rest); add(d, g.quad); add(d, g.rest2); }
    d.i((int64_t)v.halos.size());
    for (const View::Halo &h : v.halos) { d.ints(h.peers); d.ints(h.send_off); d.ints(h.recv_off); add(d, h.send_idx); add(d, h.recv_idx); }
    d.i((int64_t)v.send_floats); d.i((int64_t)v.recv_floats);
    d.i(v.has_mailbox); d.i(v.mb_slots); d.i(v.mb_off_table); d.i(v.mb_data_off); d.i(v.mb_bytes);
    add(d, v.mb_header);
    d.i((int64_t)v.mb_my_off.size());
    for (const auto &o : v.mb_my_off) d.ints(o);
}

// ---- a case: mesh, state, planner options, the solver fields that shape the tables ---------------------------------------------------------

enum Mass { kUniform, kFew, kMany };
struct Tuning {
    uint32_t flags = 0;
    int tile_lanes = 0, quad_lanes = 512, narrow_min_tiles = 10240, win_dwords_cap = 0;
    bool pack_tiles = true, split = false, peer = false, sharded = false;
    Mass mass = kUniform;
    bool varied_rest = false;        // every spring its own rest length (else: the distance of its particles at rest)
};
struct State { std::vector<float> pos, vel, invm, dist_rest, vol_rest, bend_rest; };

State make_state(const Mesh &m, const Tuning &t) {
    State s;
    const size_t n = m.rest.size() / 3;
    s.pos = m.rest; s.vel.resize(3 * n); s.invm.resize(n);
    for (size_t k = 0; k < 3 * n; ++k) { s.pos[k] += 0.001f * (float)(k % 7); s.vel[k] = 0.25f * (float)((k * 5) % 11) - 1.0f; }
    for (size_t p = 0; p < n; ++p) s.invm[p] = t.mass == kUniform ? 1.0f : t.mass == kFew ? 1.0f / (float)(1 + p % 3) : 1.0f + 0.001f * (float)(p % 1000);
    for (size_t k = 0; k + 2 <= m.dist.size(); k += 2) {
        const float *a = &m.rest[3 * (size_t)m.dist[k]], *b = &m.rest[3 * (size_t)m.dist[k + 1]];
        const float r = std::sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]));
        s.dist_rest.push_back(t.varied_rest ? 1.0f + 1e-5f * (float)(k / 2) : r);
    }
    for (size_t k = 0; k < m.vol.size() / 4; ++k) s.vol_rest.push_back(0.1f + 0.01f * (float)(k % 13));
    for (size_t k = 0; k < m.bend.size() / 4; ++k) { s.bend_rest.push_back(0.5f + 0.125f * (float)(k % 5)); s.bend_rest.push_back(1.0f + 0.0625f * (float)(k % 3)); }
    return s;
}

// abi.hip plan_shape: mailbox header word 3
uint32_t shape_of(const sbp::Plan &P) {
    return 1u + (P.tiling ? 1u : 0u) + 4u * (uint32_t)std::min<size_t>(P.t2_layers.size(), 0xfffu) + 0x4000u * (uint32_t)std::min<size_t>(P.gcolours.size(), 0xffffu);
}
uint64_t hash_of(const sbp::Plan &P) { return 0x9e3779b97f4a7c15ull * (uint64_t)(P.n + 1) + (uint64_t)P.opts.world; }     // (any value: it only travels into the header)

bool g_paths = false;
std::set<std::string> g_reached;

}  // namespace

#ifdef TABLES_DIGEST_PARENT
// ---- host stand-ins for the HIP calls build_device makes, and the rest of the library it refers to ----------------------------------------
extern "C" {
hipError_t sb_host_malloc(void **p, size_t n) { *p = std::calloc(1, n ? n : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t sb_host_ext_malloc(void **p, size_t n, unsigned int) { return sb_host_malloc(p, n); }
hipError_t sb_host_host_malloc(void **p, size_t n, unsigned int) { return sb_host_malloc(p, n); }
hipError_t sb_host_memcpy(void *d, const void *s, size_t n, hipMemcpyKind) { std::memcpy(d, s, n); return hipSuccess; }
hipError_t sb_host_memset(void *d, int v, size_t n) { std::memset(d, v, n); return hipSuccess; }
hipError_t sb_host_free(void *p) { std::free(p); return hipSuccess; }
hipError_t sb_host_host_free(void *p) { std::free(p); return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "hip"; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipGraphExecDestroy(hipGraphExec_t) { return hipSuccess; }
hipError_t hipIpcCloseMemHandle(void *) { return hipSuccess; }
}
namespace sbi {
uint32_t plan_shape(const sb_solver *s) { return shape_of(s->plan->plan); }
int fail(int code, const std::string &) { return code; }
RcclApi &rccl(bool) { static RcclApi api; return api; }
ExchangeTimer::~ExchangeTimer() {}
}  // namespace sbi
#endif

namespace {

#ifdef TABLES_DIGEST_PARENT
struct Built {
    std::unique_ptr<sb_solver> s;
    View view() const {
        View v;
        v.n_owned = s->n_owned; v.n_local = s->n_local; v.dev_bytes = s->dev_bytes;
        v.pos3 = Span::of(s->d_pos3.p, s->d_pos3.count); v.vel = Span::of(s->d_vel.p, s->d_vel.count); v.wf = Span::of(s->d_wf.p, s->d_wf.count);
        v.w8 = Span::of(s->d_w8.p, s->d_w8.count); v.wpal = Span::of(s->d_wpal.p, s->d_wpal.count);
        v.w_palette = s->w_palette; v.w_uniform = s->w_uniform; v.fused_unpack = s->fused_unpack;
        for (int tl = 0; tl < 3; ++tl) {
            const DevTiling &D = s->tiling[tl];
            copy_scalars(v.T[tl], D);
            v.T[tl].tiles = Span::of(D.tiles.p, D.tiles.count); v.T[tl].overflow = Span::of(D.runs_overflow.p, D.runs_overflow.count);
            v.T[tl].stream = Span::of(D.stream.p, D.stream.count); v.T[tl].gather = Span::of(D.gather.p, D.gather.count);
        }
        v.t2_layer_range = s->t2_layer_range;
        for (const auto &G : s->gcolours)
            v.gcolours.push_back({G->type, G->count, Span::of(G->ij.p, G->ij.count), Span::of(G->rest.p, G->rest.count), Span::of(G->quad.p, G->quad.count), Span::of(G->rest2.p, G->rest2.count)});
        for (const auto &G : s->halos)
            v.halos.push_back({G->peers, G->send_off, G->recv_off, Span::of(G->send_idx.p, G->send_idx.count), Span::of(G->recv_idx.p, G->recv_idx.count)});
        v.send_floats = s->d_sendbuf.count; v.recv_floats = s->d_recvbuf.count;
        const auto &PS = s->peer;
        v.has_mailbox = PS.mailbox != nullptr;
        if (v.has_mailbox) {
            v.mb_slots = PS.n_slots; v.mb_off_table = (int64_t)PS.off_table; v.mb_data_off = (int64_t)PS.data_off_words; v.mb_bytes = (int64_t)PS.bytes;
            v.mb_header = Span::of(PS.mailbox, PS.data_off_words); v.mb_my_off = PS.my_off;
        }
        return v;
    }
};
Built build(const sbp::Input &in, const sbp::Opts &o, const State &st, const Tuning &t) {
    Built b;
    b.s.reset(new sb_solver());
    sb_solver *s = b.s.get();
    s->plan.reset(new sb_plan());
    sbp::build_plan(in, o, s->plan->plan);
    sbp::extract_local(s->plan->plan, in, o.rank, s->plan->local);
    s->pos = st.pos; s->vel = st.vel; s->invm = st.invm; s->dist_rest = st.dist_rest; s->vol_rest = st.vol_rest; s->bend_rest = st.bend_rest;
    s->tune_flags = t.flags; s->tile_lanes = t.tile_lanes; s->quad_lanes = t.quad_lanes; s->narrow_min_tiles = t.narrow_min_tiles;
    s->win_dwords_cap = t.win_dwords_cap; s->pack_tiles = t.pack_tiles; s->overlap_halo = t.split; s->peer.enabled = t.peer; s->sharded = t.sharded;
    s->plan_hash = hash_of(s->plan->plan);
    sbi::build_device(s);
    return b;
}
#else
struct Built {
    sbp::Plan P; sbp::LocalPlan L;
    sbt::TableOptions opt;
    sbt::HostTables H;
    View view() const {
        View v;
        v.n_owned = H.n_owned; v.n_local = H.n_local;
        v.pos3 = Span::of(H.pos3); v.vel = Span::of(H.vel); v.wf = Span::of(H.wf); v.w8 = Span::of(H.w8); v.wpal = Span::of(H.wpal);
        v.w_palette = H.w_palette; v.w_uniform = H.w_uniform; v.fused_unpack = H.fused_unpack;
        // what tables.hip build_device accounts for: every upload, the previous positions, the tick parameters, the exchange buffers, the mailbox
        int64_t bytes = (int64_t)(v.pos3.bytes() + v.vel.bytes() + v.wf.bytes() + v.w8.bytes() + v.wpal.bytes()) + H.n_local * 12 + (int64_t)sizeof(sbk::TickParams);
        for (int tl = 0; tl < 3; ++tl) {
            const sbt::HostTiling &D = H.T[tl];
            copy_scalars(v.T[tl], D);
            v.T[tl].tiles = Span::of(D.tiles); v.T[tl].overflow = Span::of(D.runs_overflow); v.T[tl].stream = Span::of(D.stream); v.T[tl].gather = Span::of(D.gather);
            bytes += (int64_t)(v.T[tl].tiles.bytes() + v.T[tl].overflow.bytes() + v.T[tl].stream.bytes() + v.T[tl].gather.bytes());
        }
        v.t2_layer_range = H.t2_layer_range;
        for (const sbt::HostGColour &G : H.gcolours) {
            v.gcolours.push_back({G.type, G.count, Span::of(G.ij), Span::of(G.rest), Span::of(G.quad), Span::of(G.rest2)});
            bytes += (int64_t)(Span::of(G.ij).bytes() + Span::of(G.rest).bytes() + Span::of(G.quad).bytes() + Span::of(G.rest2).bytes());
        }
        for (const sbt::HostHalo &G : H.halos) {
            v.halos.push_back({G.peers, G.send_off, G.recv_off, Span::of(G.send_idx), Span::of(G.recv_idx)});
            bytes += (int64_t)(Span::of(G.send_idx).bytes() + Span::of(G.recv_idx).bytes());
        }
        v.send_floats = H.send_floats; v.recv_floats = H.recv_floats;
        bytes += (int64_t)(4 * (H.send_floats + H.recv_floats));
        const sbt::HostMailbox &M = H.mailbox;
        v.has_mailbox = opt.peer_enabled && L.world > 1;
        if (v.has_mailbox) {
            v.mb_slots = M.n_slots; v.mb_off_table = (int64_t)M.off_table; v.mb_data_off = (int64_t)M.data_off_words; v.mb_bytes = (int64_t)M.bytes;
            v.mb_header = Span::of(M.header); v.mb_my_off = M.my_off;
            bytes += (int64_t)M.bytes;
        }
        v.dev_bytes = bytes;
        return v;
    }
};
Built build(const sbp::Input &in, const sbp::Opts &o, const State &st, const Tuning &t) {
    Built b;
    sbp::build_plan(in, o, b.P);
    sbp::extract_local(b.P, in, o.rank, b.L);
    sbt::TableOptions &opt = b.opt;
    opt.tune_flags = t.flags; opt.tile_lanes = t.tile_lanes; opt.quad_lanes = t.quad_lanes; opt.narrow_min_tiles = t.narrow_min_tiles;
    opt.win_dwords_cap = t.win_dwords_cap; opt.pack_tiles = t.pack_tiles; opt.split_launches = t.split; opt.peer_enabled = t.peer; opt.sharded = t.sharded;
    opt.plan_hash = hash_of(b.P);
    opt.plan_shape = t.peer && o.world > 1 ? shape_of(b.P) : 0u;
    const sbt::TableInput ti{&b.P, &b.L, st.pos.data(), st.vel.data(), st.invm.data(), st.dist_rest.data(), st.vol_rest.data(), st.bend_rest.data(),
                             (int64_t)st.vol_rest.size(), (int64_t)st.bend_rest.size()};
    sbt::build_tables(ti, opt, b.H);
    return b;
}
#endif

#ifndef TABLES_DIGEST_PARENT
// the branches of the builder a rank's tables show it took
void note_paths(const View &v, const View *unordered, const sbp::Opts &o, const Tuning &t, size_t n_plan_tiles[3]) {
    auto hit = [](const std::string &s) { g_reached.insert(s); };
    const std::string w = "_w" + std::to_string(o.world);
    hit(v.w_uniform ? "uniform_mass" : v.w_palette ? "mass_palette" : "float_masses");
    for (int tl = 0; tl < 3; ++tl) {
        const View::Tiling &T = v.T[tl];
        const int64_t n_tiles = T.scalars[0], n_boundary = T.scalars[10], item_waves = T.scalars[12] / 1000;
        if (tl < 2 && n_boundary > 0 && n_boundary < n_tiles) hit("boundary_order_t" + std::to_string(tl) + w);
        if ((size_t)n_tiles < n_plan_tiles[tl]) hit("multi_member_packs");
        if (T.overflow.n) hit("run_overflow");
        if (tl == 2 && v.t2_layer_range.size() >= 2 && T.gather.n) hit("t2_gather_layers");
        if (T.scalars[5] < n_tiles) hit("shared_programs");
        if ((t.flags & SB_TUNE_NO_SHARED_PROGRAMS) && n_tiles > 1) hit("unshared_programs");
        for (int64_t k = 0; k < n_tiles; ++k) {
            const sbk::TileDesc &td = *T.td((size_t)k);
            int nd = 0, nv = 0, nb = 0;
            for (int r = 0; r < td.n_rounds; ++r) { const sbk::GroupWord g = sbk::decode_group_word(T.words()[td.s_begin + r]); nd += (int)g.n_dist; nv += (int)g.n_vol; nb += (int)g.n_bend; }
            if (td.packed_lanes == 128) hit(td.n_pal ? "lane_packed_compact" : "lane_packed_full");
            else if (td.packed_lanes == 256) hit("wide_packed");
            else if (nd) hit(td.n_pal ? "dictionary_slots" : "full_slots");
            if (nd && !td.n_pal && !(t.flags & SB_TUNE_NO_PALETTE)) hit("palette_overflow");
            if (td.n_steps) hit("wave_items_" + std::to_string(64 * item_waves));
            if (nv) hit("tet_slots");
            if (nb) hit("hinge_slots");
        }
        if (unordered && T.tiles.n == unordered->T[tl].tiles.n && std::memcmp(T.tiles.p, unordered->T[tl].tiles.p, T.tiles.bytes()) != 0)
            hit(tl == 2 ? "cost_order_t2_layers" : (t.split && n_boundary > 0 && n_boundary < n_tiles) ? "cost_order_split_ranges" : "cost_order_one_range");
    }
    for (const View::GColour &g : v.gcolours) hit("gcolour_type" + std::to_string(g.type));
    if (o.world > 1) hit(v.fused_unpack ? "fused_unpack" : "no_fused_unpack");
    if (v.has_mailbox) hit("mailbox" + w);
}
#endif

// one rank's tables (or the refusal of the planner / the builder) into the digest
void add_rank(Digest &d, const sbp::Input &in, const sbp::Opts &o, const State &st, const Tuning &t) {
    try {
        const Built b = build(in, o, st, t);
        const View v = b.view();
        add(d, v);
        if (!g_paths) return;
#ifndef TABLES_DIGEST_PARENT
        size_t n_plan_tiles[3];
        for (int tl = 0; tl < 3; ++tl) n_plan_tiles[tl] = b.L.T[tl].tile_ids.size();
        if (t.flags & SB_TUNE_NO_COST_ORDER) { note_paths(v, nullptr, o, t, n_plan_tiles); return; }
        Tuning u = t; u.flags |= SB_TUNE_NO_COST_ORDER;
        const Built c = build(in, o, st, u);
        const View cv = c.view();
        note_paths(v, &cv, o, t, n_plan_tiles);
#endif
    } catch (const std::exception &e) {
        d.str(e.what());
    }
}

void emit(const std::string &name, const Digest &d) {
    std::printf("%s %016llx\n", name.c_str(), (unsigned long long)d.h);
    if (!g_paths) return;
    std::fprintf(stderr, "paths %s", name.c_str());
    for (const std::string &p : g_reached) std::fprintf(stderr, " %s", p.c_str());
    std::fprintf(stderr, "\n");
    g_reached.clear();
}

void whole(const std::string &name, const Mesh &m, int world, int tile, const Tuning &t = Tuning(), int partition = 0) {      // every rank plans the whole mesh
    sbp::Opts o; o.world = world; o.tile_particles = tile; o.partition = partition;
    const State st = make_state(m, t);
    const sbp::Input in = m.input();
    Digest d;
    for (o.rank = 0; o.rank < o.world; ++o.rank) add_rank(d, in, o, st, t);
    emit(name + "_w" + std::to_string(world) + "_t" + std::to_string(tile), d);
}

void sharded(const std::string &name, const Mesh &m, int world, int tile, Tuning t) {      // every rank plans its own window
    sbp::Input all = m.input();
    sbp::Domain dom;
    sbp::compute_domain(all, dom);
    dom.set = true;
    t.sharded = true;
    Digest d;
    for (int rank = 0; rank < world; ++rank) {
        sbp::Opts o; o.rank = rank; o.world = world; o.tile_particles = tile; o.domain = dom; o.partition = 1;
        const Mesh w = cut_window(m, dom, o);
        add_rank(d, w.input(), o, make_state(w, t), t);
    }
    emit(name, d);
}

int run_corpus_file(const char *path) {      // (plan_corpus_san.cpp's format; two table shapes per entry)
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::perror("corpus"); return 2; }
    for (int entry = 0;; ++entry) {
        int32_t h[12];
        if (std::fread(h, sizeof(int32_t), 12, f) != 12) break;
        const int32_t n = h[0], md = h[1], mv = h[2], mb = h[3], world = h[4], window_rank = h[7];
        double dom[9] = {0};
        Mesh m;
        if (window_rank >= 0) {
            m.gid.resize((size_t)n);
            if (std::fread(dom, sizeof(double), 9, f) != 9 || std::fread(m.gid.data(), sizeof(int32_t), m.gid.size(), f) != m.gid.size()) return 2;
        }
        m.rest.resize((size_t)3 * n); m.dist.resize((size_t)2 * md); m.vol.resize((size_t)4 * mv); m.bend.resize((size_t)4 * mb);
        bool ok = std::fread(m.rest.data(), sizeof(float), m.rest.size(), f) == m.rest.size();
        ok = ok && std::fread(m.dist.data(), sizeof(int32_t), m.dist.size(), f) == m.dist.size();
        ok = ok && std::fread(m.vol.data(), sizeof(int32_t), m.vol.size(), f) == m.vol.size();
        ok = ok && std::fread(m.bend.data(), sizeof(int32_t), m.bend.size(), f) == m.bend.size();
        if (!ok) { std::fprintf(stderr, "truncated corpus\n"); return 2; }
        sbp::Opts o; o.world = world; o.tile_particles = h[5]; o.partition = h[6];
        for (int a = 0; a < 3; ++a) o.dims[a] = h[8 + a];
        if (o.tile_particles == 0) o.tile_particles = (mv + mb > 0) ? 256 : 512;
        if (window_rank >= 0) {
            o.domain.set = true; o.domain.n_global = (int64_t)dom[0]; o.domain.ell = dom[7]; o.domain.fill = dom[8];
            for (int a = 0; a < 3; ++a) { o.domain.lo[a] = dom[1 + a]; o.domain.hi[a] = dom[4 + a]; }
        }
        bool valid = true;      // (the ABI refuses out-of-range indices before the tables are built; the state arrays are indexed by them)
        for (int32_t v : m.dist) valid = valid && v >= 0 && v < n;
        Digest d;
        if (valid) {
            const sbp::Input in = m.input();
            Tuning t[2];
            t[0].narrow_min_tiles = 4; t[0].split = true;
            t[1].peer = true; t[1].mass = kMany; t[1].varied_rest = true; t[1].quad_lanes = 256; t[1].sharded = window_rank >= 0;
            for (const Tuning &tt : t) {
                const State st = make_state(m, tt);
                for (o.rank = (window_rank >= 0 ? window_rank : 0); o.rank < (window_rank >= 0 ? window_rank + 1 : world); ++o.rank) add_rank(d, in, o, st, tt);
            }
        }
        emit("entry" + std::to_string(entry), d);
    }
    std::fclose(f);
    return 0;
}

Tuning with(void (*set)(Tuning &)) { Tuning t; set(t); return t; }

}  // namespace

int main(int argc, char **argv) {
    if (argc > 2 && !std::strcmp(argv[1], "--corpus")) return run_corpus_file(argv[2]);
    g_paths = argc > 1 && !std::strcmp(argv[1], "--paths");
    const Mesh a = lattice(20), b = cloud(9000, 7), l = l_shape(b), f = lattice(10, true);
    // springs on a lattice: packs of rim tiles, shared programs, the three mass forms, the packed slot forms (narrow_min_tiles made small)
    whole("lattice20", a, 1, 64);
    whole("lattice20_few_masses", a, 1, 512, with([](Tuning &t) { t.mass = kFew; }));
    whole("lattice20_float_masses", a, 1, 64, with([](Tuning &t) { t.mass = kMany; }));
    whole("lattice20_lane_compact", a, 1, 64, with([](Tuning &t) { t.narrow_min_tiles = 8; }));
    whole("lattice20_lane_full", a, 1, 512, with([](Tuning &t) { t.narrow_min_tiles = 8; t.mass = kMany; t.varied_rest = true; }));
    whole("lattice20_lane_mixed", a, 1, 64, with([](Tuning &t) { t.narrow_min_tiles = 8; t.mass = kMany; t.varied_rest = true; }));
    whole("lattice20_varied_rest", a, 1, 512, with([](Tuning &t) { t.varied_rest = true; }));      // > kMaxPalette rest lengths in a tile: full slots
    whole("lattice20_no_tiling", a, 1, -1);
    whole("lattice80_wide", lattice(80), 1, 512);       // more than kWide8MaxTiles full-size tiles: 8-byte wide-packed words
    // tets and hinges on an irregular cloud: wave items, long run tables, T2 layers, global colours, cost order
    whole("cloud9000", b, 1, 128, with([](Tuning &t) { t.mass = kFew; }));
    whole("cloud9000_quad256", b, 1, 512, with([](Tuning &t) { t.quad_lanes = 256; }));
    whole("cloud9000_no_tiling", b, 1, -1);
    whole("lshape", l, 1, 128); whole("lshape_t64", l, 5, 64, with([](Tuning &t) { t.split = true; }));
    whole("fullstencil10", f, 1, 64); whole("fullstencil10", f, 4, 64, with([](Tuning &t) { t.peer = true; }));
    // ranks: boundary tiles first / last, fused unpack, the overlapped schedule's split ranges, the peer mailbox
    for (int world : {2, 8}) {
        whole("lattice20_ranks", a, world, 64);
        whole("lattice20_ranks_split", a, world, 64, with([](Tuning &t) { t.split = true; t.varied_rest = true; }));
        whole("lattice20_ranks_peer", a, world, 64, with([](Tuning &t) { t.peer = true; }));
        whole("cloud9000_ranks_split", b, world, 128, with([](Tuning &t) { t.split = true; t.mass = kMany; }));
        whole("cloud9000_ranks_peer", b, world, 128, with([](Tuning &t) { t.peer = true; }));
    }
    whole("lshape_rcb", l, 3, 128, with([](Tuning &t) { t.split = true; }), 2);
    sharded("sharded_lattice24_w8_t64", lattice(24), 8, 64, with([](Tuning &t) { t.peer = true; }));
    sharded("sharded_lattice20_w3_t27", lattice(20), 3, 27, Tuning());
    { Mesh s; s.rest = {0.f, 0.f, 0.f}; whole("single", s, 1, 512); whole("single", s, 2, 512, with([](Tuning &t) { t.peer = true; })); }
    // every switch build_device reads, turned once where it acts (SB_TUNE_PEER_COARSE only picks the mailbox's allocator: not a table)
    whole("tune_no_mass_palette", a, 1, 64, with([](Tuning &t) { t.flags = SB_TUNE_NO_MASS_PALETTE; t.mass = kFew; }));
    whole("tune_no_uniform_mass", a, 1, 64, with([](Tuning &t) { t.flags = SB_TUNE_NO_UNIFORM_MASS; }));
    whole("tune_no_palette", a, 1, 64, with([](Tuning &t) { t.flags = SB_TUNE_NO_PALETTE; t.narrow_min_tiles = 8; }));
    whole("tune_no_wave_items", b, 1, 128, with([](Tuning &t) { t.flags = SB_TUNE_NO_WAVE_ITEMS; }));
    whole("tune_no_lane_pack", a, 1, 64, with([](Tuning &t) { t.flags = SB_TUNE_NO_LANE_PACK; t.narrow_min_tiles = 8; }));
    whole("tune_no_cost_order", b, 1, 128, with([](Tuning &t) { t.flags = SB_TUNE_NO_COST_ORDER; }));
    whole("tune_no_fused_unpack", a, 2, 64, with([](Tuning &t) { t.flags = SB_TUNE_NO_FUSED_UNPACK; }));
    whole("tune_no_wide_slots", lattice(80), 1, 512, with([](Tuning &t) { t.flags = SB_TUNE_NO_WIDE_SLOTS; }));
    whole("tune_no_shared_programs", a, 1, 64, with([](Tuning &t) { t.flags = SB_TUNE_NO_SHARED_PROGRAMS; }));
    whole("tune_no_pack", a, 1, 64, with([](Tuning &t) { t.pack_tiles = false; }));
    whole("tune_win_dwords", b, 1, 512, with([](Tuning &t) { t.win_dwords_cap = 2048; }));
    whole("tune_tile_lanes256", a, 1, 64, with([](Tuning &t) { t.tile_lanes = 256; t.narrow_min_tiles = 8; }));
    whole("tune_tile_lanes128", lattice(80), 1, 512, with([](Tuning &t) { t.tile_lanes = 128; }));
    return 0;
}
