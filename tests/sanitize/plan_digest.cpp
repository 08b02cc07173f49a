// Digest driver for the host planner (softbodyunity_amd/csrc/plan.cpp): for every case of a fixed corpus it builds the Plan and the
// LocalPlan of EVERY rank and prints `<case> <64-bit digest>` over every field of both -- the tile tables (rounds, lane order of
// t_dist / t_quad, gather, runs) included, which the other CPU tests do not see. tests/test_plan_digest.py compares the lines with
// tests/golden/plan_digests.json, so a change of the planner that is meant to leave plans alone can be shown to on a machine
// without a GPU. A planner exception is part of the digest (its message). CPU only.
//
//   plan_digest                 the fixed corpus
//   plan_digest --paths         ... and on stderr, per case, whether the counting sorts (dense grids) or the comparison sorts ran
//   plan_digest --corpus FILE   the entries of a corpus file in plan_corpus_san.cpp's format instead (differential runs)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "plan.hpp"
#include "plan_meshes.hpp"

namespace {

using namespace meshes;

struct Digest {                 // FNV-style, one 64-bit word at a time; every vector goes in with its length
    uint64_t h = 1469598103934665603ull;
    void u64(uint64_t v) { h = (h ^ v) * 1099511628211ull; h ^= h >> 29; }
    void i(int64_t v) { u64((uint64_t)v); }
    void f64(double v) { uint64_t b; std::memcpy(&b, &v, 8); u64(b); }
    void f32(float v) { uint32_t b; std::memcpy(&b, &v, 4); u64(b); }
    void str(const char *s) { for (; *s; ++s) u64((uint8_t)*s); u64(0x100); }
    template <class T> void ints(const std::vector<T> &v) { i((int64_t)v.size()); for (const T &x : v) i((int64_t)x); }
    void runs(const std::vector<sbp::Run> &v) { i((int64_t)v.size()); for (const sbp::Run &r : v) { i(r.start); i(r.len); } }
};

void add_domain(Digest &d, const sbp::Domain &m) {
    d.i(m.set); d.i(m.n_global); d.f64(m.ell); d.f64(m.fill);
    for (int a = 0; a < 3; ++a) { d.f64(m.lo[a]); d.f64(m.hi[a]); }
}

void add_plan(Digest &d, const sbp::Plan &P) {
    const sbp::Opts &o = P.opts;
    d.i(o.rank); d.i(o.world); d.i(o.tile_particles); d.i(o.partition); d.i(o.third_tiling); d.i(o.third_list); d.i(o.merge_tiles);
    d.i(o.balanced_lists); d.i(o.cluster_layers); d.i(o.mixed_groups); d.i(o.bank_aware_lanes);
    for (int a = 0; a < 3; ++a) d.i(o.dims[a]);
    add_domain(d, o.domain);
    d.i(P.n); d.i(P.tiling); d.i(P.partition);
    for (int a = 0; a < 3; ++a) { d.i(P.m[a]); d.i(P.dims[a]); }
    add_domain(d, P.domain);
    d.ints(P.rank_cost); d.ints(P.new_of_old); d.ints(P.old_of_new); d.ints(P.owner_of_old);
    for (int tl = 0; tl < 3; ++tl) {
        const sbp::Tiling &T = P.T[tl];
        d.i((int64_t)T.tiles.size());
        for (const sbp::Tile &t : T.tiles) {
            d.i(t.owner); d.i(t.run_begin); d.i(t.run_count); d.i(t.n_local); d.i(t.round_begin); d.i(t.n_rounds);
            d.i(t.d_begin); d.i(t.q_begin); d.i(t.d_end); d.i(t.q_end); d.i(t.seq_begin); d.i(t.seq_end);
            for (int p = 0; p < 2; ++p) { d.i(t.order_begin[p]); d.i(t.order_end[p]); }
            d.i(t.gather_begin);
        }
        d.runs(T.runs); d.ints(T.rounds); d.ints(T.t_dist); d.ints(T.t_dist_id); d.ints(T.t_quad); d.ints(T.t_quad_id);
        d.ints(T.t_quad_type); d.ints(T.gather); d.i(T.max_local); d.i(T.max_runs);
    }
    d.i((int64_t)P.t2_layers.size());
    for (const auto &l : P.t2_layers) { d.i(l.first); d.i(l.second); }
    d.i((int64_t)P.gcolours.size());
    for (const sbp::GColour &g : P.gcolours) { d.i(g.type); d.ints(g.ids); d.i(g.cut); }
    for (int p = 0; p < 2; ++p) {
        d.ints(P.order_type[p]); d.ints(P.order_id[p]);
        d.i((int64_t)P.phases[p].size());
        for (const sbp::Phase &ph : P.phases[p]) {
            d.i(ph.kind); d.i(ph.type); d.i(ph.tiling); d.i(ph.gcolour); d.i(ph.order_begin); d.i(ph.order_end);
            d.i(ph.task_begin); d.i(ph.task_end); d.i(ph.halo_slot); d.i(ph.layer);
        }
        d.ints(P.task_off[p]); d.ints(P.group_off[p]);
    }
    d.i(P.cons_in_tiles); d.i(P.cons_in_global);
}

void add_local(Digest &d, const sbp::LocalPlan &L) {
    d.i(L.rank); d.i(L.world); d.i(L.n_owned); d.ints(L.local_to_old);
    for (int tl = 0; tl < 3; ++tl) {
        const sbp::LocalTiling &T = L.T[tl];
        d.ints(T.tile_ids); d.runs(T.runs); d.ints(T.run_begin); d.ints(T.gather); d.ints(T.gather_begin);
    }
    d.i((int64_t)L.gcolours.size());
    for (const sbp::LocalGColour &g : L.gcolours) { d.i(g.type); d.ints(g.idx); d.ints(g.id); }
    d.i((int64_t)L.halo.size());
    for (const sbp::HaloSlot &H : L.halo) {
        d.i((int64_t)H.send_idx.size()); d.i((int64_t)H.recv_idx.size());
        for (const auto &v : H.send_idx) d.ints(v);
        for (const auto &v : H.recv_idx) d.ints(v);
    }
    for (int p = 0; p < 2; ++p) d.ints(L.order_mask[p]);
    d.ints(L.pair_hash);
}

bool g_paths = false;

// one rank's Plan + LocalPlan (or the planner's refusal) into the digest
void add_rank(Digest &d, const sbp::Input &in, const sbp::Opts &o) {
    try {
        sbp::Plan P; sbp::LocalPlan L;
        sbp::build_plan(in, o, P);
        sbp::extract_local(P, in, o.rank, L);
        add_plan(d, P); add_local(d, L);
        if (g_paths && o.rank == 0) {
            const sbp::Grid G = sbp::make_grid(P.domain, o.tile_particles > 0 ? o.tile_particles : 512);
            const int64_t lim = 8 * (int64_t)in.n + 4096, nc = (int64_t)G.nc[0] * G.nc[1] * G.nc[2];
            const int64_t ns = (int64_t)(G.nc[0] + 1) * (G.nc[1] + 1) * (G.nc[2] + 1);
            std::fprintf(stderr, "    n %d cells %lld: T1 %s, T0 %s, partition %d%s, fill %.2f, tiles %zu/%zu/%zu, T2 layers %zu, global colours %zu\n", in.n, (long long)nc,
                         o.tile_particles <= 0 ? "off" : (ns <= lim ? "counting sort" : "std::sort"),
                         o.tile_particles <= 0 ? "stable_sort by owner" : (o.world * nc <= lim ? "counting sort" : "std::sort"),
                         P.partition, P.partition == 2 ? (nc <= lim ? " (dense cells)" : " (sorted cells)") : "", P.domain.fill,
                         P.T[0].tiles.size(), P.T[1].tiles.size(), P.T[2].tiles.size(), P.t2_layers.size(), P.gcolours.size());
        }
    } catch (const std::exception &e) {
        d.str(e.what());
    }
}

void emit(const std::string &name, const Digest &d) { std::printf("%s %016llx\n", name.c_str(), (unsigned long long)d.h); }

void whole(const std::string &name, const Mesh &m, sbp::Opts o) {       // every rank of o.world plans the whole mesh
    if (g_paths) std::fprintf(stderr, "%s\n", name.c_str());
    Digest d;
    const sbp::Input in = m.input();
    for (o.rank = 0; o.rank < o.world; ++o.rank) add_rank(d, in, o);
    emit(name, d);
}
void whole(const std::string &name, const Mesh &m, int world, int tile, int partition = 0) {
    sbp::Opts o; o.world = world; o.tile_particles = tile; o.partition = partition;
    whole(name + "_w" + std::to_string(world) + "_t" + std::to_string(tile) + (partition ? "_p" + std::to_string(partition) : ""), m, o);
}

void sharded(const std::string &name, const Mesh &m, int world, int tile) {      // every rank plans its own window
    if (g_paths) std::fprintf(stderr, "%s\n", name.c_str());
    sbp::Input all = m.input();
    sbp::Domain dom;
    sbp::compute_domain(all, dom);
    dom.set = true;
    Digest d;
    for (int rank = 0; rank < world; ++rank) {
        sbp::Opts o; o.rank = rank; o.world = world; o.tile_particles = tile; o.domain = dom; o.partition = 1;
        const Mesh w = cut_window(m, dom, o);
        d.ints(w.gid);
        add_rank(d, w.input(), o);
    }
    emit(name, d);
}

int run_corpus_file(const char *path) {
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
        Digest d;
        const sbp::Input in = m.input();
        for (o.rank = (window_rank >= 0 ? window_rank : 0); o.rank < (window_rank >= 0 ? window_rank + 1 : world); ++o.rank) add_rank(d, in, o);
        emit("entry" + std::to_string(entry), d);
    }
    std::fclose(f);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc > 2 && !std::strcmp(argv[1], "--corpus")) return run_corpus_file(argv[2]);
    g_paths = argc > 1 && !std::strcmp(argv[1], "--paths");
    // the cases of plan_san.cpp, every rank
    const Mesh a = lattice(20), b = cloud(9000, 7), c = lattice(3), l = l_shape(b);
    for (int tile : {512, 64, -1}) { whole("lattice20", a, 1, tile); whole("cloud9000", b, 1, tile); }
    for (int world : {2, 3, 8}) { whole("lattice20", a, world, 64); whole("cloud9000", b, world, 128); whole("lattice3", c, world, 512); }
    for (int world : {3, 8}) { whole("lattice20", a, world, 64, 2); whole("cloud9000", b, world, 128, 2); }
    whole("lshape", l, 1, 128); whole("lshape", l, 8, 128); whole("lshape", l, 5, 64);
    sharded("sharded_lattice24_w8_t64", lattice(24), 8, 64); sharded("sharded_lattice20_w3_t27", lattice(20), 3, 27);
    {
        Mesh s; s.rest = {0.f, 0.f, 0.f};
        whole("single", s, 1, 512); whole("single", s, 2, 512);
    }
    // every switch of Opts turned once, on the mesh where all of them act
    for (int world : {1, 5}) {
        const std::string w = "_w" + std::to_string(world);
        auto with = [&](const char *name, void (*set)(sbp::Opts &)) {
            sbp::Opts o; o.world = world; o.tile_particles = 128;
            set(o);
            whole(std::string("lshape_") + name + w, l, o);
        };
        with("no_third_tiling", [](sbp::Opts &o) { o.third_tiling = false; });
        with("no_third_list", [](sbp::Opts &o) { o.third_list = false; });
        with("no_merge_tiles", [](sbp::Opts &o) { o.merge_tiles = false; });
        with("no_cluster_layers", [](sbp::Opts &o) { o.cluster_layers = false; });
        with("no_mixed_groups", [](sbp::Opts &o) { o.mixed_groups = false; });
        with("no_bank_aware_lanes", [](sbp::Opts &o) { o.bank_aware_lanes = false; });
        with("balanced_lists1", [](sbp::Opts &o) { o.balanced_lists = 1; });
        with("balanced_lists2", [](sbp::Opts &o) { o.balanced_lists = 2; });
        with("balanced_lists3", [](sbp::Opts &o) { o.balanced_lists = 3; });
    }
    {   // explicit block grids
        sbp::Opts o; o.world = 4; o.tile_particles = 64; o.dims[0] = 1; o.dims[1] = 4; o.dims[2] = 1;
        whole("lattice20_dims_1x4x1", a, o);
        o.world = 6; o.tile_particles = 128; o.dims[0] = 3; o.dims[1] = 1; o.dims[2] = 2;
        whole("cloud9000_dims_3x1x2", b, o);
    }
    // a particle of valence 300: more than 128 colours in its tile (greedy_colour_wide)
    { const Mesh h = hub(300, 4); whole("hub300", h, 1, 512); whole("hub300", h, 1, -1); whole("hub300", h, 2, 512); }
    // nearly all grid cells empty: the comparison sorts of T1, T0 and the RCB partition
    { const Mesh s = sparse_clusters(4, 600); whole("sparse", s, 1, 64); whole("sparse", s, 3, 64, 2); whole("sparse", s, 4, 8); }
    // every spring of the 26-neighbour stencil: T2 layers and global colours on a regular mesh
    { const Mesh f = lattice(10, true); whole("fullstencil10", f, 1, 64); whole("fullstencil10", f, 4, 64); }
    return 0;
}
