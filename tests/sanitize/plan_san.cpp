// AddressSanitizer / UBSan driver for the host planner and the host table builder (softbodyunity_amd/csrc/plan.cpp, tables_host.cpp):
// builds plans, and the tables of every plan (tables_san.hpp), for a lattice, an
// irregular cloud with 4-vertex constraints and a few degenerate inputs, for several world sizes, and checks the basic
// partition invariants. CPU only (GPU sanitizers are not available on the pool); built and run by tests/test_sanitizers.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <vector>

#include "plan.hpp"
#include "plan_meshes.hpp"
#include "tables_san.hpp"

namespace {

using namespace meshes;

void check(const Mesh &m, int world, int tile, int partition = 0) {
    const sbp::Input in = m.input();
    for (int rank = 0; rank < world; rank += (world > 4 ? 3 : 1)) {
        sbp::Opts o; o.rank = rank; o.world = world; o.tile_particles = tile; o.partition = partition;
        sbp::Plan P; sbp::LocalPlan L;
        sbp::build_plan(in, o, P);
        sbp::extract_local(P, in, rank, L);
        const int64_t total = in.m_d + in.m_v + in.m_b;
        for (int par = 0; par < 2; ++par)
            if ((int64_t)P.order_id[par].size() != total) throw std::runtime_error("order does not cover every constraint");
        std::vector<char> seen(in.n, 0);
        for (int32_t q : P.old_of_new) { if (q < 0 || q >= in.n || seen[q]) throw std::runtime_error("numbering is not a permutation"); seen[q] = 1; }
        if (L.n_owned < 0 || L.n_owned > (int64_t)L.local_to_old.size()) throw std::runtime_error("bad owned count");
        for (const auto &H : L.halo)
            if ((int)H.send_idx.size() != world || (int)H.recv_idx.size() != world) throw std::runtime_error("halo slot size");
        san_tables(in, P, L);
    }
}

// Sharded authoring: every rank plans the window rank_window() gives it; owned counts must add up to the whole mesh and the pair
// hashes must be symmetric.
void check_sharded(const Mesh &m, int world, int tile) {
    sbp::Input whole{m.rest.data(), (int32_t)(m.rest.size() / 3), m.dist.data(), (int64_t)m.dist.size() / 2, nullptr, 0, nullptr, 0};
    sbp::Domain dom;
    sbp::compute_domain(whole, dom);
    dom.set = true;
    std::vector<std::vector<uint64_t>> pair((size_t)world);
    int64_t owned_total = 0;
    for (int rank = 0; rank < world; ++rank) {
        sbp::Opts o; o.rank = rank; o.world = world; o.tile_particles = tile; o.domain = dom; o.partition = 1;
        const Mesh w = cut_window(m, dom, o);
        const sbp::Input in = w.input();
        sbp::Plan P; sbp::LocalPlan L;
        sbp::build_plan(in, o, P);
        sbp::extract_local(P, in, rank, L);
        san_tables(in, P, L);
        owned_total += L.n_owned;
        pair[(size_t)rank] = L.pair_hash;
    }
    if (owned_total != whole.n) throw std::runtime_error("sharded ranks do not own the whole mesh between them");
    for (int a = 0; a < world; ++a) for (int b = 0; b < world; ++b) if (a != b && pair[(size_t)a][(size_t)b] != pair[(size_t)b][(size_t)a]) throw std::runtime_error("pair hashes are not symmetric");
}

template <class F> void expect_throw(const char *what, F f) {
    try { f(); } catch (const std::exception &) { return; }
    std::fprintf(stderr, "expected an exception: %s\n", what);
    std::exit(2);
}

}  // namespace

int main() {
    const Mesh a = lattice(20), b = cloud(9000, 7), c = lattice(3);
    for (int tile : {512, 64, -1}) { check(a, 1, tile); check(b, 1, tile); }
    for (int world : {2, 3, 8}) { check(a, world, 64); check(b, world, 128); check(c, world, 512); }
    for (int world : {3, 8}) { check(a, world, 64, 2); check(b, world, 128, 2); }       // RCB forced
    {   // a mesh that fills its box unevenly: fill-aware grid, balanced lists, tile merge; automatic partition (RCB)
        const Mesh l = l_shape(b);
        check(l, 1, 128); check(l, 8, 128); check(l, 5, 64);
    }
    check_sharded(lattice(24), 8, 64); check_sharded(lattice(20), 3, 27);
    {   // a single particle, no constraints
        Mesh s; s.rest = {0.f, 0.f, 0.f};
        check(s, 1, 512); check(s, 2, 512);
    }
    Mesh bad = lattice(4);
    bad.dist[1] = 1000;
    expect_throw("index out of range", [&] { check(bad, 1, 512); });
    Mesh nan = lattice(4);
    nan.rest[5] = NAN;
    expect_throw("non-finite rest position", [&] { check(nan, 1, 512); });
    Mesh rep = lattice(4);
    rep.dist[1] = rep.dist[0];
    expect_throw("repeated particle", [&] { check(rep, 1, 512); });
    std::puts("SANITIZE OK");
    return 0;
}
