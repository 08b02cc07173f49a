// The host table builder (softbodyunity_amd/csrc/tables_host.cpp) on a plan the sanitizer drivers have just built: two shapes of
// options, so that the packed slot forms, the wave items, the split cost order and the mailbox layout all run under the sanitizers.
#pragma once
#include <stdexcept>
#include <vector>

#include "tables_host.hpp"

inline void san_tables(const sbp::Input &in, const sbp::Plan &P, const sbp::LocalPlan &L) {
    const size_t n = (size_t)in.n;
    std::vector<float> pos(in.rest, in.rest + 3 * n), vel(3 * n, 0.5f), invm(n), dist((size_t)in.m_d), vol((size_t)in.m_v, 0.25f), bend(2 * (size_t)in.m_b, 0.75f);
    for (int shape = 0; shape < 2; ++shape) {
        sbt::TableOptions opt;
        if (shape == 0) { opt.narrow_min_tiles = 4; opt.split_launches = true; }
        else { opt.quad_lanes = 256; opt.peer_enabled = L.world <= sbk::kMaxPeers + 1; opt.plan_hash = 0x0123456789abcdefull; opt.plan_shape = 7; }
        for (size_t p = 0; p < n; ++p) invm[p] = shape ? 1.0f + 0.001f * (float)(p % 1000) : 1.0f;
        for (size_t k = 0; k < dist.size(); ++k) dist[k] = shape ? 1.0f + 1e-5f * (float)k : 1.0f;
        const sbt::TableInput ti{&P, &L, pos.data(), vel.data(), invm.data(), dist.data(), vol.data(), bend.data(), in.m_v, in.m_b};
        sbt::HostTables H;
        sbt::build_tables(ti, opt, H);
        int64_t slots = 0;
        for (const sbt::HostTiling &T : H.T) {
            slots += T.n_slots;
            for (const sbk::TileDesc &td : T.tiles)
                if ((size_t)td.s_begin + td.s_len > T.stream.size()) throw std::runtime_error("a tile's program leaves the stream");
        }
        for (const sbt::HostGColour &G : H.gcolours) slots += G.count;
        if (L.world == 1 && slots != in.m_d + in.m_v + in.m_b) throw std::runtime_error("the tables do not hold every constraint once");
    }
}
