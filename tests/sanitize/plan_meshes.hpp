// Mesh generators shared by the planner's CPU drivers (plan_san.cpp: sanitizers; plan_digest.cpp: digests of whole plans).
// Everything here is integer or exactly rounded float arithmetic on std::mt19937 output, so a mesh is the same on every machine.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <random>
#include <vector>

#include "plan.hpp"

namespace meshes {

struct Mesh {
    std::vector<float> rest;
    std::vector<int32_t> dist, vol, bend;
    std::vector<int32_t> gid;       // a window of a larger mesh (cut_window): whole-mesh ids, ascending; else empty
    sbp::Input input() const {
        sbp::Input in{rest.data(), (int32_t)(rest.size() / 3), dist.data(), (int64_t)dist.size() / 2,
                      vol.data(), (int64_t)vol.size() / 4, bend.data(), (int64_t)bend.size() / 4};
        if (!gid.empty()) in.global_id = gid.data();
        return in;
    }
};

// n^3 lattice with the axis springs; full_stencil: springs to all 26 neighbours (13 per particle, each pair once)
inline Mesh lattice(int n, bool full_stencil = false) {
    Mesh m;
    for (int z = 0; z < n; ++z) for (int y = 0; y < n; ++y) for (int x = 0; x < n; ++x) { m.rest.push_back((float)x); m.rest.push_back((float)y); m.rest.push_back((float)z); }
    auto id = [n](int x, int y, int z) { return (z * n + y) * n + x; };
    for (int z = 0; z < n; ++z) for (int y = 0; y < n; ++y) for (int x = 0; x < n; ++x) {
        if (!full_stencil) {
            if (x + 1 < n) { m.dist.push_back(id(x, y, z)); m.dist.push_back(id(x + 1, y, z)); }
            if (y + 1 < n) { m.dist.push_back(id(x, y, z)); m.dist.push_back(id(x, y + 1, z)); }
            if (z + 1 < n) { m.dist.push_back(id(x, y, z)); m.dist.push_back(id(x, y, z + 1)); }
            continue;
        }
        for (int dz = 0; dz <= 1; ++dz) for (int dy = (dz ? -1 : 0); dy <= 1; ++dy) for (int dx = ((dz || dy) ? -1 : 1); dx <= 1; ++dx) {
            const int X = x + dx, Y = y + dy, Z = z + dz;
            if (X < 0 || X >= n || Y < 0 || Y >= n || Z >= n) continue;
            m.dist.push_back(id(x, y, z)); m.dist.push_back(id(X, Y, Z));
        }
    }
    return m;
}

inline Mesh cloud(int n, unsigned seed) {     // jittered points, each joined to a few near neighbours by index proximity
    Mesh m;
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    const int side = (int)std::ceil(std::cbrt((double)n));
    for (int p = 0; p < n; ++p) {
        int x = p % side, y = (p / side) % side, z = p / (side * side);
        m.rest.push_back(x + 0.6f * u(rng)); m.rest.push_back(y + 0.6f * u(rng)); m.rest.push_back(z + 0.6f * u(rng));
    }
    auto ok = [n](int q) { return q >= 0 && q < n; };
    for (int p = 0; p < n; ++p) {
        const int nb[5] = {p + 1, p + side, p + side * side, p + side + 1, p - side + 1};
        for (int q : nb) if (ok(q) && q != p) { m.dist.push_back(p); m.dist.push_back(q); }
        if (ok(p + 1) && ok(p + side) && ok(p + side * side)) {
            m.vol.push_back(p); m.vol.push_back(p + 1); m.vol.push_back(p + side); m.vol.push_back(p + side * side);
            if (p % 3 == 0) { m.bend.push_back(p); m.bend.push_back(p + 1); m.bend.push_back(p + side); m.bend.push_back(p + side * side); }
        }
    }
    return m;
}

// An L-shaped part of the cloud (three quarters of the box empty in one corner region): fill < 0.8, so the fill-aware grid, the
// balanced extra lists and the tile merge of plan.cpp run; automatic partition => RCB.
inline Mesh l_shape(const Mesh &full) {
    const int32_t n = (int32_t)(full.rest.size() / 3);
    float hi[3] = {0, 0, 0};
    for (int32_t p = 0; p < n; ++p) for (int a = 0; a < 3; ++a) hi[a] = std::max(hi[a], full.rest[3 * p + a]);
    std::vector<int32_t> map((size_t)n, -1);
    Mesh m;
    for (int32_t p = 0; p < n; ++p) {
        const float *x = &full.rest[3 * (size_t)p];
        if (x[0] > 0.45f * hi[0] && x[1] > 0.45f * hi[1]) continue;         // cut a column out
        map[(size_t)p] = (int32_t)(m.rest.size() / 3);
        m.rest.insert(m.rest.end(), x, x + 3);
    }
    auto keep = [&](const std::vector<int32_t> &src, int nv, std::vector<int32_t> &dst) {
        for (size_t k = 0; k + nv <= src.size(); k += nv) {
            bool ok = true;
            for (int a = 0; a < nv; ++a) ok &= map[(size_t)src[k + a]] >= 0;
            if (ok) for (int a = 0; a < nv; ++a) dst.push_back(map[(size_t)src[k + a]]);
        }
    };
    keep(full.dist, 2, m.dist); keep(full.vol, 4, m.vol); keep(full.bend, 4, m.bend);
    return m;
}

// One hub particle joined to every one of n_sat satellites in a shell around it, + a ring through the satellites: the hub needs
// n_sat colours (plan.cpp greedy_colour_wide once n_sat > 128).
inline Mesh hub(int n_sat, unsigned seed) {
    Mesh m;
    m.rest = {0.f, 0.f, 0.f};
    std::mt19937 rng(seed);
    auto unit = [&] { return (float)(int32_t)(rng() >> 8) * (1.0f / 8388608.0f) - 1.0f; };       // [-1, 1), exact
    while ((int)(m.rest.size() / 3) < 1 + n_sat) {
        const float x = unit(), y = unit(), z = unit(), r2 = x * x + y * y + z * z;
        if (r2 < 0.64f || r2 > 1.44f) continue;
        m.rest.push_back(x); m.rest.push_back(y); m.rest.push_back(z);
    }
    for (int k = 0; k < n_sat; ++k) { m.dist.push_back(0); m.dist.push_back(1 + k); }
    for (int k = 0; k < n_sat; ++k) { m.dist.push_back(1 + k); m.dist.push_back(1 + (k + 1) % n_sat); }
    return m;
}

// Eight small lattices at the corners of a box `gap` lattice spacings wide: nearly every cell of the planner's grid is empty
// (n_cells > 8 n + 4096), which takes the comparison sorts of T0, T1 and the RCB partition instead of the counting sorts.
inline Mesh sparse_clusters(int side, int gap) {
    const Mesh one = lattice(side);
    const int32_t n1 = (int32_t)(one.rest.size() / 3);
    Mesh m;
    for (int c = 0; c < 8; ++c) {
        const float off[3] = {(float)((c & 1) * gap), (float)(((c >> 1) & 1) * gap), (float)(((c >> 2) & 1) * gap)};
        for (int32_t p = 0; p < n1; ++p) for (int a = 0; a < 3; ++a) m.rest.push_back(one.rest[3 * (size_t)p + a] + off[a]);
        for (int32_t v : one.dist) m.dist.push_back(v + c * n1);
    }
    return m;
}

// The window of `m` (distance constraints only) that o.rank of a sharded solver plans: the particles inside rank_window()'s box.
inline Mesh cut_window(const Mesh &m, const sbp::Domain &dom, const sbp::Opts &o) {
    const int32_t n = (int32_t)(m.rest.size() / 3);
    int clo[3], chi[3]; double blo[3], bhi[3];
    sbp::rank_window(dom, o, clo, chi, blo, bhi);
    std::vector<int32_t> map((size_t)n, -1);
    Mesh w;
    for (int32_t p = 0; p < n; ++p) {
        bool in = true;
        for (int a = 0; a < 3; ++a) in &= m.rest[3 * (size_t)p + a] >= blo[a] && m.rest[3 * (size_t)p + a] < bhi[a];
        if (!in) continue;
        map[(size_t)p] = (int32_t)w.gid.size(); w.gid.push_back(p);
        w.rest.insert(w.rest.end(), &m.rest[3 * (size_t)p], &m.rest[3 * (size_t)p] + 3);
    }
    for (size_t k = 0; k + 2 <= m.dist.size(); k += 2)
        if (map[(size_t)m.dist[k]] >= 0 && map[(size_t)m.dist[k + 1]] >= 0) { w.dist.push_back(map[(size_t)m.dist[k]]); w.dist.push_back(map[(size_t)m.dist[k + 1]]); }
    return w;
}

}  // namespace meshes
