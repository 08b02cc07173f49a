// authoring.cpp — see authoring.hpp. Host only.
//
// No reference counterpart exists (/root/reference/README.md:1 is the whole reference tree).
#include "authoring.hpp"

#include <atomic>

namespace sbi {

static Status bad(int code, const char *who, const char *what) { return Status{code, std::string(who) + what}; }

Status AuthoredMesh::set_particles(const char *who, const float *pos_xyz, const float *vel_xyz, const float *inv_mass, int32_t count) {
    if (!pos_xyz || !inv_mass || count <= 0) return bad(SB_ERR_INVALID_ARG, who, ": bad argument");
    for (int32_t p = 0; p < count; ++p) if (!(inv_mass[p] >= 0.0f)) return bad(SB_ERR_INVALID_ARG, who, ": inverse mass must be >= 0");
    n = count;
    pos.assign(pos_xyz, pos_xyz + 3 * (size_t)count);
    if (vel_xyz) vel.assign(vel_xyz, vel_xyz + 3 * (size_t)count); else vel.assign(3 * (size_t)count, 0.0f);
    invm.assign(inv_mass, inv_mass + count);
    return {};
}

Status AuthoredMesh::set_rest_positions(const char *who, const float *rest_xyz, int32_t count) {
    if (group) {
        if (!rest_xyz || count != n) return bad(SB_ERR_INVALID_ARG, who, ": bad argument (n differs from sb_group_set_particles?)");
    } else {
        if (!rest_xyz) return bad(SB_ERR_INVALID_ARG, who, ": bad argument");
        if (count != n) return bad(SB_ERR_INVALID_ARG, who, ": n differs from sb_set_particles");
    }
    rest.assign(rest_xyz, rest_xyz + 3 * (size_t)count);
    return {};
}

Status AuthoredMesh::set_constraints(int t, const char *who, const int32_t *idx, const float *rest_values, int32_t m, float compliance) {
    const int nv = kKinds[t].nv, nrest = kKinds[t].nrest;
    if (m < 0 || (m > 0 && (!idx || !rest_values))) return bad(SB_ERR_INVALID_ARG, who, ": bad argument");
    if (n <= 0) return bad(SB_ERR_STATE, who, group ? " before sb_group_set_particles" : " before sb_set_particles");
    if (!(compliance >= 0.0f)) return bad(SB_ERR_INVALID_ARG, who, ": compliance must be >= 0");
    std::atomic<bool> out_of_range{false};
    sbp::parallel_for_chunks((int64_t)m * nv, 1 << 22, [&](int64_t, int64_t kb, int64_t ke) {
        for (int64_t k = kb; k < ke; ++k) if (idx[k] < 0 || idx[k] >= n) { out_of_range = true; return; }
    });
    if (out_of_range) return bad(SB_ERR_INVALID_ARG, who, ": particle index out of range");
    kind[t].idx.assign(idx, idx + (size_t)m * nv);
    kind[t].rest.assign(rest_values, rest_values + (size_t)m * nrest);
    kind[t].compliance = compliance;
    return {};
}

Status AuthoredMesh::set_ground_plane(const char *who, float nx, float ny, float nz, float d, int32_t enabled) {
    if (!(nx == nx) || !(ny == ny) || !(nz == nz) || !(d == d)) return bad(SB_ERR_INVALID_ARG, who, ": NaN");
    plane[0] = nx; plane[1] = ny; plane[2] = nz; plane[3] = d;
    plane_on = enabled ? 1 : 0;
    return {};
}

void AuthoredMesh::release_bulk() {
    for (std::vector<float> *v : {&pos, &vel, &rest}) std::vector<float>().swap(*v);
    for (Constraints &c : kind) { std::vector<int32_t>().swap(c.idx); std::vector<float>().swap(c.rest); }
}

AuthoredMesh AuthoredMesh::without_bulk() const {
    AuthoredMesh k;
    k.n = n; k.invm = invm; k.plane_on = plane_on;
    for (int t = 0; t < 3; ++t) k.kind[t].compliance = kind[t].compliance;
    for (int a = 0; a < 4; ++a) k.plane[a] = plane[a];
    return k;
}

sbp::Input make_input(const AuthoredMesh &m) {
    return sbp::Input{m.rest_or_pos().data(), m.n, m.kind[0].idx.data(), m.count(0), m.kind[1].idx.data(), m.count(1), m.kind[2].idx.data(), m.count(2)};
}

Window cut_window(const AuthoredMesh &whole, const double lo[3], const double hi[3]) {
    Window w;
    AuthoredMesh &m = w.mesh;
    const std::vector<float> &rp = whole.rest_or_pos();
    std::vector<int32_t> new_of((size_t)whole.n, -1);
    for (int32_t p = 0; p < whole.n; ++p) {
        bool in = true;
        for (int a = 0; a < 3; ++a) { const double c = (double)rp[3 * (size_t)p + a]; in = in && c >= lo[a] && c < hi[a]; }
        if (in) { new_of[(size_t)p] = (int32_t)w.gid.size(); w.gid.push_back(p); }
    }
    const size_t nw = w.gid.size();
    m.n = (int32_t)nw;
    m.pos.resize(3 * nw); m.vel.resize(3 * nw); m.invm.resize(nw);
    if (!whole.rest.empty()) m.rest.resize(3 * nw);
    for (size_t k = 0; k < nw; ++k) {
        const size_t p = (size_t)w.gid[k];
        for (int c = 0; c < 3; ++c) {
            m.pos[3 * k + c] = whole.pos[3 * p + c]; m.vel[3 * k + c] = whole.vel[3 * p + c];
            if (!whole.rest.empty()) m.rest[3 * k + c] = whole.rest[3 * p + c];
        }
        m.invm[k] = whole.invm[p];
    }
    for (int t = 0; t < 3; ++t) {
        const AuthoredMesh::Constraints &from = whole.kind[t];
        AuthoredMesh::Constraints &to = m.kind[t];
        const int nv = kKinds[t].nv, nr = kKinds[t].nrest;
        to.compliance = from.compliance;
        for (int64_t k = 0; k < whole.count(t); ++k) {
            bool in = true;
            for (int q = 0; q < nv; ++q) in = in && new_of[(size_t)from.idx[(size_t)(nv * k + q)]] >= 0;
            if (!in) continue;
            for (int q = 0; q < nv; ++q) to.idx.push_back(new_of[(size_t)from.idx[(size_t)(nv * k + q)]]);
            for (int q = 0; q < nr; ++q) to.rest.push_back(from.rest[(size_t)(nr * k + q)]);
        }
    }
    for (int a = 0; a < 4; ++a) m.plane[a] = whole.plane[a];
    m.plane_on = whole.plane_on;
    return w;
}

}  // namespace sbi
