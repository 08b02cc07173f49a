// impulse.hip — impulses between two ticks (sb_apply_impulses, SPEC.md 2c): validation, the host-side expansion of SURFACE items, the
// sort of sparse entries into per-particle runs, and the launches (the tables travel in a TableRing, device_handles.hpp). The group's entry point (group.hip) shares the
// validation, the expansion and the rank path.
//
// No reference counterpart exists (/root/reference/README.md:1 is the whole reference tree); the exported function is part of the
// [BUILDER-DEFINED] boundary of SURVEY.md §8b (include/softbody.h).
#include "solver_internal.hpp"
#include "impulse_kernels.hip.hpp"

using namespace sbi;

namespace sbi {

static bool finite(float f) { return std::isfinite(f); }

int64_t impulse_triangles_in_force(const RenderState &R) {
    if (R.emb.m > 0) return R.emb.tri.empty() ? -1 : (int64_t)(R.emb.tri.size() / 3);
    return R.tri.empty() ? -1 : (int64_t)(R.tri.size() / 3);
}

// The whole list, before anything is applied (SPEC.md 2c, "Errors"). n: particles of the caller's numbering; m_tri: triangles of the
// render mode in force, -1 = none; rank: a rank of a partitioned solver, which takes no SURFACE item.
int validate_impulses(const char *who, const sb_impulse *items, int32_t count, int32_t n, int64_t m_tri, bool rank) {
    const std::string W = who;
    for (int32_t i = 0; i < count; ++i) {
        const sb_impulse &it = items[i];
        const std::string at = W + ": item " + std::to_string(i) + ": ";
        if (it.kind != SB_IMPULSE_PARTICLE && it.kind != SB_IMPULSE_SURFACE && it.kind != SB_IMPULSE_RADIAL) return fail(SB_ERR_INVALID_ARG, at + "unknown kind");
        if (it.flags & ~(uint32_t)(SB_IMPULSE_VELOCITY_CHANGE | SB_IMPULSE_LINEAR_FALLOFF)) return fail(SB_ERR_INVALID_ARG, at + "unknown flag bit");
        if ((it.flags & SB_IMPULSE_LINEAR_FALLOFF) && it.kind != SB_IMPULSE_RADIAL) return fail(SB_ERR_INVALID_ARG, at + "SB_IMPULSE_LINEAR_FALLOFF on a non-radial item");
        if (it.reserved[0] != 0 || it.reserved[1] != 0) return fail(SB_ERR_INVALID_ARG, at + "reserved must be 0");
        if (it.kind == SB_IMPULSE_PARTICLE) {
            if (it.index < 0 || it.index >= n) return fail(SB_ERR_INVALID_ARG, at + "particle index out of range");
        } else if (it.kind == SB_IMPULSE_SURFACE) {
            if (rank) return fail(SB_ERR_UNSUPPORTED, at + "a SURFACE item on a rank of a partitioned solver (world > 1): its triangles' particles may belong to other ranks (sb_group_apply_impulses serves that case)");
            if (m_tri < 0) return fail(SB_ERR_STATE, at + "a SURFACE item while no triangle list is in force (neither render triangles, nor an embedding with m_tri > 0)");
            if (it.index < -1 || it.index >= m_tri) return fail(SB_ERR_INVALID_ARG, at + "triangle index out of range");
            if (it.index >= 0 && (!finite(it.u) || !finite(it.v))) return fail(SB_ERR_INVALID_ARG, at + "NaN or infinite barycentric coordinate");
        } else {
            if (!(it.radius > 0.0f)) return fail(SB_ERR_INVALID_ARG, at + "radius must be positive (+inf is allowed)");
            if (!finite(it.strength)) return fail(SB_ERR_INVALID_ARG, at + "NaN or infinite strength");
        }
        for (int c = 0; c < 3; ++c) if (!finite(it.vec[c])) return fail(SB_ERR_INVALID_ARG, at + "NaN or infinite vec");
    }
    return SB_OK;
}

// A validated list with its SURFACE items expanded into PARTICLE-like entries (p, G), in SPEC.md 2c's order: what the rank path takes.
// A G is used as computed (it may have overflowed; the rank path does not look at it again).
void expand_impulses(const RenderState &R, const sb_impulse *items, int32_t count, std::vector<sb_impulse> &out) {
    out.clear();
    out.reserve((size_t)count);
    const bool embedded = R.emb.m > 0;
    const std::vector<int32_t> &tri = embedded ? R.emb.tri : R.tri;
    for (int32_t i = 0; i < count; ++i) {
        const sb_impulse &it = items[i];
        if (it.kind != SB_IMPULSE_SURFACE) { out.push_back(it); continue; }
        if (it.index < 0) continue;
        const float t0 = 1.0f - it.u;
        const float b[3] = {t0 - it.v, it.u, it.v};
        sb_impulse e{};
        e.kind = SB_IMPULSE_PARTICLE;
        e.flags = it.flags & SB_IMPULSE_VELOCITY_CHANGE;
        for (int q = 0; q < 3; ++q) {
            const int32_t r = tri[3 * (size_t)it.index + q];
            if (!embedded) {
                e.index = r;
                for (int c = 0; c < 3; ++c) e.vec[c] = b[q] * it.vec[c];
                out.push_back(e);
                continue;
            }
            for (int k = 0; k < 4; ++k) {
                e.index = R.emb.cage[4 * (size_t)r + k];
                const float bw = b[q] * R.emb.w[4 * (size_t)r + k];
                for (int c = 0; c < 3; ++c) e.vec[c] = bw * it.vec[c];
                out.push_back(e);
            }
        }
    }
}

namespace {

// The tables of one sparse run inside a call's table: [particle per lane][offsets, one more][pad to 16 bytes][float4 entries]
struct SparseRun {
    int32_t begin = 0, end = 0;                          // the run's items in the list
    std::vector<std::pair<int32_t, int32_t>> mine;       // (device particle, position in the list) of the entries this rank owns, sorted
    size_t n_lanes = 0, head = 0, at = 0;                // distinct particles; bytes in front of the entries; where the run starts in the table
    size_t bytes() const { return head + mine.size() * sizeof(float4); }
};

// One run of PARTICLE entries: the ones this rank owns, sorted (stably) by device particle, one lane per distinct particle.
SparseRun sort_sparse(const sb_solver *s, const sb_impulse *items, int32_t begin, int32_t end, const std::vector<int32_t> &lof) {
    SparseRun R;
    R.begin = begin; R.end = end;
    for (int32_t i = begin; i < end; ++i) {
        const int32_t l = lof[(size_t)items[i].index];
        if (l >= 0 && l < s->n_owned) R.mine.emplace_back(l, i);
    }
    std::stable_sort(R.mine.begin(), R.mine.end(), [](const std::pair<int32_t, int32_t> &a, const std::pair<int32_t, int32_t> &b) { return a.first < b.first; });
    for (size_t k = 0; k < R.mine.size(); ++k) R.n_lanes += k == 0 || R.mine[k].first != R.mine[k - 1].first;
    R.head = ((2 * R.n_lanes + 1) * sizeof(int32_t) + 15) / 16 * 16;
    return R;
}

void fill_sparse(const SparseRun &R, const sb_impulse *items, char *h) {
    int32_t *part = (int32_t *)h, *off = part + R.n_lanes;
    float4 *entries = (float4 *)(h + R.head);
    size_t r = 0;
    for (size_t k = 0; k < R.mine.size(); ++k) {
        if (k == 0 || R.mine[k].first != R.mine[k - 1].first) { part[r] = R.mine[k].first; off[r] = (int32_t)k; ++r; }
        const sb_impulse &it = items[R.mine[k].second];
        const uint32_t vc = (it.flags & SB_IMPULSE_VELOCITY_CHANGE) ? 1u : 0u;
        float wbits; std::memcpy(&wbits, &vc, sizeof(wbits));
        entries[k] = make_float4(it.vec[0], it.vec[1], it.vec[2], wbits);
    }
    off[R.n_lanes] = (int32_t)R.mine.size();
}

void launch_sparse(sb_solver *s, const SparseRun &R, const char *d) {
    hipLaunchKernelGGL(sbk::impulse_sparse_kernel, dim3((unsigned)((R.n_lanes + 255) / 256)), dim3(256), 0, s->stream, s->pos_view(), s->d_vel.p,
                       (const int32_t *)d, (const int32_t *)d + R.n_lanes, (const float4 *)(d + R.head), (int)R.n_lanes);
    HIP_CHECK(hipGetLastError());
}

// One run of RADIAL items: passes over the owned particles, up to kRadialBatch consecutive items each.
void launch_radial(sb_solver *s, const sb_impulse *items, int32_t count) {
    if (s->n_owned == 0) return;
    for (int32_t b = 0; b < count; b += sbk::kRadialBatch) {
        sbk::RadialBatch B{};
        B.count = std::min<int32_t>(sbk::kRadialBatch, count - b);
        for (int i = 0; i < B.count; ++i) {
            const sb_impulse &it = items[b + i];
            sbk::RadialItem &I = B.item[i];
            I.cx = it.vec[0]; I.cy = it.vec[1]; I.cz = it.vec[2];
            I.radius = it.radius; I.r2max = it.radius * it.radius;
            I.strength = it.strength; I.flags = it.flags;
        }
        hipLaunchKernelGGL(sbk::impulse_radial_kernel, dim3((unsigned)((s->n_owned + 255) / 256)), dim3(256), 0, s->stream, s->pos_view(), s->d_vel.p,
                           (int64_t)s->n_owned, B);
        HIP_CHECK(hipGetLastError());
    }
}

}  // namespace

// The rank path: a validated list of PARTICLE and RADIAL items in the rank's numbering (SURFACE items already expanded), applied to the
// particles this rank owns. Completes the tick first -- velocities exist only once its last kernel has run -- which also lands pending
// kinematic targets, on every rank alike (an empty list too: the ranks of a group stay in the same tick state).
int apply_impulses_validated(sb_solver *s, const sb_impulse *items, int32_t count) {
    int rc = set_device(s); if (rc) return rc;
    const std::vector<int32_t> &lof = local_of_old(s);
    // the sparse runs' tables first, side by side in ONE table of the ring with one event behind the call's last sparse kernel: however
    // many runs a call has, it waits for nothing of its own
    std::vector<SparseRun> sparse;
    size_t bytes = 0;
    for (int32_t i = 0; i < count;) {
        int32_t j = i;
        const bool radial = items[i].kind == SB_IMPULSE_RADIAL;
        while (j < count && (items[j].kind == SB_IMPULSE_RADIAL) == radial) ++j;
        if (!radial) {
            sparse.push_back(sort_sparse(s, items, i, j, lof));
            sparse.back().at = bytes;
            if (!sparse.back().mine.empty()) bytes += sparse.back().bytes();       // (a multiple of 16)
        }
        i = j;
    }
    int q = -1;
    if (bytes) {
        q = s->imp_ring.acquire(bytes);
        char *h = s->imp_ring.host(q);
        for (const SparseRun &R : sparse) if (!R.mine.empty()) fill_sparse(R, items, h + R.at);
    }
    flush_deferred(s);
    size_t next_sparse = 0;
    for (int32_t i = 0; i < count;) {
        int32_t j = i;
        const bool radial = items[i].kind == SB_IMPULSE_RADIAL;
        while (j < count && (items[j].kind == SB_IMPULSE_RADIAL) == radial) ++j;
        if (radial) launch_radial(s, items + i, j - i);
        else {
            const SparseRun &R = sparse[next_sparse++];
            if (!R.mine.empty()) launch_sparse(s, R, s->imp_ring.device(q) + R.at);
        }
        i = j;
    }
    if (q >= 0) s->imp_ring.retire(q, s->stream);
    return SB_OK;
}

}  // namespace sbi

extern "C" {

int sb_apply_impulses(sb_solver *s, const sb_impulse *items, int32_t count) {
    if (!s || count < 0 || (count > 0 && !items)) return fail(SB_ERR_INVALID_ARG, "sb_apply_impulses: bad argument (null handle, null items or negative count)");
    if (!s->finalized) return fail(SB_ERR_STATE, "sb_apply_impulses before sb_finalize");
    if (count == 0) return SB_OK;
    return guarded([&]() -> int {
        const bool rank = s->desc.world > 1;
        if (int rc = validate_impulses("sb_apply_impulses", items, count, s->mesh->n, rank ? -1 : impulse_triangles_in_force(s->render), rank)) return rc;
        bool surface = false;
        for (int32_t i = 0; i < count && !surface; ++i) surface = items[i].kind == SB_IMPULSE_SURFACE;
        if (!surface) return apply_impulses_validated(s, items, count);
        std::vector<sb_impulse> flat;
        expand_impulses(s->render, items, count, flat);
        return apply_impulses_validated(s, flat.data(), (int32_t)flat.size());
    });
}

}  // extern "C"
