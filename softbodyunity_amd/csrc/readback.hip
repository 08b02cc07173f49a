// readback.hip — state reads and writes, kinematic targets, the asynchronous render readback with GPU vertex normals, tangents, embedded render vertices and the bounding box
//
// No reference counterpart exists (/root/reference/README.md:1 is the whole reference tree); the exported functions are the
// [BUILDER-DEFINED] boundary of SURVEY.md §8b (include/softbody*.h).
#include "solver_internal.hpp"
#include "readback_kernels.hip.hpp"

using namespace sbi;

namespace sbi {

// Owned particle l of a rank -> its index in the array a read is delivered in: the rank's own numbering (the caller's, or its window's
// under sharded authoring), or -- for a group that gathers several ranks into one array -- the whole mesh's (id_map[window index]).
static void scatter_owned(const sb_solver *s, const float *staged, float *out, const int32_t *id_map) {
    const sbp::LocalPlan &L = s->plan->local;
    sbp::parallel_for_chunks(s->n_owned, 1 << 18, [&](int64_t, int64_t lb, int64_t le) {     // owned particles have distinct caller ids
        for (int64_t l = lb; l < le; ++l) {
            int32_t o = L.local_to_old[l];
            if (id_map) o = id_map[o];
            for (int c = 0; c < 3; ++c) out[3 * (size_t)o + c] = staged[3 * (size_t)l + c];
        }
    });
}

// Positions (or velocities) of the particles this rank OWNS, written into `out` at their caller index (id_map: see scatter_owned);
// entries of other ranks' particles are left alone. Position reads PEEK while the tick's last kernel is held back (the tick stays
// fusable with the next one), on every rank of a partitioned solver too: the held-back kernel runs on T0 tiles, which hold owned
// particles only and need no ghost.
int get_state_owned(sb_solver *s, float *out, bool velocity, const int32_t *id_map) {
    int rc = set_device(s); if (rc) return rc;
    const bool peek = !velocity && can_peek(s);
    if (peek) { peek_positions(s, false); if (s->kin_pending >= 0) scatter_kinematic(s, s->d_peek.p); }     // (pending targets show in what is read; they stay pending)
    else flush_deferred(s);
    HIP_CHECK(hipStreamSynchronize(s->stream));
    check_peer_error(s);
    s->h_stage.resize((size_t)s->n_owned * 3);
    const float *src = velocity ? s->d_vel.p : (peek ? s->d_peek.p : s->d_pos3.p);
    if (s->n_owned) HIP_CHECK(hipMemcpy(s->h_stage.data(), src, (size_t)s->n_owned * 3 * sizeof(float), hipMemcpyDeviceToHost));
    scatter_owned(s, s->h_stage.data(), out, id_map);
    return SB_OK;
}

}  // namespace sbi

static int get_state(sb_solver *s, float *out, int32_t n, bool velocity) {
    if (!s || !out) return fail(SB_ERR_INVALID_ARG, "sb_get_*: null argument");
    if (!s->finalized) return fail(SB_ERR_STATE, "sb_get_* before sb_finalize");
    if (n != s->n) return fail(SB_ERR_INVALID_ARG, "sb_get_*: n differs from sb_set_particles");
    return guarded([&]() -> int {
        if (s->desc.world != 1) return get_state_owned(s, out, velocity, nullptr);       // only the entries this rank owns (the caller merges the ranks' arrays)
        int rc = set_device(s); if (rc) return rc;
        const sbp::LocalPlan &L = s->plan->local;
        // positions while the tick's last kernel is deferred: peek instead of completing the tick (the next sb_step keeps its fusion)
        const bool peek = !velocity && can_peek(s);
        if (peek) { peek_positions(s, false); if (s->kin_pending >= 0) scatter_kinematic(s, s->d_peek.p); }     // (pending targets show in what is read; they stay pending)
        else flush_deferred(s);
        // single rank: every entry is ours, so the permutation to caller numbering runs on the GPU and one copy
        // lands in the caller's array (a host-side scatter costs 25 ms for 16.7 M particles)
        if (!s->d_local_to_old.p) s->d_local_to_old.upload(L.local_to_old, s->dev_bytes);
        if (!s->d_get_scratch.p) s->d_get_scratch.alloc((size_t)s->n * 3, s->dev_bytes);
        sbk::PosView src = s->pos_view();
        if (peek) src.xyz = s->d_peek.p;
        if (velocity) src.xyz = s->d_vel.p;
        hipLaunchKernelGGL(sbk::snapshot_kernel, dim3((unsigned)((s->n_owned + 255) / 256)), dim3(256), 0, s->stream, src,
                           s->d_local_to_old.p, s->d_get_scratch.p, (int)s->n_owned);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(out, s->d_get_scratch.p, (size_t)s->n * 3 * sizeof(float), hipMemcpyDeviceToHost, s->stream));
        HIP_CHECK(hipStreamSynchronize(s->stream));
        return SB_OK;
    });
}

extern "C" {

int sb_get_positions(sb_solver *s, float *out, int32_t n) { return get_state(s, out, n, false); }
int sb_get_velocities(sb_solver *s, float *out, int32_t n) { return get_state(s, out, n, true); }

}  // extern "C"

namespace sbi {

// The rank's numbering (caller's, or its window's) -> device numbering, -1 for a particle this rank does not hold; built at first use.
const std::vector<int32_t> &local_of_old(sb_solver *s) {
    if (s->local_of_old.empty()) {
        const sbp::LocalPlan &L = s->plan->local;
        s->local_of_old.assign((size_t)s->n, -1);
        for (size_t l = 0; l < L.local_to_old.size(); ++l) s->local_of_old[(size_t)L.local_to_old[l]] = (int32_t)l;
    }
    return s->local_of_old;
}

// Where a render snapshot of this rank reads the tick-end positions from, made valid on the solver's stream: while the tick's last kernel
// is held back that is a PEEK into the side array (compact: only the T0 tiles that hold a particle of `wanted_local`; the subset is built
// once per render set), else the state itself after the tick has been completed. Pending kinematic targets show in a peek.
const float *render_source(sb_solver *s, bool compact, const std::vector<int32_t> &wanted_local) {
    if (!can_peek(s)) { flush_deferred(s); return s->d_pos3.p; }
    if (compact && s->n_peek_tiles < 0) build_peek_subset(s, wanted_local);
    peek_positions(s, compact);
    if (s->kin_pending >= 0) scatter_kinematic(s, s->d_peek.p);
    return s->d_peek.p;
}

// Launch helpers for a host that gathers several ranks' snapshots on one device (group.hip): dst may live on another device.
void launch_snapshot_all(sb_solver *s, const float *src_xyz, const int32_t *d_target_of_local, float *dst_xyz) {
    if (!s->n_owned) return;
    sbk::PosView src = s->pos_view();
    src.xyz = const_cast<float *>(src_xyz);
    hipLaunchKernelGGL(sbk::snapshot_kernel, dim3((unsigned)((s->n_owned + 255) / 256)), dim3(256), 0, s->stream, src, d_target_of_local, dst_xyz, (int)s->n_owned);
    HIP_CHECK(hipGetLastError());
}
void launch_snapshot_subset(sb_solver *s, const float *src_xyz, const int32_t *d_ids, const int32_t *d_local, int count, float *dst_xyz) {
    if (count <= 0) return;
    sbk::PosView src = s->pos_view();
    src.xyz = const_cast<float *>(src_xyz);
    hipLaunchKernelGGL(sbk::snapshot_subset_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s->stream, src, d_ids, d_local, dst_xyz, count);
    HIP_CHECK(hipGetLastError());
}
void launch_normals(hipStream_t st, const float *snap_xyz, const int32_t *adj_off, const int32_t *adj_tri, const int32_t *tri, float *nrm_xyz, int count,
                    const int32_t *subset, float *subset_pos_xyz) {
    if (count <= 0) return;
    hipLaunchKernelGGL(sbk::normals_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, snap_xyz, adj_off, adj_tri, tri, nrm_xyz, count, subset, subset_pos_xyz);
    HIP_CHECK(hipGetLastError());
}
void launch_normals_tangents(hipStream_t st, const float *snap_xyz, const int32_t *adj_off, const int32_t *adj_tri, const int32_t *tri, const float4 *tri_k,
                             float *nrm_xyz, float4 *tan_xyzw, int count, const int32_t *subset, float *subset_pos_xyz) {
    if (count <= 0) return;
    hipLaunchKernelGGL(sbk::normals_tangents_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, snap_xyz, adj_off, adj_tri, tri, tri_k, nrm_xyz, tan_xyzw,
                       count, subset, subset_pos_xyz);
    HIP_CHECK(hipGetLastError());
}

void launch_skin(hipStream_t st, const float *src_xyz, const int4 *cage, const float4 *weights, float *out_xyz, int m) {
    if (m <= 0) return;
    hipLaunchKernelGGL(sbk::skin_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, src_xyz, cage, weights, out_xyz, m);
    HIP_CHECK(hipGetLastError());
}

void ReadbackBounds::prepare(int64_t &acct) {
    if (h_box) return;
    d_partials.alloc((size_t)2 * 6 * sbk::kBoundsMaxGroups, acct);
    d_box.alloc((size_t)8 * (kSlots + 1), acct);
    HIP_CHECK(hipHostMalloc((void **)&h_box, (size_t)8 * (kSlots + 1) * sizeof(float), hipHostMallocDefault));
}

void launch_bounds(hipStream_t st, ReadbackBounds &B, int slot, const float *xyz, const int32_t *rows, int64_t count, int64_t &acct) {
    B.prepare(acct);
    float *partials = B.d_partials.p + (slot == ReadbackBounds::kQuerySlot ? (size_t)6 * sbk::kBoundsMaxGroups : 0);
    const int groups = (int)std::min<int64_t>((count + sbk::kBoundsLanes - 1) / sbk::kBoundsLanes, sbk::kBoundsMaxGroups);
    if (groups) hipLaunchKernelGGL(sbk::bounds_partial_kernel, dim3((unsigned)groups), dim3(sbk::kBoundsLanes), 0, st, xyz, rows, (int)count, partials);
    hipLaunchKernelGGL(sbk::bounds_final_kernel, dim3(1), dim3(sbk::kBoundsLanes), 0, st, partials, groups, B.d_box.p + 8 * (size_t)slot);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(B.h_box + 8 * (size_t)slot, B.d_box.p + 8 * (size_t)slot, 8 * sizeof(float), hipMemcpyDeviceToHost, st));
}

int get_bounds_owned(sb_solver *s, float lo[3], float hi[3]) {
    int rc = set_device(s); if (rc) return rc;
    const bool peek = can_peek(s);
    if (peek) { peek_positions(s, false); if (s->kin_pending >= 0) scatter_kinematic(s, s->d_peek.p); }     // (as get_state_owned reads positions)
    else flush_deferred(s);
    launch_bounds(s->stream, s->bnd, ReadbackBounds::kQuerySlot, peek ? s->d_peek.p : s->d_pos3.p, nullptr, s->n_owned, s->dev_bytes);
    HIP_CHECK(hipStreamSynchronize(s->stream));
    check_peer_error(s);
    s->bnd.read(ReadbackBounds::kQuerySlot, lo, hi);
    return SB_OK;
}

int check_embedding_args(const char *who, int32_t n, const int32_t *cage, const float *w, int32_t m, const int32_t *tri, int32_t m_tri) {
    const std::string me(who);
    if (m < 0 || m_tri < 0) return fail(SB_ERR_INVALID_ARG, me + ": negative count");
    if ((m > 0 && (!cage || !w)) || (m_tri > 0 && !tri)) return fail(SB_ERR_INVALID_ARG, me + ": null pointer with a positive count");
    for (int64_t c = 0; c < 4 * (int64_t)m; ++c) {
        if (cage[c] < 0 || cage[c] >= n) return fail(SB_ERR_INVALID_ARG, me + ": cage particle index out of range (render vertex " + std::to_string(c / 4) + ")");
        if (!std::isfinite(w[c])) return fail(SB_ERR_INVALID_ARG, me + ": weight is NaN or infinite (render vertex " + std::to_string(c / 4) + ")");
    }
    for (int64_t c = 0; c < 3 * (int64_t)m_tri; ++c)
        if (tri[c] < 0 || tri[c] >= m) return fail(SB_ERR_INVALID_ARG, me + ": triangle index out of range (triangles index render vertices)");
    return SB_OK;
}

// SPEC.md 6c, static part. Host code of a unit built with contraction off: two rounded products and one subtraction for det, four IEEE divisions.
void tangent_coefficients(const std::vector<float> &uv, const std::vector<int32_t> &tri, std::vector<float4> &k) {
    const size_t m = tri.size() / 3;
    k.resize(m);
    for (size_t t = 0; t < m; ++t) {
        const size_t a = 2 * (size_t)tri[3 * t], b = 2 * (size_t)tri[3 * t + 1], c = 2 * (size_t)tri[3 * t + 2];
        const float du1 = uv[b] - uv[a], dv1 = uv[b + 1] - uv[a + 1], du2 = uv[c] - uv[a], dv2 = uv[c + 1] - uv[a + 1];
        const float p0 = du1 * dv2, p1 = du2 * dv1;
        const float det = p0 - p1;
        const float k0 = dv2 / det, k1 = dv1 / det, k2 = du1 / det, k3 = du2 / det;
        const bool ok = det != 0.0f && std::isfinite(k0) && std::isfinite(k1) && std::isfinite(k2) && std::isfinite(k3);
        k[t] = ok ? make_float4(k0, k1, k2, k3) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);      // a UV-degenerate triangle contributes zeros
    }
}

void RenderTangents::prepare(const std::vector<int32_t> &tri, size_t n_rows, int64_t &acct) {
    if (dirty) {
        std::vector<float4> k;
        tangent_coefficients(uv, tri, k);
        d_k.upload(k, acct);
        dirty = false;
    }
    if (rows < n_rows || !h_tan[kSlots - 1]) {
        for (int q = 0; q < kSlots; ++q) {
            if (h_tan[q]) { (void)hipHostFree(h_tan[q]); h_tan[q] = nullptr; }
            d_tan[q].alloc(n_rows, acct);
            HIP_CHECK(hipHostMalloc((void **)&h_tan[q], std::max<size_t>(n_rows, 1) * sizeof(float4), hipHostMallocDefault));
        }
        rows = n_rows;
    }
}

int set_render_uvs(const char *who, RenderTangents &T, const float *uv, int32_t count, int64_t rows, bool readback_pending) {
    const std::string me(who);
    if (readback_pending) return fail(SB_ERR_STATE, me + " while a readback is pending");
    if (count == 0) { T.clear(); return SB_OK; }       // tangents off
    if (rows < 0) return fail(SB_ERR_STATE, me + ": no render mode with triangles is set (sb_set_render_triangles, or sb_set_render_embedding with m_tri > 0, comes first)");
    if (count < 0 || !uv) return fail(SB_ERR_INVALID_ARG, me + ": bad argument");
    if (count != rows)
        return fail(SB_ERR_INVALID_ARG, me + ": count is " + std::to_string(count) + ", the render mode in force has " + std::to_string(rows) + " vertices");
    for (int64_t c = 0; c < 2 * (int64_t)count; ++c)
        if (!std::isfinite(uv[c])) return fail(SB_ERR_INVALID_ARG, me + ": UV is NaN or infinite (vertex " + std::to_string(c / 2) + ")");
    T.uv.assign(uv, uv + 2 * (size_t)count);
    T.dirty = true;
    return SB_OK;
}

void build_adjacency(const std::vector<int32_t> &tri, int32_t n_vertices, std::vector<int32_t> &off, std::vector<int32_t> &adj) {
    const int64_t m = (int64_t)tri.size() / 3;
    off.assign((size_t)n_vertices + 1, 0); adj.resize((size_t)3 * m);
    for (int64_t c = 0; c < 3 * m; ++c) ++off[(size_t)tri[c] + 1];
    for (int32_t v = 0; v < n_vertices; ++v) off[(size_t)v + 1] += off[v];
    std::vector<int32_t> cur(off.begin(), off.end() - 1);
    for (int64_t t = 0; t < m; ++t)
        for (int j = 0; j < 3; ++j) adj[(size_t)cur[tri[3 * t + j]]++] = (int32_t)t;
}

// Replace positions and velocities of every particle this rank holds (owned and ghost); id_map as in get_state_owned.
int set_state_from(sb_solver *s, const float *pos, const float *vel, const int32_t *id_map) {
    int rc = set_device(s); if (rc) return rc;
    const sbp::LocalPlan &L = s->plan->local;
    flush_deferred(s);
    HIP_CHECK(hipStreamSynchronize(s->stream));
    std::vector<float> hp((size_t)s->n_local * 3), hv((size_t)s->n_local * 3);
    for (int64_t l = 0; l < s->n_local; ++l) {
        int32_t o = L.local_to_old[l];
        if (id_map) o = id_map[o];
        for (int c = 0; c < 3; ++c) { hp[3 * (size_t)l + c] = pos[3 * (size_t)o + c]; hv[3 * (size_t)l + c] = vel[3 * (size_t)o + c]; }
    }
    HIP_CHECK(hipMemcpy(s->d_pos3.p, hp.data(), hp.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(s->d_vel.p, hv.data(), hv.size() * sizeof(float), hipMemcpyHostToDevice));
    return SB_OK;
}

// Kinematic targets of the pinned particles THIS RANK OWNS among `count` entries (ids in the rank's numbering; an id this rank does not
// own is skipped: its owner applies it and the ghost copy arrives with the next exchange). Validation (range, inverse mass 0, no NaN, no
// id twice) covers every entry the rank can see. See sb_set_kinematic_positions.
int set_kinematic(sb_solver *s, const int32_t *ids, const float *pos, int32_t count) {
    int rc = set_device(s); if (rc) return rc;
    const std::vector<int32_t> &lof = local_of_old(s);
    if (s->kin_seen.size() != (size_t)s->n) s->kin_seen.assign((size_t)s->n, 0);
    const uint32_t stamp = ++s->kin_stamp;
    int32_t n_mine = 0;
    for (int32_t k = 0; k < count; ++k) {
        if (ids[k] < 0 || ids[k] >= s->n) return fail(SB_ERR_INVALID_ARG, "sb_set_kinematic_positions: particle index out of range");
        if (s->invm[(size_t)ids[k]] != 0.0f)
            return fail(SB_ERR_INVALID_ARG, "sb_set_kinematic_positions: particle " + std::to_string(ids[k]) + " has a non-zero inverse mass (only pinned particles are kinematic)");
        for (int c = 0; c < 3; ++c) if (!(pos[3 * (size_t)k + c] == pos[3 * (size_t)k + c])) return fail(SB_ERR_INVALID_ARG, "sb_set_kinematic_positions: NaN");
        // each id at most once: twice would be an order-dependent result and, in the fused path, a write race on one target slot
        if (s->kin_seen[(size_t)ids[k]] == stamp) return fail(SB_ERR_INVALID_ARG, "sb_set_kinematic_positions: particle " + std::to_string(ids[k]) + " appears twice");
        s->kin_seen[(size_t)ids[k]] = stamp;
        const int32_t l = lof[(size_t)ids[k]];
        if (l >= 0 && l < s->n_owned) ++n_mine;
    }
    if (n_mine == 0) return SB_OK;
    if (s->kin_pending >= 0) flush_deferred(s);       // two moves without a tick between them: the earlier one takes effect first
    const int q = s->kin_next;
    s->kin_next = (q + 1) % sb_solver::kKinSlots;
    if (!s->ev_kin[q]) HIP_CHECK(hipEventCreateWithFlags(&s->ev_kin[q], hipEventDisableTiming));
    else HIP_CHECK(hipEventSynchronize(s->ev_kin[q]));       // the kernel that read this table (four calls ago) is done
    if (s->kin_cap[q] < (size_t)n_mine) {
        if (s->h_kin_idx[q]) { (void)hipHostFree(s->h_kin_idx[q]); s->h_kin_idx[q] = nullptr; }
        if (s->h_kin_pos[q]) { (void)hipHostFree(s->h_kin_pos[q]); s->h_kin_pos[q] = nullptr; }
        const size_t cap = std::max<size_t>(256, (size_t)n_mine * 2);
        // mapped pinned memory: the kernels read the tables in place, through the device-side alias of the allocation
        HIP_CHECK(hipHostMalloc((void **)&s->h_kin_idx[q], cap * sizeof(int32_t), hipHostMallocMapped));
        HIP_CHECK(hipHostMalloc((void **)&s->h_kin_pos[q], cap * 3 * sizeof(float), hipHostMallocMapped));
        HIP_CHECK(hipHostGetDevicePointer((void **)&s->d_kin_idx[q], s->h_kin_idx[q], 0));
        HIP_CHECK(hipHostGetDevicePointer((void **)&s->d_kin_pos[q], s->h_kin_pos[q], 0));
        s->kin_cap[q] = cap;
    }
    int32_t w = 0;
    for (int32_t k = 0; k < count; ++k) {
        const int32_t l = lof[(size_t)ids[k]];
        if (l < 0 || l >= s->n_owned) continue;
        s->h_kin_idx[q][w] = l;
        for (int c = 0; c < 3; ++c) s->h_kin_pos[q][3 * (size_t)w + c] = pos[3 * (size_t)k + c];
        ++w;
    }
    // PENDING until the next tick starts (the previous tick's held-back last kernel still reads the old positions of these
    // particles): a fused first kernel takes them along, every other way across the tick boundary scatters them (flush_deferred)
    s->kin_pending = q; s->kin_pending_count = n_mine;
    return SB_OK;
}

}  // namespace sbi

extern "C" {

int sb_set_state(sb_solver *s, const float *pos, const float *vel, int32_t n) {
    if (!s || !pos || !vel) return fail(SB_ERR_INVALID_ARG, "sb_set_state: null argument");
    if (!s->finalized) return fail(SB_ERR_STATE, "sb_set_state before sb_finalize");
    if (n != s->n) return fail(SB_ERR_INVALID_ARG, "sb_set_state: n differs from sb_set_particles");
    return guarded([&]() -> int { return set_state_from(s, pos, vel, nullptr); });
}

int sb_set_kinematic_positions(sb_solver *s, const int32_t *ids, const float *pos, int32_t count) {
    if (!s || count < 0 || (count > 0 && (!ids || !pos))) return fail(SB_ERR_INVALID_ARG, "sb_set_kinematic_positions: bad argument");
    if (!s->finalized) return fail(SB_ERR_STATE, "sb_set_kinematic_positions before sb_finalize");
    if (count == 0) return SB_OK;
    return guarded([&]() -> int { return set_kinematic(s, ids, pos, count); });
}

}  // extern "C"

// sb_readback_begin with an embedding set (SPEC.md 6b), slot k: the skinned visual mesh instead of the particles. The kernel reads the
// tick-end positions where they are -- the state, or a peek of the T0 tiles that hold a cage particle -- so no particle snapshot is taken.
static void begin_embedded(sb_solver *s, int k) {
    sb_solver::Embedding &E = s->emb;
    const size_t m3 = (size_t)E.m * 3;
    if (E.dirty) {      // cage in device numbering, the distinct cage particles, incident-triangle lists, the slots' buffers
        HIP_CHECK(hipStreamSynchronize(s->copy_stream));
        const std::vector<int32_t> &lof = local_of_old(s);
        std::vector<int4> cage((size_t)E.m);
        std::vector<float4> w((size_t)E.m);
        std::vector<uint8_t> seen((size_t)s->n_local, 0);
        E.wanted_local.clear();
        for (int32_t r = 0; r < E.m; ++r) {
            int32_t l[4];
            for (int j = 0; j < 4; ++j) {
                l[j] = lof[(size_t)E.cage[4 * (size_t)r + j]];
                if (!seen[(size_t)l[j]]) { seen[(size_t)l[j]] = 1; E.wanted_local.push_back(l[j]); }
            }
            cage[(size_t)r] = make_int4(l[0], l[1], l[2], l[3]);
            w[(size_t)r] = make_float4(E.w[4 * (size_t)r], E.w[4 * (size_t)r + 1], E.w[4 * (size_t)r + 2], E.w[4 * (size_t)r + 3]);
        }
        E.release();
        E.d_cage.upload(cage, s->dev_bytes); E.d_w.upload(w, s->dev_bytes);
        if (!E.tri.empty()) {
            std::vector<int32_t> off, adj;
            build_adjacency(E.tri, E.m, off, adj);
            E.d_tri.upload(E.tri, s->dev_bytes); E.d_adj_off.upload(off, s->dev_bytes); E.d_adj_tri.upload(adj, s->dev_bytes);
        }
        for (int q = 0; q < sb_solver::kSnapSlots; ++q) {
            E.d_pos[q].alloc(m3, s->dev_bytes);
            HIP_CHECK(hipHostMalloc((void **)&E.h_pos[q], m3 * sizeof(float), hipHostMallocDefault));
            if (!E.tri.empty()) {
                E.d_nrm[q].alloc(m3, s->dev_bytes);
                HIP_CHECK(hipHostMalloc((void **)&E.h_nrm[q], m3 * sizeof(float), hipHostMallocDefault));
            }
        }
        E.dirty = false;
        s->n_peek_tiles = -1;       // the peek's tile subset follows the cage particles
    }
    // skinning on the compute stream (ordered after every tick enqueued so far, before the next one) ...
    const float *src = render_source(s, /*compact=*/true, E.wanted_local);
    launch_skin(s->stream, src, E.d_cage.p, E.d_w.p, E.d_pos[k].p, (int)E.m);
    HIP_CHECK(hipEventRecord(s->ev_snap[k], s->stream));
    // ... normals (SPEC.md 6a on the skinned array) and D2H on the copy stream
    HIP_CHECK(hipStreamWaitEvent(s->copy_stream, s->ev_snap[k], 0));
    HIP_CHECK(hipMemcpyAsync(E.h_pos[k], E.d_pos[k].p, m3 * sizeof(float), hipMemcpyDeviceToHost, s->copy_stream));
    s->snap_has_normals[k] = false; s->tan.snap_has[k] = false;
    if (!E.tri.empty()) {
        if (s->tan.on()) {      // SPEC.md 6c: normals and tangents in one walk
            s->tan.prepare(E.tri, (size_t)E.m, s->dev_bytes);
            launch_normals_tangents(s->copy_stream, E.d_pos[k].p, E.d_adj_off.p, E.d_adj_tri.p, E.d_tri.p, s->tan.d_k.p, E.d_nrm[k].p, s->tan.d_tan[k].p, (int)E.m, nullptr, nullptr);
            HIP_CHECK(hipMemcpyAsync(s->tan.h_tan[k], s->tan.d_tan[k].p, (size_t)E.m * sizeof(float4), hipMemcpyDeviceToHost, s->copy_stream));
            s->tan.snap_has[k] = true;
        } else
            launch_normals(s->copy_stream, E.d_pos[k].p, E.d_adj_off.p, E.d_adj_tri.p, E.d_tri.p, E.d_nrm[k].p, (int)E.m, nullptr, nullptr);
        HIP_CHECK(hipMemcpyAsync(E.h_nrm[k], E.d_nrm[k].p, m3 * sizeof(float), hipMemcpyDeviceToHost, s->copy_stream));
        s->snap_has_normals[k] = true;
    }
    s->snap_compact[k] = false; s->snap_has_render_set[k] = false; s->snap_embedded[k] = true;
    s->bnd.snap_has[k] = s->bnd.enabled;
    if (s->bnd.enabled) launch_bounds(s->copy_stream, s->bnd, k, E.d_pos[k].p, nullptr, E.m, s->dev_bytes);      // SPEC.md 6d on the skinned vertices
    HIP_CHECK(hipEventRecord(s->ev_copied[k], s->copy_stream));
    ++s->snap_pending;
}

extern "C" {

/* ---- asynchronous render readback -------------------------------------------- */

int sb_readback_begin(sb_solver *s) {
    if (!s) return fail(SB_ERR_INVALID_ARG, "sb_readback_begin: null handle");
    if (!s->finalized) return fail(SB_ERR_STATE, "sb_readback_begin before sb_finalize");
    if (s->snap_pending == 2) return fail(SB_ERR_STATE, "sb_readback_begin: two snapshots already pending, call sb_readback_end");
    return guarded([&]() -> int {
        int rc = set_device(s); if (rc) return rc;
        if (!s->copy_stream) {
            HIP_CHECK(hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking));
            for (int k = 0; k < sb_solver::kSnapSlots; ++k) {
                HIP_CHECK(hipEventCreateWithFlags(&s->ev_snap[k], hipEventDisableTiming));
                HIP_CHECK(hipEventCreateWithFlags(&s->ev_copied[k], hipEventDisableTiming));
            }
        }
        const int k = (s->snap_head + s->snap_pending) % sb_solver::kSnapSlots;
        if (s->emb.m > 0) { begin_embedded(s, k); return SB_OK; }       // (no particle snapshot: its n-sized buffers are not even allocated)
        if (!s->h_snap[sb_solver::kSnapSlots - 1]) {
            if (!s->d_local_to_old.p) s->d_local_to_old.upload(s->plan->local.local_to_old, s->dev_bytes);
            for (int q = 0; q < sb_solver::kSnapSlots; ++q) {
                if (s->h_snap[q]) continue;
                s->d_snap[q].alloc((size_t)s->n * 3, s->dev_bytes);
                HIP_CHECK(hipMemset(s->d_snap[q].p, 0, (size_t)s->n * 3 * sizeof(float)));
                HIP_CHECK(hipHostMalloc((void **)&s->h_snap[q], (size_t)s->n * 3 * sizeof(float), hipHostMallocDefault));
                std::memset(s->h_snap[q], 0, (size_t)s->n * 3 * sizeof(float));
            }
        }
        s->snap_embedded[k] = false;
        // snapshot on the compute stream (ordered after every tick enqueued so far, before the next one) ...
        const bool compact = s->render_set_only && !s->render_tri.empty();
        // a rank of a partitioned solver serves the render particles it OWNS; vertex normals need the neighbours' particles too and are
        // computed on the gathered snapshot (sb_group_readback_*), not per rank
        const bool single = s->desc.world == 1;
        if (!s->render_tri.empty() && s->render_dirty) {     // (re)build the incident-triangle lists: triangle ids ascending per particle
            HIP_CHECK(hipStreamSynchronize(s->copy_stream));
            const int64_t m = (int64_t)s->render_tri.size() / 3;
            std::vector<int32_t> off((size_t)s->n + 1, 0), adj((size_t)3 * m);
            for (int64_t c = 0; c < 3 * m; ++c) ++off[(size_t)s->render_tri[c] + 1];
            s->render_set.clear();
            const std::vector<int32_t> &lof = local_of_old(s);
            for (int32_t v = 0; v < s->n; ++v) {
                if (off[(size_t)v + 1] && lof[(size_t)v] >= 0 && lof[(size_t)v] < s->n_owned) s->render_set.push_back(v);
                off[(size_t)v + 1] += off[v];
            }
            std::vector<int32_t> cur(off.begin(), off.end() - 1);
            for (int64_t t = 0; t < m; ++t)
                for (int j = 0; j < 3; ++j) adj[(size_t)cur[s->render_tri[3 * t + j]]++] = (int32_t)t;
            std::vector<int32_t> local_of(s->render_set.size());
            for (size_t q = 0; q < local_of.size(); ++q) local_of[q] = lof[(size_t)s->render_set[q]];
            s->render_local = local_of;
            s->d_tri.upload(s->render_tri, s->dev_bytes);
            s->d_adj_off.upload(off, s->dev_bytes);
            s->d_adj_tri.upload(adj, s->dev_bytes);
            s->d_render_set.upload(s->render_set, s->dev_bytes);
            s->d_render_local.upload(local_of, s->dev_bytes);
            for (int q = 0; q < sb_solver::kSnapSlots; ++q) {
                if (single && !s->h_nrm[q]) {
                    s->d_nrm[q].alloc((size_t)s->n * 3, s->dev_bytes);
                    HIP_CHECK(hipHostMalloc((void **)&s->h_nrm[q], (size_t)s->n * 3 * sizeof(float), hipHostMallocDefault));
                }
                s->d_cpos[q].alloc(s->render_set.size() * 3, s->dev_bytes);
                if (s->h_cpos[q]) { (void)hipHostFree(s->h_cpos[q]); s->h_cpos[q] = nullptr; }
                HIP_CHECK(hipHostMalloc((void **)&s->h_cpos[q], std::max<size_t>(s->render_set.size(), 1) * 3 * sizeof(float), hipHostMallocDefault));
            }
            s->render_dirty = false;
            s->n_peek_tiles = -1;
        }
        const bool tangents = single && !s->render_tri.empty() && s->tan.on();
        if (tangents) s->tan.prepare(s->render_tri, (size_t)s->n, s->dev_bytes);      // (sized like the normals: n rows, whatever a snapshot carries)
        sbk::PosView src = s->pos_view();
        // the tick's last kernel is deferred: snapshot a peek and leave it deferred
        src.xyz = const_cast<float *>(render_source(s, compact, s->render_local));
        if (compact) {      // only the render set leaves the device: snapshot just those particles
            const int cnt = (int)s->render_set.size();
            if (cnt && single)      // (into the caller-numbered array: the normals kernel gathers neighbours by caller id and emits the compact arrays)
                hipLaunchKernelGGL(sbk::snapshot_subset_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s->stream, src,
                                   s->d_render_set.p, s->d_render_local.p, s->d_snap[k].p, cnt);
            else if (cnt)           // (no normals here: straight into the compact array)
                hipLaunchKernelGGL(sbk::snapshot_compact_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s->stream, src,
                                   s->d_render_local.p, s->d_cpos[k].p, cnt);
        } else if (s->n_owned)
            hipLaunchKernelGGL(sbk::snapshot_kernel, dim3((unsigned)((s->n_owned + 255) / 256)), dim3(256), 0, s->stream,
                               src, s->d_local_to_old.p, s->d_snap[k].p, (int)s->n_owned);
        HIP_CHECK(hipEventRecord(s->ev_snap[k], s->stream));
        // ... D2H on the copy stream, overlapping whatever the compute stream does next
        HIP_CHECK(hipStreamWaitEvent(s->copy_stream, s->ev_snap[k], 0));
        if (!compact)
            HIP_CHECK(hipMemcpyAsync(s->h_snap[k], s->d_snap[k].p, (size_t)s->n * 3 * sizeof(float), hipMemcpyDeviceToHost, s->copy_stream));
        s->snap_has_normals[k] = false; s->tan.snap_has[k] = false;
        s->snap_compact[k] = compact;
        s->snap_has_render_set[k] = !s->render_tri.empty();
        if (compact && !single && !s->render_set.empty())
            HIP_CHECK(hipMemcpyAsync(s->h_cpos[k], s->d_cpos[k].p, s->render_set.size() * 3 * sizeof(float), hipMemcpyDeviceToHost, s->copy_stream));
        if (!s->render_tri.empty() && single) {
            const int count = compact ? (int)s->render_set.size() : (int)s->n;
            if (tangents) {     // SPEC.md 6c: normals and tangents in one walk
                launch_normals_tangents(s->copy_stream, s->d_snap[k].p, s->d_adj_off.p, s->d_adj_tri.p, s->d_tri.p, s->tan.d_k.p, s->d_nrm[k].p, s->tan.d_tan[k].p, count,
                                        compact ? s->d_render_set.p : (const int32_t *)nullptr, compact ? s->d_cpos[k].p : (float *)nullptr);
                HIP_CHECK(hipMemcpyAsync(s->tan.h_tan[k], s->tan.d_tan[k].p, (size_t)count * sizeof(float4), hipMemcpyDeviceToHost, s->copy_stream));
                s->tan.snap_has[k] = true;
            } else {
                hipLaunchKernelGGL(sbk::normals_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s->copy_stream, s->d_snap[k].p,
                                   s->d_adj_off.p, s->d_adj_tri.p, s->d_tri.p, s->d_nrm[k].p, count,
                                   compact ? s->d_render_set.p : (const int32_t *)nullptr, compact ? s->d_cpos[k].p : (float *)nullptr);
                HIP_CHECK(hipGetLastError());
            }
            HIP_CHECK(hipMemcpyAsync(s->h_nrm[k], s->d_nrm[k].p, (size_t)count * 3 * sizeof(float), hipMemcpyDeviceToHost, s->copy_stream));
            if (compact)
                HIP_CHECK(hipMemcpyAsync(s->h_cpos[k], s->d_cpos[k].p, (size_t)count * 3 * sizeof(float), hipMemcpyDeviceToHost, s->copy_stream));
            s->snap_has_normals[k] = true;
        }
        s->bnd.snap_has[k] = s->bnd.enabled;
        if (s->bnd.enabled) {       // SPEC.md 6d on what this snapshot delivers: the compact array, or the rows of the full one this rank owns
            if (compact) launch_bounds(s->copy_stream, s->bnd, k, s->d_cpos[k].p, nullptr, (int64_t)s->render_set.size(), s->dev_bytes);
            else launch_bounds(s->copy_stream, s->bnd, k, s->d_snap[k].p, single ? (const int32_t *)nullptr : s->d_local_to_old.p, single ? (int64_t)s->n : s->n_owned, s->dev_bytes);
        }
        HIP_CHECK(hipEventRecord(s->ev_copied[k], s->copy_stream));
        ++s->snap_pending;
        return SB_OK;
    });
}

int sb_readback_end(sb_solver *s, const float **pos_xyz_out) {
    if (!s || !pos_xyz_out) return fail(SB_ERR_INVALID_ARG, "sb_readback_end: null argument");
    if (s->snap_pending == 0) return fail(SB_ERR_STATE, "sb_readback_end without a pending sb_readback_begin");
    return guarded([&]() -> int {
        int rc = set_device(s); if (rc) return rc;
        const int k = s->snap_head;
        HIP_CHECK(hipEventSynchronize(s->ev_copied[k]));
        check_peer_error(s);       // (the snapshot was taken behind every tick enqueued before it)
        *pos_xyz_out = s->snap_embedded[k] ? s->emb.h_pos[k] : (s->snap_compact[k] ? s->h_cpos[k] : s->h_snap[k]);
        s->snap_last_ended = k;
        s->snap_head = (s->snap_head + 1) % sb_solver::kSnapSlots; --s->snap_pending;
        return SB_OK;
    });
}

int sb_set_render_triangles(sb_solver *s, const int32_t *tri, int32_t m) {
    if (!s || m < 0 || (m > 0 && !tri)) return fail(SB_ERR_INVALID_ARG, "sb_set_render_triangles: bad argument");
    if (s->n <= 0) return fail(SB_ERR_STATE, "sb_set_render_triangles before sb_set_particles");
    if (s->snap_pending) return fail(SB_ERR_STATE, "sb_set_render_triangles while a readback is pending");
    if (m > 0 && s->emb.m > 0)
        return fail(SB_ERR_STATE, "sb_set_render_triangles: a render embedding is set (switch it off first: sb_set_render_embedding with m_vertices = 0)");
    return guarded([&]() -> int {
        for (int64_t c = 0; c < 3 * (int64_t)m; ++c)
            if (tri[c] < 0 || tri[c] >= s->n) return fail(SB_ERR_INVALID_ARG, "sb_set_render_triangles: particle index out of range");
        s->tan.clear();         // every call that is accepted clears the UVs (sb_set_render_uvs): they belong to the triangle list they were given for
        s->render_tri.assign(tri, tri + 3 * (size_t)m);
        s->render_dirty = true;
        if (m == 0) s->render_set_only = false;
        for (bool &b : s->snap_has_normals) b = false;
        for (bool &b : s->snap_has_render_set) b = false;
        return SB_OK;
    });
}

int sb_set_render_embedding(sb_solver *s, const int32_t *cage_ijkl, const float *weights4, int32_t m_vertices, const int32_t *tri_abc, int32_t m_tri) {
    if (!s) return fail(SB_ERR_INVALID_ARG, "sb_set_render_embedding: null handle");
    if (s->desc.world > 1)
        return fail(SB_ERR_UNSUPPORTED, "sb_set_render_embedding: a rank of a partitioned solver does not hold every cage particle; a partitioned body is "
                    "skinned on the gathered snapshot (sb_group_set_render_embedding)");
    if (s->n <= 0) return fail(SB_ERR_STATE, "sb_set_render_embedding before sb_set_particles");
    if (s->snap_pending) return fail(SB_ERR_STATE, "sb_set_render_embedding while a readback is pending");
    if (m_vertices > 0 && !s->render_tri.empty())
        return fail(SB_ERR_STATE, "sb_set_render_embedding: render triangles are set (switch them off first: sb_set_render_triangles with m = 0)");
    return guarded([&]() -> int {
        if (int rc = check_embedding_args("sb_set_render_embedding", s->n, cage_ijkl, weights4, m_vertices, tri_abc, m_tri)) return rc;
        s->tan.clear();         // every call that is accepted clears the UVs (sb_set_render_uvs)
        if (m_vertices == 0 && s->emb.m == 0) return SB_OK;      // off already
        std::vector<int32_t> cage(cage_ijkl, cage_ijkl + 4 * (size_t)m_vertices), tri(tri_abc, tri_abc + 3 * (size_t)m_tri);
        std::vector<float> w(weights4, weights4 + 4 * (size_t)m_vertices);
        if (s->finalized) { int rc = set_device(s); if (rc) return rc; }
        if (s->copy_stream) HIP_CHECK(hipStreamSynchronize(s->copy_stream));
        s->emb.release();       // (pointers handed out by earlier readbacks of the embedding end here)
        s->emb.cage.swap(cage); s->emb.w.swap(w); s->emb.tri.swap(tri);
        s->emb.m = m_vertices;
        s->emb.dirty = m_vertices > 0;
        s->n_peek_tiles = -1;
        for (bool &b : s->snap_has_normals) b = false;
        for (bool &b : s->snap_has_render_set) b = false;
        if (s->snap_last_ended >= 0 && s->snap_embedded[s->snap_last_ended]) s->snap_last_ended = -1;
        return SB_OK;
    });
}

int sb_readback_get_normals(sb_solver *s, const float **out) {
    if (!s || !out) return fail(SB_ERR_INVALID_ARG, "sb_readback_get_normals: null argument");
    if (s->desc.world > 1)
        return fail(SB_ERR_UNSUPPORTED, "sb_readback_get_normals: a rank of a partitioned solver does not hold its neighbours' particles; vertex normals of a partitioned "
                    "body are computed on the gathered snapshot (sb_group_readback_get_normals)");
    if (s->snap_last_ended < 0 || !s->snap_has_normals[s->snap_last_ended])
        return fail(SB_ERR_STATE, "sb_readback_get_normals: no finished readback with render triangles set");
    *out = s->snap_embedded[s->snap_last_ended] ? s->emb.h_nrm[s->snap_last_ended] : s->h_nrm[s->snap_last_ended];
    return SB_OK;
}

int sb_set_render_uvs(sb_solver *s, const float *uv, int32_t count) {
    if (!s) return fail(SB_ERR_INVALID_ARG, "sb_set_render_uvs: null handle");
    if (s->desc.world > 1)
        return fail(SB_ERR_UNSUPPORTED, "sb_set_render_uvs: a rank of a partitioned solver does not hold its neighbours' particles; vertex tangents of a partitioned "
                    "body are computed on the gathered snapshot (sb_group_set_render_uvs)");
    return guarded([&]() -> int {
        if (s->finalized) { int rc = set_device(s); if (rc) return rc; }
        const int64_t rows = !s->render_tri.empty() ? (int64_t)s->n : (s->emb.m > 0 && !s->emb.tri.empty() ? (int64_t)s->emb.m : -1);
        return set_render_uvs("sb_set_render_uvs", s->tan, uv, count, rows, s->snap_pending != 0);
    });
}

int sb_readback_get_tangents(sb_solver *s, const float **out) {
    if (!s || !out) return fail(SB_ERR_INVALID_ARG, "sb_readback_get_tangents: null argument");
    if (s->desc.world > 1)
        return fail(SB_ERR_UNSUPPORTED, "sb_readback_get_tangents: a rank of a partitioned solver does not hold its neighbours' particles; vertex tangents of a partitioned "
                    "body are computed on the gathered snapshot (sb_group_readback_get_tangents)");
    if (s->snap_last_ended < 0 || !s->tan.snap_has[s->snap_last_ended])
        return fail(SB_ERR_STATE, "sb_readback_get_tangents: no finished readback with render UVs set");
    *out = reinterpret_cast<const float *>(s->tan.h_tan[s->snap_last_ended]);
    return SB_OK;
}

int sb_set_readback_bounds(sb_solver *s, int32_t enabled) {
    if (!s) return fail(SB_ERR_INVALID_ARG, "sb_set_readback_bounds: null handle");
    if (s->snap_pending) return fail(SB_ERR_STATE, "sb_set_readback_bounds while a readback is pending");
    s->bnd.enabled = enabled != 0;
    return SB_OK;
}

int sb_readback_get_bounds(sb_solver *s, float lo_xyz[3], float hi_xyz[3]) {
    if (!s || !lo_xyz || !hi_xyz) return fail(SB_ERR_INVALID_ARG, "sb_readback_get_bounds: null argument");
    if (s->snap_last_ended < 0 || !s->bnd.snap_has[s->snap_last_ended])
        return fail(SB_ERR_STATE, "sb_readback_get_bounds: no finished readback that was begun with bounds on (sb_set_readback_bounds)");
    s->bnd.read(s->snap_last_ended, lo_xyz, hi_xyz);
    return SB_OK;
}

int sb_get_bounds(sb_solver *s, float lo_xyz[3], float hi_xyz[3]) {
    if (!s || !lo_xyz || !hi_xyz) return fail(SB_ERR_INVALID_ARG, "sb_get_bounds: null argument");
    if (!s->finalized) return fail(SB_ERR_STATE, "sb_get_bounds before sb_finalize");
    return guarded([&]() -> int { return get_bounds_owned(s, lo_xyz, hi_xyz); });
}

int sb_set_readback_render_set_only(sb_solver *s, int32_t on) {
    if (!s) return fail(SB_ERR_INVALID_ARG, "sb_set_readback_render_set_only: null handle");
    if (s->snap_pending) return fail(SB_ERR_STATE, "sb_set_readback_render_set_only while a readback is pending");
    if (on && s->render_tri.empty()) return fail(SB_ERR_STATE, "sb_set_readback_render_set_only: set the render triangles first");
    s->render_set_only = on != 0;
    return SB_OK;
}

int sb_readback_get_render_set(sb_solver *s, const int32_t **ids, int32_t *count) {
    if (!s || !ids || !count) return fail(SB_ERR_INVALID_ARG, "sb_readback_get_render_set: null argument");
    if (s->emb.m > 0) return fail(SB_ERR_STATE, "sb_readback_get_render_set: a render embedding is set (the readback brings render vertices, not particles)");
    if (s->snap_last_ended < 0 || !s->snap_has_render_set[s->snap_last_ended])
        return fail(SB_ERR_STATE, "sb_readback_get_render_set: no finished readback with render triangles set");
    *ids = s->render_set.data();
    *count = (int32_t)s->render_set.size();
    return SB_OK;
}

}  // extern "C"
