// render.hip — the asynchronous render readback: the launch helpers of its kernels, the stage a solver and a group share behind the packed
// xyz array (GPU vertex normals, tangents, compact positions, the bounding box and their copies to pinned memory), the bodies their entry
// points share, and the solver's own sb_readback_* / sb_set_render_* entry points
//
// No reference counterpart exists (/root/reference/README.md:1 is the whole reference tree); the exported functions are the
// [BUILDER-DEFINED] boundary of SURVEY.md §8b (include/softbody*.h).
#include "solver_internal.hpp"
#include "readback_kernels.hip.hpp"
#include "closest_kernels.hip.hpp"

using namespace sbi;

namespace sbi {

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
static void launch_normals(hipStream_t st, const float *snap_xyz, const RenderTopology &T, float *nrm_xyz, int count, const int32_t *subset, float *subset_pos_xyz) {
    if (count <= 0) return;
    hipLaunchKernelGGL(sbk::normals_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, snap_xyz, T.d_adj_off.p, T.d_adj_tri.p, T.d_tri.p, nrm_xyz, count, subset,
                       subset_pos_xyz);
    HIP_CHECK(hipGetLastError());
}
// the same with tangents (SPEC.md 6c): tri_k = RenderTangents::d_k, tan_xyzw one float4 per lane
static void launch_normals_tangents(hipStream_t st, const float *snap_xyz, const RenderTopology &T, const float4 *tri_k, float *nrm_xyz, float4 *tan_xyzw, int count,
                                    const int32_t *subset, float *subset_pos_xyz) {
    if (count <= 0) return;
    hipLaunchKernelGGL(sbk::normals_tangents_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, snap_xyz, T.d_adj_off.p, T.d_adj_tri.p, T.d_tri.p, tri_k, nrm_xyz,
                       tan_xyzw, count, subset, subset_pos_xyz);
    HIP_CHECK(hipGetLastError());
}

void launch_skin(hipStream_t st, const float *src_xyz, const int4 *cage, const float4 *weights, float *out_xyz, int m) {
    if (m <= 0) return;
    hipLaunchKernelGGL(sbk::skin_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, src_xyz, cage, weights, out_xyz, m);
    HIP_CHECK(hipGetLastError());
}

void ReadbackBounds::prepare(int64_t &acct) {
    if (box.h.p) return;
    d_partials.alloc((size_t)2 * 6 * sbk::kBoundsMaxGroups, acct);
    box.alloc((size_t)8 * (kSnapSlots + 1), acct);
}

void launch_bounds(hipStream_t st, ReadbackBounds &B, int slot, const float *xyz, const int32_t *rows, int64_t count, int64_t &acct) {
    B.prepare(acct);
    float *partials = B.d_partials.p + (slot == ReadbackBounds::kQuerySlot ? (size_t)6 * sbk::kBoundsMaxGroups : 0);
    const int groups = (int)std::min<int64_t>((count + sbk::kBoundsLanes - 1) / sbk::kBoundsLanes, sbk::kBoundsMaxGroups);
    if (groups) hipLaunchKernelGGL(sbk::bounds_partial_kernel, dim3((unsigned)groups), dim3(sbk::kBoundsLanes), 0, st, xyz, rows, (int)count, partials);
    hipLaunchKernelGGL(sbk::bounds_final_kernel, dim3(1), dim3(sbk::kBoundsLanes), 0, st, partials, groups, B.box.d.p + 8 * (size_t)slot);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(B.box.h.p + 8 * (size_t)slot, B.box.d.p + 8 * (size_t)slot, 8 * sizeof(float), hipMemcpyDeviceToHost, st));
}

static_assert(sizeof(sb_ray_hit) == sizeof(uint4), "raycast_final_kernel writes an sb_ray_hit as one 16-byte store");
static_assert(sizeof(sb_closest_hit) == sizeof(uint4), "closest_final_kernel writes an sb_closest_hit as one 16-byte store");

void ReadbackRaycast::prepare(int64_t &acct) {
    if (stream) return;
    rays.alloc((size_t)8 * sbk::kRayBatch, acct);
    hits.alloc((size_t)sbk::kRayBatch, acct);
    d_partials.alloc((size_t)sbk::kRayMaxGroups * sbk::kRayBatch, acct);
    stream.create();
}

// SPEC.md 6c, static part: (dv2, dv1, du1, du2) / det per triangle in f32, zeros where det == 0 or a quotient is not finite. Host code of a
// unit built with contraction off: two rounded products and one subtraction for det, four IEEE divisions.
static void tangent_coefficients(const std::vector<float> &uv, const std::vector<int32_t> &tri, std::vector<float4> &k) {
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
    if (rows < n_rows || !tan[kSnapSlots - 1].h.p) {
        for (auto &t : tan) t.alloc(n_rows, acct);
        rows = n_rows;
    }
}

// incident-triangle lists per vertex, triangle ids ascending (what normals_kernel walks)
static void build_adjacency(const std::vector<int32_t> &tri, int32_t n_vertices, std::vector<int32_t> &off, std::vector<int32_t> &adj) {
    const int64_t m = (int64_t)tri.size() / 3;
    off.assign((size_t)n_vertices + 1, 0); adj.resize((size_t)3 * m);
    for (int64_t c = 0; c < 3 * m; ++c) ++off[(size_t)tri[c] + 1];
    for (int32_t v = 0; v < n_vertices; ++v) off[(size_t)v + 1] += off[v];
    std::vector<int32_t> cur(off.begin(), off.end() - 1);
    for (int64_t t = 0; t < m; ++t)
        for (int j = 0; j < 3; ++j) adj[(size_t)cur[tri[3 * t + j]]++] = (int32_t)t;
}

std::vector<int32_t> RenderTopology::upload(const std::vector<int32_t> &tri, int32_t n_vertices, int64_t &acct) {
    std::vector<int32_t> off, adj;
    build_adjacency(tri, n_vertices, off, adj);
    d_tri.upload(tri, acct); d_adj_off.upload(off, acct); d_adj_tri.upload(adj, acct);
    return off;
}

void RenderEmbedding::upload(const std::vector<int4> &cage_in_source_numbering, int64_t &acct) {
    const size_t m3 = (size_t)m * 3;
    std::vector<float4> w4((size_t)m);
    for (size_t r = 0; r < (size_t)m; ++r) w4[r] = make_float4(w[4 * r], w[4 * r + 1], w[4 * r + 2], w[4 * r + 3]);
    release();
    d_cage.upload(cage_in_source_numbering, acct); d_w.upload(w4, acct);
    if (!tri.empty()) topo.upload(tri, m, acct);
    for (int q = 0; q < kSnapSlots; ++q) {
        pos[q].alloc(m3, acct);
        if (!tri.empty()) nrm[q].alloc(m3, acct);
    }
    dirty = false;
}

void launch_normals_stage(hipStream_t st, RenderState &R, int k, const float *xyz, int count, bool compact, size_t tan_rows, int64_t &acct) {
    const bool embedded = R.slot[k].embedded;
    const RenderTopology &T = embedded ? R.emb.topo : R.topo;
    Mirror<float> &nrm = embedded ? R.emb.nrm[k] : R.nrm[k];
    const int32_t *subset = compact ? R.d_set.p : nullptr;
    float *subset_pos = compact ? R.cpos[k].d.p : nullptr;
    if (R.tan.on()) {       // SPEC.md 6c: normals and tangents in one walk
        R.tan.prepare(embedded ? R.emb.tri : R.tri, tan_rows, acct);
        launch_normals_tangents(st, xyz, T, R.tan.d_k.p, nrm.d.p, R.tan.tan[k].d.p, count, subset, subset_pos);
        R.tan.tan[k].copy_out(st, (size_t)count);
    } else
        launch_normals(st, xyz, T, nrm.d.p, count, subset, subset_pos);
    nrm.copy_out(st, (size_t)count * 3);
    if (compact) R.cpos[k].copy_out(st, (size_t)count * 3);
    R.slot[k].has_normals = true;
    R.tan.snap_has[k] = R.tan.on();
}

void launch_bounds_stage(hipStream_t st, ReadbackBounds &B, int k, const float *xyz, const int32_t *rows, int64_t count, int64_t &acct) {
    B.snap_has[k] = B.enabled;
    if (B.enabled) launch_bounds(st, B, k, xyz, rows, count, acct);
}

const float *end_slot(RenderState &R) {
    const int k = R.head;
    R.last_ended = k;
    R.head = (R.head + 1) % kSnapSlots; --R.pending;
    return R.slot[k].embedded ? R.emb.pos[k].h.p : (R.slot[k].compact ? R.cpos[k].h.p : R.pos[k].h.p);
}

int set_render_triangles(const char *who, RenderState &R, int32_t n, const int32_t *tri, int32_t m) {
    for (int64_t c = 0; c < 3 * (int64_t)m; ++c)
        if (tri[c] < 0 || tri[c] >= n) return fail(SB_ERR_INVALID_ARG, std::string(who) + ": particle index out of range");
    R.tan.clear();          // every call that is accepted clears the UVs (set_render_uvs): they belong to the triangle list they were given for
    R.tri.assign(tri, tri + 3 * (size_t)m);
    R.dirty = true;
    if (m == 0) R.set_only = false;
    R.forget_normals();
    return SB_OK;
}

static int check_embedding_args(const std::string &me, int32_t n, const int32_t *cage, const float *w, int32_t m, const int32_t *tri, int32_t m_tri) {
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

int set_render_embedding(const char *who, RenderState &R, int32_t n, const int32_t *cage_ijkl, const float *weights4, int32_t m_vertices, const int32_t *tri_abc, int32_t m_tri) {
    if (int rc = check_embedding_args(who, n, cage_ijkl, weights4, m_vertices, tri_abc, m_tri)) return rc;
    R.tan.clear();          // every call that is accepted clears the UVs (set_render_uvs)
    if (m_vertices == 0 && R.emb.m == 0) return SB_OK;       // off already
    std::vector<int32_t> cage(cage_ijkl, cage_ijkl + 4 * (size_t)m_vertices), tri(tri_abc, tri_abc + 3 * (size_t)m_tri);
    std::vector<float> w(weights4, weights4 + 4 * (size_t)m_vertices);
    if (R.copy_stream) HIP_CHECK(hipStreamSynchronize(R.copy_stream));
    R.emb.release();        // (pointers handed out by earlier readbacks of the embedding end here)
    R.emb.cage.swap(cage); R.emb.w.swap(w); R.emb.tri.swap(tri);
    R.emb.m = m_vertices;
    R.emb.dirty = m_vertices > 0;
    R.forget_normals();
    if (R.last_ended >= 0 && R.slot[R.last_ended].embedded) R.last_ended = -1;
    return SB_OK;
}

int set_render_uvs(const char *who, RenderState &R, int32_t n, const float *uv, int32_t count) {
    const std::string me(who);
    const int64_t rows = !R.tri.empty() ? (int64_t)n : (R.emb.m > 0 && !R.emb.tri.empty() ? (int64_t)R.emb.m : -1);     // vertices of the triangle-bearing render mode in force
    if (R.pending) return fail(SB_ERR_STATE, me + " while a readback is pending");
    if (count == 0) { R.tan.clear(); return SB_OK; }       // tangents off
    if (rows < 0) return fail(SB_ERR_STATE, me + ": no render mode with triangles is set (sb_set_render_triangles, or sb_set_render_embedding with m_tri > 0, comes first)");
    if (count < 0 || !uv) return fail(SB_ERR_INVALID_ARG, me + ": bad argument");
    if (count != rows)
        return fail(SB_ERR_INVALID_ARG, me + ": count is " + std::to_string(count) + ", the render mode in force has " + std::to_string(rows) + " vertices");
    for (int64_t c = 0; c < 2 * (int64_t)count; ++c)
        if (!std::isfinite(uv[c])) return fail(SB_ERR_INVALID_ARG, me + ": UV is NaN or infinite (vertex " + std::to_string(c / 2) + ")");
    R.tan.uv.assign(uv, uv + 2 * (size_t)count);
    R.tan.dirty = true;
    return SB_OK;
}

int set_readback_bounds(const char *who, RenderState &R, int32_t enabled) {
    if (R.pending) return fail(SB_ERR_STATE, std::string(who) + " while a readback is pending");
    R.bnd.enabled = enabled != 0;
    return SB_OK;
}

int set_readback_render_set_only(const char *who, RenderState &R, int32_t on) {
    if (R.pending) return fail(SB_ERR_STATE, std::string(who) + " while a readback is pending");
    if (on && R.tri.empty()) return fail(SB_ERR_STATE, std::string(who) + ": set the render triangles first");
    R.set_only = on != 0;
    return SB_OK;
}

int readback_get_normals(const char *who, RenderState &R, const float **out) {
    const int k = R.last_ended;
    if (k < 0 || !R.slot[k].has_normals) return fail(SB_ERR_STATE, std::string(who) + ": no finished readback with render triangles set");
    *out = R.slot[k].embedded ? R.emb.nrm[k].h.p : R.nrm[k].h.p;
    return SB_OK;
}

int readback_get_tangents(const char *who, RenderState &R, const float **out) {
    if (R.last_ended < 0 || !R.tan.snap_has[R.last_ended]) return fail(SB_ERR_STATE, std::string(who) + ": no finished readback with render UVs set");
    *out = reinterpret_cast<const float *>(R.tan.tan[R.last_ended].h.p);
    return SB_OK;
}

int readback_get_bounds(const char *who, const char *setter, RenderState &R, float lo_xyz[3], float hi_xyz[3]) {
    if (R.last_ended < 0 || !R.bnd.snap_has[R.last_ended])
        return fail(SB_ERR_STATE, std::string(who) + ": no finished readback that was begun with bounds on (" + setter + ")");
    R.bnd.read(R.last_ended, lo_xyz, hi_xyz);
    return SB_OK;
}

// (keyed on has_render_set, which a rank of a partitioned solver sets although it has no normals; on a group's render device the two flags agree)
int readback_get_render_set(const char *who, RenderState &R, const int32_t **ids, int32_t *count) {
    if (R.emb.m > 0) return fail(SB_ERR_STATE, std::string(who) + ": a render embedding is set (the readback brings render vertices, not particles)");
    if (R.last_ended < 0 || !R.slot[R.last_ended].has_render_set) return fail(SB_ERR_STATE, std::string(who) + ": no finished readback with render triangles set");
    *ids = R.set.data();
    *count = (int32_t)R.set.size();
    return SB_OK;
}

int readback_raycast(const char *who, RenderState &R, const float *rays, int32_t count, sb_ray_hit *hits_out, int64_t &acct) {
    const std::string me(who);
    if (count < 0) return fail(SB_ERR_INVALID_ARG, me + ": negative count");
    if (count > 0 && (!rays || !hits_out)) return fail(SB_ERR_INVALID_ARG, me + ": null pointer with a positive count");
    for (int64_t r = 0; r < count; ++r) {       // every ray before anything is written
        const float *q = rays + 8 * r;
        for (int c : {0, 1, 2, 4, 5, 6})
            if (!std::isfinite(q[c])) return fail(SB_ERR_INVALID_ARG, me + ": origin or direction is NaN or infinite (ray " + std::to_string(r) + ")");
        if (!(q[3] >= 0.0f)) return fail(SB_ERR_INVALID_ARG, me + ": t_max is NaN or negative (ray " + std::to_string(r) + ")");
    }
    // the snapshot ended last, where it was taken with triangles in force and they were not set again since (has_normals says both)
    const int k = R.last_ended;
    if (k < 0) return fail(SB_ERR_STATE, me + ": no readback has ended");
    if (!R.slot[k].has_normals)
        return fail(SB_ERR_STATE, me + ": the snapshot ended last has no triangles to cast against (taken without render triangles, or the render mode was set again since)");
    if (count == 0) return SB_OK;
    const bool embedded = R.slot[k].embedded;
    const float *xyz = embedded ? R.emb.pos[k].d.p : R.pos[k].d.p;        // (a compact snapshot wrote the render set's rows of the caller-numbered array)
    const RenderTopology &T = embedded ? R.emb.topo : R.topo;
    const int m = (int)((embedded ? R.emb.tri.size() : R.tri.size()) / 3);
    ReadbackRaycast &Q = R.ray;
    Q.prepare(acct);
    const int groups = (int)std::min<int64_t>(((int64_t)m + sbk::kRayLanes - 1) / sbk::kRayLanes, sbk::kRayMaxGroups);
    for (int64_t done = 0; done < count; done += sbk::kRayBatch) {
        const int nb = (int)std::min<int64_t>(count - done, sbk::kRayBatch);
        std::memcpy(Q.rays.h.p, rays + 8 * done, (size_t)nb * 8 * sizeof(float));
        HIP_CHECK(hipMemcpyAsync(Q.rays.d.p, Q.rays.h.p, (size_t)nb * 8 * sizeof(float), hipMemcpyHostToDevice, Q.stream));
        hipLaunchKernelGGL(sbk::raycast_partial_kernel, dim3((unsigned)groups, (unsigned)((nb + sbk::kRayTile - 1) / sbk::kRayTile)), dim3(sbk::kRayLanes), 0, Q.stream, xyz,
                           T.d_tri.p, m, Q.rays.d.p, nb, Q.d_partials.p);
        hipLaunchKernelGGL(sbk::raycast_final_kernel, dim3((unsigned)nb), dim3(sbk::kRayLanes), 0, Q.stream, Q.d_partials.p, groups, Q.hits.d.p);
        HIP_CHECK(hipGetLastError());
        Q.hits.copy_out(Q.stream, (size_t)nb);
        HIP_CHECK(hipStreamSynchronize(Q.stream));
        std::memcpy(hits_out + done, Q.hits.h.p, (size_t)nb * sizeof(sb_ray_hit));
    }
    return SB_OK;
}

int readback_closest_points(const char *who, RenderState &R, const float *queries, int32_t count, sb_closest_hit *hits_out, int64_t &acct) {
    const std::string me(who);
    if (count < 0) return fail(SB_ERR_INVALID_ARG, me + ": negative count");
    if (count > 0 && (!queries || !hits_out)) return fail(SB_ERR_INVALID_ARG, me + ": null pointer with a positive count");
    for (int64_t r = 0; r < count; ++r) {       // every query before anything is written
        const float *q = queries + 4 * r;
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(q[c])) return fail(SB_ERR_INVALID_ARG, me + ": a coordinate is NaN or infinite (query " + std::to_string(r) + ")");
        if (!(q[3] >= 0.0f)) return fail(SB_ERR_INVALID_ARG, me + ": max_distance is NaN or negative (query " + std::to_string(r) + ")");
    }
    // the snapshot ended last, under the ray cast's condition (has_normals: taken with triangles in force, and they were not set again since)
    const int k = R.last_ended;
    if (k < 0) return fail(SB_ERR_STATE, me + ": no readback has ended");
    if (!R.slot[k].has_normals)
        return fail(SB_ERR_STATE, me + ": the snapshot ended last has no triangles to query (taken without render triangles, or the render mode was set again since)");
    if (count == 0) return SB_OK;
    const bool embedded = R.slot[k].embedded;
    const float *xyz = embedded ? R.emb.pos[k].d.p : R.pos[k].d.p;
    const RenderTopology &T = embedded ? R.emb.topo : R.topo;
    const int m = (int)((embedded ? R.emb.tri.size() : R.tri.size()) / 3);
    ReadbackRaycast &Q = R.ray;                 // the ray cast's stream and buffers: a batch of queries is half a batch of rays, the hits and partials are the same size
    Q.prepare(acct);
    const int groups = (int)std::min<int64_t>(((int64_t)m + sbk::kRayLanes - 1) / sbk::kRayLanes, sbk::kRayMaxGroups);
    for (int64_t done = 0; done < count; done += sbk::kClosestBatch) {
        const int nb = (int)std::min<int64_t>(count - done, sbk::kClosestBatch);
        std::memcpy(Q.rays.h.p, queries + 4 * done, (size_t)nb * 4 * sizeof(float));
        HIP_CHECK(hipMemcpyAsync(Q.rays.d.p, Q.rays.h.p, (size_t)nb * 4 * sizeof(float), hipMemcpyHostToDevice, Q.stream));
        hipLaunchKernelGGL(sbk::closest_partial_kernel, dim3((unsigned)groups, (unsigned)((nb + sbk::kClosestTile - 1) / sbk::kClosestTile)), dim3(sbk::kRayLanes), 0, Q.stream, xyz,
                           T.d_tri.p, m, Q.rays.d.p, nb, Q.d_partials.p);
        hipLaunchKernelGGL(sbk::closest_final_kernel, dim3((unsigned)nb), dim3(sbk::kRayLanes), 0, Q.stream, Q.d_partials.p, groups, Q.hits.d.p);
        HIP_CHECK(hipGetLastError());
        Q.hits.copy_out(Q.stream, (size_t)nb);
        HIP_CHECK(hipStreamSynchronize(Q.stream));
        std::memcpy(hits_out + done, Q.hits.h.p, (size_t)nb * sizeof(sb_closest_hit));
    }
    return SB_OK;
}

}  // namespace sbi

// sb_readback_begin with an embedding set (SPEC.md 6b), slot k: the skinned visual mesh instead of the particles. The kernel reads the
// tick-end positions where they are -- the state, or a peek of the T0 tiles that hold a cage particle -- so no particle snapshot is taken.
static void begin_embedded(sb_solver *s, int k) {
    RenderState &R = s->render;
    RenderEmbedding &E = R.emb;
    if (E.dirty) {      // cage in device numbering, the distinct cage particles
        HIP_CHECK(hipStreamSynchronize(R.copy_stream));
        const std::vector<int32_t> &lof = local_of_old(s);
        std::vector<int4> cage((size_t)E.m);
        std::vector<uint8_t> seen((size_t)s->n_local, 0);
        s->cage_local.clear();
        for (int32_t r = 0; r < E.m; ++r) {
            int32_t l[4];
            for (int j = 0; j < 4; ++j) {
                l[j] = lof[(size_t)E.cage[4 * (size_t)r + j]];
                if (!seen[(size_t)l[j]]) { seen[(size_t)l[j]] = 1; s->cage_local.push_back(l[j]); }
            }
            cage[(size_t)r] = make_int4(l[0], l[1], l[2], l[3]);
        }
        E.upload(cage, s->dev_bytes);
        s->n_peek_tiles = -1;       // the peek's tile subset follows the cage particles
    }
    // skinning on the compute stream (ordered after every tick enqueued so far, before the next one) ...
    const float *src = tick_end_positions(s, /*subset=*/true, s->cage_local);
    launch_skin(s->stream, src, E.d_cage.p, E.d_w.p, E.pos[k].d.p, (int)E.m);
    HIP_CHECK(hipEventRecord(s->ev_snap[k], s->stream));
    // ... normals (SPEC.md 6a on the skinned array) and D2H on the copy stream
    HIP_CHECK(hipStreamWaitEvent(R.copy_stream, s->ev_snap[k], 0));
    E.pos[k].copy_out(R.copy_stream, (size_t)E.m * 3);
    R.slot[k] = RenderState::Slot{};
    R.slot[k].embedded = true;
    R.tan.snap_has[k] = false;
    if (!E.tri.empty()) launch_normals_stage(R.copy_stream, R, k, E.pos[k].d.p, (int)E.m, false, (size_t)E.m, s->dev_bytes);
    launch_bounds_stage(R.copy_stream, R.bnd, k, E.pos[k].d.p, nullptr, E.m, s->dev_bytes);      // SPEC.md 6d on the skinned vertices
    HIP_CHECK(hipEventRecord(R.ev_copied[k], R.copy_stream));
    ++R.pending;
}

extern "C" {

/* ---- asynchronous render readback -------------------------------------------- */

int sb_readback_begin(sb_solver *s) {
    if (!s) return fail(SB_ERR_INVALID_ARG, "sb_readback_begin: null handle");
    if (!s->finalized) return fail(SB_ERR_STATE, "sb_readback_begin before sb_finalize");
    if (s->render.pending == 2) return fail(SB_ERR_STATE, "sb_readback_begin: two snapshots already pending, call sb_readback_end");
    return guarded([&]() -> int {
        int rc = set_device(s); if (rc) return rc;
        RenderState &R = s->render;
        if (!R.ev_copied[kSnapSlots - 1]) {       // first use, keyed on what it creates last (create() is idempotent)
            R.copy_stream.create();
            for (int k = 0; k < kSnapSlots; ++k) {
                s->ev_snap[k].create(hipEventDisableTiming);
                R.ev_copied[k].create(hipEventDisableTiming);
            }
        }
        const int k = R.next_slot();
        if (R.emb.m > 0) { begin_embedded(s, k); return SB_OK; }       // (no particle snapshot: its n-sized buffers are not even allocated)
        const size_t n3 = (size_t)s->mesh->n * 3;
        if (!R.pos[kSnapSlots - 1].h.p) {      // first use: a slot counts as made once its pinned side is there, which comes last
            if (!s->d_local_to_old.p) s->d_local_to_old.upload(s->plan->local.local_to_old, s->dev_bytes);
            for (int q = 0; q < kSnapSlots; ++q) {
                if (R.pos[q].h.p) continue;
                R.pos[q].d.alloc(n3, s->dev_bytes);
                HIP_CHECK(hipMemset(R.pos[q].d.p, 0, n3 * sizeof(float)));
                R.pos[q].pin();
                std::memset(R.pos[q].h.p, 0, n3 * sizeof(float));
            }
        }
        // snapshot on the compute stream (ordered after every tick enqueued so far, before the next one) ...
        const bool compact = R.set_only && !R.tri.empty();
        // a rank of a partitioned solver serves the render particles it OWNS; vertex normals need the neighbours' particles too and are
        // computed on the gathered snapshot (sb_group_readback_*), not per rank
        const bool single = s->desc.world == 1;
        if (!R.tri.empty() && R.dirty) {     // the incident-triangle lists, and the render set: the particles they name that this rank owns
            HIP_CHECK(hipStreamSynchronize(R.copy_stream));
            const std::vector<int32_t> off = R.topo.upload(R.tri, s->mesh->n, s->dev_bytes);
            const std::vector<int32_t> &lof = local_of_old(s);
            R.set.clear(); s->render_local.clear();
            for (int32_t v = 0; v < s->mesh->n; ++v)
                if (off[(size_t)v + 1] > off[v] && lof[(size_t)v] >= 0 && lof[(size_t)v] < s->n_owned) { R.set.push_back(v); s->render_local.push_back(lof[(size_t)v]); }
            R.d_set.upload(R.set, s->dev_bytes);
            s->d_render_local.upload(s->render_local, s->dev_bytes);
            for (int q = 0; q < kSnapSlots; ++q) {
                if (single && !R.nrm[q].h.p) R.nrm[q].alloc(n3, s->dev_bytes);
                R.cpos[q].alloc(R.set.size() * 3, s->dev_bytes);
            }
            R.dirty = false;
            s->n_peek_tiles = -1;
        }
        // the tick's last kernel is deferred: snapshot a peek and leave it deferred
        const float *src = tick_end_positions(s, compact, s->render_local);
        const int cnt = (int)R.set.size();
        // compact: only the render set leaves the device. A single rank snapshots just those particles into the caller-numbered array (the
        // normals kernel gathers neighbours by caller id and emits the compact arrays); a partitioned rank has no normals: straight into the compact array
        if (!compact) launch_snapshot_all(s, src, s->d_local_to_old.p, R.pos[k].d.p);
        else if (single) launch_snapshot_subset(s, src, R.d_set.p, s->d_render_local.p, cnt, R.pos[k].d.p);
        else if (cnt) {
            sbk::PosView view = s->pos_view();
            view.xyz = const_cast<float *>(src);
            hipLaunchKernelGGL(sbk::snapshot_compact_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s->stream, view, s->d_render_local.p, R.cpos[k].d.p, cnt);
        }
        HIP_CHECK(hipEventRecord(s->ev_snap[k], s->stream));
        // ... D2H on the copy stream, overlapping whatever the compute stream does next
        HIP_CHECK(hipStreamWaitEvent(R.copy_stream, s->ev_snap[k], 0));
        if (!compact) R.pos[k].copy_out(R.copy_stream, n3);
        R.slot[k] = RenderState::Slot{};
        R.slot[k].compact = compact;
        R.slot[k].has_render_set = !R.tri.empty();
        R.tan.snap_has[k] = false;
        if (compact && !single) R.cpos[k].copy_out(R.copy_stream, (size_t)cnt * 3);
        if (!R.tri.empty() && single) launch_normals_stage(R.copy_stream, R, k, R.pos[k].d.p, compact ? cnt : (int)s->mesh->n, compact, (size_t)s->mesh->n, s->dev_bytes);
        // SPEC.md 6d on what this snapshot delivers: the compact array, or the rows of the full one this rank owns
        if (compact) launch_bounds_stage(R.copy_stream, R.bnd, k, R.cpos[k].d.p, nullptr, cnt, s->dev_bytes);
        else launch_bounds_stage(R.copy_stream, R.bnd, k, R.pos[k].d.p, single ? (const int32_t *)nullptr : s->d_local_to_old.p, single ? (int64_t)s->mesh->n : s->n_owned, s->dev_bytes);
        HIP_CHECK(hipEventRecord(R.ev_copied[k], R.copy_stream));
        ++R.pending;
        return SB_OK;
    });
}

int sb_readback_end(sb_solver *s, const float **pos_xyz_out) {
    if (!s || !pos_xyz_out) return fail(SB_ERR_INVALID_ARG, "sb_readback_end: null argument");
    if (s->render.pending == 0) return fail(SB_ERR_STATE, "sb_readback_end without a pending sb_readback_begin");
    return guarded([&]() -> int {
        int rc = set_device(s); if (rc) return rc;
        HIP_CHECK(hipEventSynchronize(s->render.ev_copied[s->render.head]));
        check_peer_error(s);       // (the snapshot was taken behind every tick enqueued before it)
        *pos_xyz_out = end_slot(s->render);
        return SB_OK;
    });
}

int sb_set_render_triangles(sb_solver *s, const int32_t *tri, int32_t m) {
    if (!s || m < 0 || (m > 0 && !tri)) return fail(SB_ERR_INVALID_ARG, "sb_set_render_triangles: bad argument");
    if (s->mesh->n <= 0) return fail(SB_ERR_STATE, "sb_set_render_triangles before sb_set_particles");
    if (s->render.pending) return fail(SB_ERR_STATE, "sb_set_render_triangles while a readback is pending");
    if (m > 0 && s->render.emb.m > 0)
        return fail(SB_ERR_STATE, "sb_set_render_triangles: a render embedding is set (switch it off first: sb_set_render_embedding with m_vertices = 0)");
    return guarded([&]() -> int { return set_render_triangles("sb_set_render_triangles", s->render, s->mesh->n, tri, m); });
}

int sb_set_render_embedding(sb_solver *s, const int32_t *cage_ijkl, const float *weights4, int32_t m_vertices, const int32_t *tri_abc, int32_t m_tri) {
    if (!s) return fail(SB_ERR_INVALID_ARG, "sb_set_render_embedding: null handle");
    if (s->desc.world > 1)
        return fail(SB_ERR_UNSUPPORTED, "sb_set_render_embedding: a rank of a partitioned solver does not hold every cage particle; a partitioned body is "
                    "skinned on the gathered snapshot (sb_group_set_render_embedding)");
    if (s->mesh->n <= 0) return fail(SB_ERR_STATE, "sb_set_render_embedding before sb_set_particles");
    if (s->render.pending) return fail(SB_ERR_STATE, "sb_set_render_embedding while a readback is pending");
    if (m_vertices > 0 && !s->render.tri.empty())
        return fail(SB_ERR_STATE, "sb_set_render_embedding: render triangles are set (switch them off first: sb_set_render_triangles with m = 0)");
    return guarded([&]() -> int {
        if (s->finalized) { int rc = set_device(s); if (rc) return rc; }
        const bool was_on = s->render.emb.m > 0;
        const int rc = set_render_embedding("sb_set_render_embedding", s->render, s->mesh->n, cage_ijkl, weights4, m_vertices, tri_abc, m_tri);
        if (rc == SB_OK && (was_on || m_vertices > 0)) s->n_peek_tiles = -1;
        return rc;
    });
}

int sb_readback_get_normals(sb_solver *s, const float **out) {
    if (!s || !out) return fail(SB_ERR_INVALID_ARG, "sb_readback_get_normals: null argument");
    if (s->desc.world > 1)
        return fail(SB_ERR_UNSUPPORTED, "sb_readback_get_normals: a rank of a partitioned solver does not hold its neighbours' particles; vertex normals of a partitioned "
                    "body are computed on the gathered snapshot (sb_group_readback_get_normals)");
    return readback_get_normals("sb_readback_get_normals", s->render, out);
}

int sb_set_render_uvs(sb_solver *s, const float *uv, int32_t count) {
    if (!s) return fail(SB_ERR_INVALID_ARG, "sb_set_render_uvs: null handle");
    if (s->desc.world > 1)
        return fail(SB_ERR_UNSUPPORTED, "sb_set_render_uvs: a rank of a partitioned solver does not hold its neighbours' particles; vertex tangents of a partitioned "
                    "body are computed on the gathered snapshot (sb_group_set_render_uvs)");
    return guarded([&]() -> int {
        if (s->finalized) { int rc = set_device(s); if (rc) return rc; }
        return set_render_uvs("sb_set_render_uvs", s->render, s->mesh->n, uv, count);
    });
}

int sb_readback_get_tangents(sb_solver *s, const float **out) {
    if (!s || !out) return fail(SB_ERR_INVALID_ARG, "sb_readback_get_tangents: null argument");
    if (s->desc.world > 1)
        return fail(SB_ERR_UNSUPPORTED, "sb_readback_get_tangents: a rank of a partitioned solver does not hold its neighbours' particles; vertex tangents of a partitioned "
                    "body are computed on the gathered snapshot (sb_group_readback_get_tangents)");
    return readback_get_tangents("sb_readback_get_tangents", s->render, out);
}

int sb_set_readback_bounds(sb_solver *s, int32_t enabled) {
    if (!s) return fail(SB_ERR_INVALID_ARG, "sb_set_readback_bounds: null handle");
    return set_readback_bounds("sb_set_readback_bounds", s->render, enabled);
}

int sb_readback_get_bounds(sb_solver *s, float lo_xyz[3], float hi_xyz[3]) {
    if (!s || !lo_xyz || !hi_xyz) return fail(SB_ERR_INVALID_ARG, "sb_readback_get_bounds: null argument");
    return readback_get_bounds("sb_readback_get_bounds", "sb_set_readback_bounds", s->render, lo_xyz, hi_xyz);
}

int sb_readback_raycast(sb_solver *s, const float *rays, int32_t count, sb_ray_hit *hits_out) {
    if (!s) return fail(SB_ERR_INVALID_ARG, "sb_readback_raycast: null handle");
    if (s->desc.world > 1)
        return fail(SB_ERR_UNSUPPORTED, "sb_readback_raycast: a rank of a partitioned solver does not hold its neighbours' particles; rays against a partitioned "
                    "body are cast on the gathered snapshot (sb_group_readback_raycast)");
    return guarded([&]() -> int {
        if (s->finalized) { int rc = set_device(s); if (rc) return rc; }
        return readback_raycast("sb_readback_raycast", s->render, rays, count, hits_out, s->dev_bytes);
    });
}

int sb_set_readback_render_set_only(sb_solver *s, int32_t on) {
    if (!s) return fail(SB_ERR_INVALID_ARG, "sb_set_readback_render_set_only: null handle");
    return set_readback_render_set_only("sb_set_readback_render_set_only", s->render, on);
}

int sb_readback_get_render_set(sb_solver *s, const int32_t **ids, int32_t *count) {
    if (!s || !ids || !count) return fail(SB_ERR_INVALID_ARG, "sb_readback_get_render_set: null argument");
    return readback_get_render_set("sb_readback_get_render_set", s->render, ids, count);
}

}  // extern "C"
