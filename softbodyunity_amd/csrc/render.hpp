// render.hpp — the render readback's state and stage, shared by a solver (render.hip) and by a group's render device (group.hip): snapshot
// slots, device buffers with their pinned twins, incident-triangle lists, the embedding, tangents, bounds. Included by solver_internal.hpp
// (after device_handles.hpp: every buffer, stream and event here gives itself back, with the owner's device current); plain structs and free functions, the owner passes what differs (a count, a pointer, a stream).
//
// No reference counterpart exists (/root/reference/README.md:1 is the whole reference tree).
#pragma once

struct sb_solver;

namespace sbi {

// three slots, at most two pending: the slot a readback_end handed out last is never the next one to be filled, so its pointer stays
// valid until the SECOND readback_begin after it (softbody.h, softbody_group.h)
constexpr int kSnapSlots = 3;

// Render tangents (sb_set_render_uvs, SPEC.md 6c): the UVs of the render mode in force, the per-triangle coefficient table made from
// them, and per snapshot slot the tangents on the device and in pinned memory.
struct RenderTangents {
    std::vector<float> uv;                 // 2 floats per vertex of the render mode in force; empty = tangents off
    bool dirty = false;                    // UVs changed since the coefficient table was uploaded
    DevBuf<float4> d_k;                    // (dv2, dv1, du1, du2) / det per triangle, zeros for a UV-degenerate one
    Mirror<float4> tan[kSnapSlots];
    size_t rows = 0;                       // capacity of every slot's buffers
    bool snap_has[kSnapSlots] = {false, false, false};
    bool on() const { return !uv.empty(); }
    void release() {                       // device and pinned buffers (no readback is pending when the UVs or the render mode change)
        d_k.free();
        for (auto &t : tan) t.release();
        rows = 0;
    }
    void clear() {                         // tangents off: what every set_render_triangles / set_render_embedding does
        std::vector<float>().swap(uv);
        dirty = false;
        for (bool &b : snap_has) b = false;
        release();
    }
    // before a readback that computes tangents: the coefficient table of `tri` and buffers of at least n_rows rows
    void prepare(const std::vector<int32_t> &tri, size_t n_rows, int64_t &acct);
};

// Bounding box (sb_set_readback_bounds / sb_get_bounds, SPEC.md 6d): per snapshot slot -- and once more for the synchronous query, which
// runs on another stream -- the box on the device and in pinned memory, 8 floats: lo.xyz, 0, hi.xyz, 0.
struct ReadbackBounds {
    static constexpr int kQuerySlot = kSnapSlots;
    bool enabled = false;                  // readbacks begun from now on carry a box
    DevBuf<float> d_partials;              // the workgroups' boxes: one set for the copy stream, one for the query
    Mirror<float> box;                     // 8 floats per slot
    bool snap_has[kSnapSlots] = {false, false, false};
    void prepare(int64_t &acct);           // buffers, at first use
    void read(int slot, float lo[3], float hi[3]) const { for (int c = 0; c < 3; ++c) { lo[c] = box.h.p[8 * slot + c]; hi[c] = box.h.p[8 * slot + 4 + c]; } }
};

// Ray casts (sb_readback_raycast, SPEC.md 6e): a stream of its own -- a cast waits for no pending snapshot's copy -- and, from the first cast
// on, the buffers of one batch of rays: the rays and the hits with their pinned twins, the workgroups' partials. Larger counts walk in batches.
// Closest-point queries (SPEC.md 6g) are synchronous on the same stream and stage their batches in the same buffers (first cast or query).
struct ReadbackRaycast {
    Stream stream;
    Mirror<float> rays;                    // 8 floats per ray of a batch (the pinned side is the staging of the upload)
    Mirror<uint4> hits;                    // one sb_ray_hit per ray of a batch
    DevBuf<uint4> d_partials;              // (key, u, v) per (ray, workgroup)
    void prepare(int64_t &acct);           // buffers and stream, at first use
};

// Triangles and the incident-triangle lists per vertex (triangle ids ascending: what the normals kernels walk), on the device.
struct RenderTopology {
    DevBuf<int32_t> d_tri, d_adj_off, d_adj_tri;
    // -> the lists' offsets [n_vertices + 1]: vertex v is used by a triangle where off[v + 1] > off[v]
    std::vector<int32_t> upload(const std::vector<int32_t> &tri, int32_t n_vertices, int64_t &acct);
    void release() { d_tri.free(); d_adj_off.free(); d_adj_tri.free(); }      // (RenderEmbedding::release)
};

// Embedded render vertices (set_render_embedding, SPEC.md 6b): while m > 0 a readback brings the skinned visual mesh instead of the
// particles. Excludes the render triangles (either mode is switched off before the other is set).
struct RenderEmbedding {
    int32_t m = 0;                         // render vertices (0 = off)
    std::vector<int32_t> cage, tri;        // as given: 4 particles per vertex (caller numbering), triangles over the render vertices
    std::vector<float> w;                  // 4 weights per vertex
    bool dirty = false;                    // changed since the last upload
    DevBuf<int4> d_cage;                   // in the numbering of the array the skin kernel reads
    DevBuf<float4> d_w;
    RenderTopology topo;
    Mirror<float> pos[kSnapSlots], nrm[kSnapSlots];
    void release() {                       // device and pinned buffers (no readback is pending when the embedding changes)
        d_cage.free(); d_w.free(); topo.release();
        for (int k = 0; k < kSnapSlots; ++k) { pos[k].release(); nrm[k].release(); }
    }
    // first use after a change: the cage (translated by the owner into the numbering of the skin kernel's source), weights, lists, slots
    void upload(const std::vector<int4> &cage_in_source_numbering, int64_t &acct);
};

// Everything a solver and a group's render device both keep for the render readback.
struct RenderState {
    Stream copy_stream;                    // normals, tangents, bounds and every copy to the host run here, in order (the bounds partials rely on it)
    Event ev_copied[kSnapSlots];
    int head = 0, pending = 0;             // ring: slots head .. head + pending - 1 (mod kSnapSlots) are in flight
    int last_ended = -1;
    struct Slot { bool compact = false, has_normals = false, has_render_set = false, embedded = false; } slot[kSnapSlots];
    int next_slot() const { return (head + pending) % kSnapSlots; }
    // render triangles (set_render_triangles): particles in caller numbering
    std::vector<int32_t> tri;
    bool dirty = false;                    // triangles changed since the last upload
    bool set_only = false;                 // readbacks bring the render set only (compact positions + normals)
    std::vector<int32_t> set;              // the particles the triangles use (a solver: and this rank owns), ascending
    RenderTopology topo;
    DevBuf<int32_t> d_set;
    Mirror<float> pos[kSnapSlots];         // packed xyz in caller numbering: the snapshot (a group: gathered from every rank)
    Mirror<float> nrm[kSnapSlots];
    Mirror<float> cpos[kSnapSlots];        // compact positions of the render set
    RenderEmbedding emb;
    RenderTangents tan;                    // of either mode
    ReadbackBounds bnd;                    // of the delivered array, and of the synchronous query
    ReadbackRaycast ray;                   // casts against the snapshot ended last
    void forget_normals() { for (Slot &q : slot) q.has_normals = q.has_render_set = false; }
};

// ---- render.hip: the kernels' launch helpers (dst of a snapshot may live on another device) ----------------------------------------------
void launch_snapshot_all(sb_solver *s, const float *src_xyz, const int32_t *d_target_of_local, float *dst_xyz);
void launch_snapshot_subset(sb_solver *s, const float *src_xyz, const int32_t *d_ids, const int32_t *d_local, int count, float *dst_xyz);
void launch_skin(hipStream_t st, const float *src_xyz, const int4 *cage, const float4 *weights, float *out_xyz, int m);
// SPEC.md 6d on stream st: the box of rows rows[0 .. count) (rows == nullptr: 0 .. count) of a packed xyz array -> the slot's 8 floats on the
// device, then 32 bytes to the slot's pinned memory. count == 0 gives the empty box.
void launch_bounds(hipStream_t st, ReadbackBounds &B, int slot, const float *xyz, const int32_t *rows, int64_t count, int64_t &acct);

// ---- render.hip: the stage behind "slot k's packed xyz array is on stream st" ------------------------------------------------------------
// Normals (with tangents where UVs are set, SPEC.md 6a / 6c) of `count` vertices of xyz -- of the embedding's triangles where the slot is
// embedded, else of the render triangles; compact: the rows of the render set, whose positions leave in the compact array too -- and
// their copies to pinned memory. tan_rows: what the tangent buffers are sized by. Sets the slot's flags.
void launch_normals_stage(hipStream_t st, RenderState &R, int k, const float *xyz, int count, bool compact, size_t tan_rows, int64_t &acct);
// the slot's bounding box, where bounds are on
void launch_bounds_stage(hipStream_t st, ReadbackBounds &B, int k, const float *xyz, const int32_t *rows, int64_t count, int64_t &acct);
// readback_end, once the slot's copies have arrived: what it hands out, and the ring moves on
const float *end_slot(RenderState &R);

// ---- render.hip: what sb_* and sb_group_* entry points share behind their own preconditions (who = the entry point's name) ----------------
int set_render_triangles(const char *who, RenderState &R, int32_t n, const int32_t *tri, int32_t m);
// (n = particles the cage may name, or the triangles, or -- one UV pair each -- the render triangles' vertices)
int set_render_embedding(const char *who, RenderState &R, int32_t n, const int32_t *cage_ijkl, const float *weights4, int32_t m_vertices, const int32_t *tri_abc, int32_t m_tri);
int set_render_uvs(const char *who, RenderState &R, int32_t n, const float *uv, int32_t count);
int set_readback_bounds(const char *who, RenderState &R, int32_t enabled);
int set_readback_render_set_only(const char *who, RenderState &R, int32_t on);
int readback_get_normals(const char *who, RenderState &R, const float **out);
int readback_get_tangents(const char *who, RenderState &R, const float **out);
int readback_get_bounds(const char *who, const char *setter, RenderState &R, float lo_xyz[3], float hi_xyz[3]);      // setter: the name the message points to
int readback_get_render_set(const char *who, RenderState &R, const int32_t **ids, int32_t *count);
// SPEC.md 6e behind the owner's null-handle, world and device preconditions: `count` rays against the snapshot ended last, synchronous
int readback_raycast(const char *who, RenderState &R, const float *rays, int32_t count, sb_ray_hit *hits_out, int64_t &acct);
// SPEC.md 6g, the ray cast's twin on its stream and in its buffers: `count` queries (x, y, z, max_distance) against the snapshot ended last
int readback_closest_points(const char *who, RenderState &R, const float *queries, int32_t count, sb_closest_hit *hits_out, int64_t &acct);

}  // namespace sbi
