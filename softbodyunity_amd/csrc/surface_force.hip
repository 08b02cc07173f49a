// surface_force.hip — wind, air drag and pressure on the render triangles between two ticks (sb_group_apply_surface_forces, SPEC.md 2e): the
// validation of the record, the tables (built on the host at the first call after the triangles changed, released when they change) and
// the two launches (surface_force_kernels.hip.hpp: no other unit includes it). The entry point is the group's (group.hip, as for a
// placement: the solver's header is full); the rank path here takes the triangle list as an argument: a group keeps it, its rank does not.
#include "solver_internal.hpp"
#include "surface_force_kernels.hip.hpp"

using namespace sbi;

static_assert(sizeof(sb_surface_force) == 44, "sb_surface_force is 44 bytes (include/softbody_group.h)");

namespace sbi {

// The record alone, before anything is touched (SPEC.md 2e, "Errors"): needs neither a solver nor a device.
int validate_surface_force(const char *who, const sb_surface_force *f) {
    const std::string W = who;
    if (!f) return fail(SB_ERR_INVALID_ARG, W + ": null record");
    if (f->flags != 0) return fail(SB_ERR_INVALID_ARG, W + ": unknown flag bit (none is defined)");
    if (f->reserved[0] != 0 || f->reserved[1] != 0 || f->reserved[2] != 0) return fail(SB_ERR_INVALID_ARG, W + ": reserved must be 0");
    for (int c = 0; c < 3; ++c) if (!std::isfinite(f->wind[c])) return fail(SB_ERR_INVALID_ARG, W + ": NaN or infinite wind");
    if (!std::isfinite(f->normal) || f->normal < 0.0f) return fail(SB_ERR_INVALID_ARG, W + ": normal must be finite and not negative");
    if (!std::isfinite(f->tangential) || f->tangential < 0.0f) return fail(SB_ERR_INVALID_ARG, W + ": tangential must be finite and not negative");
    if (!std::isfinite(f->pressure)) return fail(SB_ERR_INVALID_ARG, W + ": NaN or infinite pressure");
    if (!std::isfinite(f->dt) || !(f->dt > 0.0f)) return fail(SB_ERR_INVALID_ARG, W + ": dt must be finite and positive");
    return SB_OK;
}

// When the render triangles change (no kernel of an earlier call may still read a table that goes)
void release_surface_tables(sb_solver *s) {
    SurfaceForceTables &T = s->surf;
    if (!T.bytes) return;
    (void)hipSetDevice(s->desc.device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    T.d_tri.free(); T.d_part.free(); T.d_off.free(); T.d_adj.free(); T.d_J.free();
    s->dev_bytes -= T.bytes;
    T.bytes = 0; T.m = 0; T.n_part = 0;
}

namespace {

// The tables of `tri` (the rank's numbering, m triangles): built into locals and moved into place at the end (device_handles.hpp, FIRST USE)
void build_surface_tables(sb_solver *s, const int32_t *tri, int64_t m) {
    const std::vector<int32_t> &lof = local_of_old(s);
    std::vector<int32_t> dtri((size_t)(3 * m));
    for (int64_t c = 0; c < 3 * m; ++c) {
        const int32_t l = lof[(size_t)tri[c]];
        if (l < 0 || l >= s->n_owned) throw std::runtime_error("surface forces: a render triangle names a particle this solver does not own");
        dtri[(size_t)c] = l;
    }
    // the render particles in ascending device order, each with the list of its incident triangles: ascending t, one entry per corner slot
    // (what RenderTopology::upload builds in caller numbering for the normals)
    std::vector<int32_t> count((size_t)s->n_local + 1, 0);
    for (int32_t l : dtri) ++count[(size_t)l + 1];
    std::vector<int32_t> part, off, slot((size_t)s->n_local, -1);
    for (int64_t l = 0; l < s->n_local; ++l)
        if (count[(size_t)l + 1]) { slot[(size_t)l] = (int32_t)part.size(); part.push_back((int32_t)l); off.push_back(0); }
    off.push_back(0);
    for (size_t k = 0; k < part.size(); ++k) off[k + 1] = off[k] + count[(size_t)part[k] + 1];
    std::vector<int32_t> cur(off.begin(), off.end() - 1), adj((size_t)(3 * m));
    for (int64_t t = 0; t < m; ++t)
        for (int j = 0; j < 3; ++j) adj[(size_t)cur[(size_t)slot[(size_t)dtri[(size_t)(3 * t + j)]]]++] = (int32_t)t;
    SurfaceForceTables T;
    T.d_tri.upload(dtri, T.bytes); T.d_part.upload(part, T.bytes); T.d_off.upload(off, T.bytes); T.d_adj.upload(adj, T.bytes);
    T.d_J.alloc((size_t)m, T.bytes);
    T.m = m; T.n_part = (int64_t)part.size();
    s->surf = std::move(T);
    s->dev_bytes += s->surf.bytes;
}

}  // namespace

bool surface_tables_built(const sb_solver *s) { return s->surf.bytes != 0; }

// The rank path: a validated record on a solver that holds the whole body (world == 1). tri: m render triangles in the rank's numbering,
// read only while the tables are not built. Completes the tick first -- velocities exist only once its last kernel has run -- which also
// lands pending kinematic targets. Asynchronous on s->stream.
int apply_surface_forces_validated(sb_solver *s, const sb_surface_force &f, const int32_t *tri, int64_t m) {
    int rc = set_device(s); if (rc) return rc;
    if (!surface_tables_built(s)) build_surface_tables(s, tri, m);
    const SurfaceForceTables &T = s->surf;
    sbk::SurfaceForceParams P;
    P.wx = f.wind[0]; P.wy = f.wind[1]; P.wz = f.wind[2];
    const float an = f.dt * f.normal, at = f.dt * f.tangential, ap = f.dt * f.pressure;
    P.hn = an / 6.0f; P.ht = at / 6.0f; P.hp = ap / 6.0f;
    flush_deferred(s);
    hipLaunchKernelGGL(sbk::surface_force_triangle_kernel, dim3((unsigned)((T.m + 255) / 256)), dim3(256), 0, s->stream, s->pos_view(), (const float *)s->d_vel.p,
                       (const int32_t *)T.d_tri.p, T.d_J.p, (int)T.m, P);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sbk::surface_force_vertex_kernel, dim3((unsigned)((T.n_part + 255) / 256)), dim3(256), 0, s->stream, s->pos_view(), s->d_vel.p,
                       (const int32_t *)T.d_part.p, (const int32_t *)T.d_off.p, (const int32_t *)T.d_adj.p, (const float4 *)T.d_J.p, (int)T.n_part);
    HIP_CHECK(hipGetLastError());
    return SB_OK;
}

}  // namespace sbi
