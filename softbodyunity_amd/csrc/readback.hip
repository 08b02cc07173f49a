// readback.hip — state reads and writes, the bounding box of the state, kinematic targets, and where the tick-end positions are for whoever reads them (the render readback itself: render.hip)
//
// No reference counterpart exists (/root/reference/README.md:1 is the whole reference tree); the exported functions are the
// [BUILDER-DEFINED] boundary of SURVEY.md §8b (include/softbody*.h).
#include "solver_internal.hpp"

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

// Where the tick-end positions are, made valid on the solver's stream (synchronising is the caller's): while the tick's last kernel is held
// back that is a PEEK into the side array -- every T0 tile, or (subset) only the tiles that hold a particle of `wanted_local`, a list built
// once per render set -- with the pending kinematic targets scattered onto it (they show in what is read and stay pending); else the state
// itself after the tick has been completed. The tick stays fusable with the next one after a peek, on every rank of a partitioned solver
// too: the held-back kernel runs on T0 tiles, which hold owned particles only and need no ghost.
const float *tick_end_positions(sb_solver *s, bool subset, const std::vector<int32_t> &wanted_local) {
    if (!can_peek(s)) { flush_deferred(s); return s->d_pos3.p; }
    if (subset && s->n_peek_tiles < 0) build_peek_subset(s, wanted_local);
    peek_positions(s, subset);
    if (s->kin_pending >= 0) scatter_kinematic(s, s->d_peek.p);
    return s->d_peek.p;
}

// Positions (or velocities, which exist only once the tick is complete) of the particles this rank OWNS, written into `out` at their
// caller index (id_map: see scatter_owned); entries of other ranks' particles are left alone.
int get_state_owned(sb_solver *s, float *out, bool velocity, const int32_t *id_map) {
    int rc = set_device(s); if (rc) return rc;
    if (velocity) flush_deferred(s);
    const float *src = velocity ? s->d_vel.p : tick_end_positions(s);
    if (s->desc.world == 1) {
        // single rank: every entry is ours, so the permutation to caller numbering runs on the GPU and one copy
        // lands in the caller's array (a host-side scatter costs 25 ms for 16.7 M particles)
        if (!s->d_local_to_old.p) s->d_local_to_old.upload(s->plan->local.local_to_old, s->dev_bytes);
        if (!s->d_get_scratch.p) s->d_get_scratch.alloc((size_t)s->mesh->n * 3, s->dev_bytes);
        launch_snapshot_all(s, src, s->d_local_to_old.p, s->d_get_scratch.p);
        HIP_CHECK(hipMemcpyAsync(out, s->d_get_scratch.p, (size_t)s->mesh->n * 3 * sizeof(float), hipMemcpyDeviceToHost, s->stream));
        HIP_CHECK(hipStreamSynchronize(s->stream));
        return SB_OK;
    }
    HIP_CHECK(hipStreamSynchronize(s->stream));
    check_peer_error(s);
    s->h_stage.resize((size_t)s->n_owned * 3);
    if (s->n_owned) HIP_CHECK(hipMemcpy(s->h_stage.data(), src, (size_t)s->n_owned * 3 * sizeof(float), hipMemcpyDeviceToHost));
    scatter_owned(s, s->h_stage.data(), out, id_map);       // (world > 1: the caller merges the ranks' arrays)
    return SB_OK;
}

}  // namespace sbi

static int get_state(sb_solver *s, float *out, int32_t n, bool velocity) {
    if (!s || !out) return fail(SB_ERR_INVALID_ARG, "sb_get_*: null argument");
    if (!s->finalized) return fail(SB_ERR_STATE, "sb_get_* before sb_finalize");
    if (n != s->mesh->n) return fail(SB_ERR_INVALID_ARG, "sb_get_*: n differs from sb_set_particles");
    return guarded([&]() -> int { return get_state_owned(s, out, velocity, nullptr); });
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
        s->local_of_old.assign((size_t)s->mesh->n, -1);
        for (size_t l = 0; l < L.local_to_old.size(); ++l) s->local_of_old[(size_t)L.local_to_old[l]] = (int32_t)l;
    }
    return s->local_of_old;
}

// sb_get_bounds: on what sb_get_positions would return now
int get_bounds_owned(sb_solver *s, float lo[3], float hi[3]) {
    int rc = set_device(s); if (rc) return rc;
    const float *xyz = tick_end_positions(s);
    launch_bounds(s->stream, s->render.bnd, ReadbackBounds::kQuerySlot, xyz, nullptr, s->n_owned, s->dev_bytes);
    HIP_CHECK(hipStreamSynchronize(s->stream));
    check_peer_error(s);
    s->render.bnd.read(ReadbackBounds::kQuerySlot, lo, hi);
    return SB_OK;
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
    if (s->kin_seen.size() != (size_t)s->mesh->n) s->kin_seen.assign((size_t)s->mesh->n, 0);
    const uint32_t stamp = ++s->kin_stamp;
    int32_t n_mine = 0;
    for (int32_t k = 0; k < count; ++k) {
        if (ids[k] < 0 || ids[k] >= s->mesh->n) return fail(SB_ERR_INVALID_ARG, "sb_set_kinematic_positions: particle index out of range");
        if (s->mesh->invm[(size_t)ids[k]] != 0.0f)
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
    const size_t pos_at = sb_solver::kin_table_pos_at(n_mine);
    const int q = s->kin_ring.acquire(pos_at + (size_t)n_mine * 3 * sizeof(float));
    int32_t *h_idx = (int32_t *)s->kin_ring.host(q);
    float *h_pos = (float *)(s->kin_ring.host(q) + pos_at);
    int32_t w = 0;
    for (int32_t k = 0; k < count; ++k) {
        const int32_t l = lof[(size_t)ids[k]];
        if (l < 0 || l >= s->n_owned) continue;
        h_idx[w] = l;
        for (int c = 0; c < 3; ++c) h_pos[3 * (size_t)w + c] = pos[3 * (size_t)k + c];
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
    if (n != s->mesh->n) return fail(SB_ERR_INVALID_ARG, "sb_set_state: n differs from sb_set_particles");
    return guarded([&]() -> int { return set_state_from(s, pos, vel, nullptr); });
}

int sb_set_kinematic_positions(sb_solver *s, const int32_t *ids, const float *pos, int32_t count) {
    if (!s || count < 0 || (count > 0 && (!ids || !pos))) return fail(SB_ERR_INVALID_ARG, "sb_set_kinematic_positions: bad argument");
    if (!s->finalized) return fail(SB_ERR_STATE, "sb_set_kinematic_positions before sb_finalize");
    if (count == 0) return SB_OK;
    return guarded([&]() -> int { return set_kinematic(s, ids, pos, count); });
}

int sb_get_bounds(sb_solver *s, float lo_xyz[3], float hi_xyz[3]) {
    if (!s || !lo_xyz || !hi_xyz) return fail(SB_ERR_INVALID_ARG, "sb_get_bounds: null argument");
    if (!s->finalized) return fail(SB_ERR_STATE, "sb_get_bounds before sb_finalize");
    return guarded([&]() -> int { return get_bounds_owned(s, lo_xyz, hi_xyz); });
}

}  // extern "C"
