// collide.hip — collider contacts between two ticks (sb_group_collide, SPEC.md 2f): the validation of the list and the launches of the one
// pass (collide_kernels.hip.hpp: no other unit includes it), a batch of records per launch, in list order; and the same with what the
// body gives back to each collider (sb_group_collide_reactions, SPEC.md 2g): the reacting pass and the launches that add its rows up.
// The group's entry points (group.hip) validate once and hand the same list to every rank.
#include "solver_internal.hpp"
#include "collide_kernels.hip.hpp"

using namespace sbi;

static_assert(sizeof(sb_collider) == 128, "sb_collider is 128 bytes (include/softbody_group.h)");
static_assert(sizeof(sbk::ColliderRec) == sizeof(sb_collider) && offsetof(sbk::ColliderRec, a) == offsetof(sb_collider, a) &&
                  offsetof(sbk::ColliderRec, rot) == offsetof(sb_collider, rot) && offsetof(sbk::ColliderRec, half) == offsetof(sb_collider, half) &&
                  offsetof(sbk::ColliderRec, radius) == offsetof(sb_collider, radius) && offsetof(sbk::ColliderRec, lin) == offsetof(sb_collider, lin) &&
                  offsetof(sbk::ColliderRec, friction) == offsetof(sb_collider, friction) && offsetof(sbk::ColliderRec, reserved) == offsetof(sb_collider, reserved),
              "ColliderRec is sb_collider");
static_assert(sizeof(sb_collider_reaction) == sbk::kReactSlots * sizeof(double) && offsetof(sb_collider_reaction, angular_impulse) == 3 * sizeof(double) &&
                  offsetof(sb_collider_reaction, contact_mass) == 6 * sizeof(double) && offsetof(sb_collider_reaction, n_contacts) == sbk::kReactSums * sizeof(double),
              "a collider's slots of a row are sb_collider_reaction");
static_assert(SB_COLLIDE_REACTIONS_MAX % sbk::kColliderBatch == 0, "every batch writes whole records of the result");
static_assert(sbk::kColliderSphere == SB_COLLIDER_SPHERE && sbk::kColliderCapsule == SB_COLLIDER_CAPSULE && sbk::kColliderBox == SB_COLLIDER_BOX, "shape codes");

namespace sbi {

// The list alone, before anything is touched (SPEC.md 2f, "Errors"): needs neither a group nor a device.
int validate_colliders(const char *who, const sb_collider *colliders, int32_t count) {
    const std::string W = who;
    if (count < 0) return fail(SB_ERR_INVALID_ARG, W + ": negative count");
    if (count > 0 && !colliders) return fail(SB_ERR_INVALID_ARG, W + ": null colliders");
    for (int32_t i = 0; i < count; ++i) {
        const sb_collider &c = colliders[i];
        const std::string at = W + ": collider " + std::to_string(i) + ": ";
        if (c.shape != SB_COLLIDER_SPHERE && c.shape != SB_COLLIDER_CAPSULE && c.shape != SB_COLLIDER_BOX) return fail(SB_ERR_INVALID_ARG, at + "unknown shape");
        if (c.flags != 0) return fail(SB_ERR_INVALID_ARG, at + "flags must be 0");
        for (int32_t r : c.reserved)
            if (r != 0) return fail(SB_ERR_INVALID_ARG, at + "reserved must be 0");
        const float *f = c.a;      // a .. restitution: 27 floats side by side (the static_asserts above)
        for (size_t k = 0; k < (offsetof(sb_collider, reserved) - offsetof(sb_collider, a)) / sizeof(float); ++k)
            if (!std::isfinite(f[k])) return fail(SB_ERR_INVALID_ARG, at + "NaN or infinite value");
        if (c.radius < 0.0f) return fail(SB_ERR_INVALID_ARG, at + "negative radius");
        for (float h : c.half)
            if (h < 0.0f) return fail(SB_ERR_INVALID_ARG, at + "negative half extent");
        if (c.friction < 0.0f) return fail(SB_ERR_INVALID_ARG, at + "negative friction");
        if (c.restitution < 0.0f || c.restitution > 1.0f) return fail(SB_ERR_INVALID_ARG, at + "restitution outside [0, 1]");
    }
    return SB_OK;
}

// The rank path: a validated list (count > 0) applied to every particle this rank holds, ghosts included -- the same arithmetic on a
// ghost gives its owner's bits, so no exchange follows. Completes the tick first, which lands pending kinematic targets. One launch per
// batch of kColliderBatch records, in list order on the rank's stream: the state a batch leaves is the next one's input. The records
// travel as kernel arguments (copied by the launch), so the caller's list is not read after the call returns. Asynchronous.
int collide_validated(sb_solver *s, const sb_collider *colliders, int32_t count) {
    int rc = set_device(s); if (rc) return rc;
    flush_deferred(s);
    if (s->n_local == 0) return SB_OK;
    const int64_t n = s->n_local, lanes = n / sbk::kCollidePerLane + n % sbk::kCollidePerLane;
    const dim3 grid((unsigned)((lanes + sbk::kCollideLanes - 1) / sbk::kCollideLanes));
    for (int32_t first = 0; first < count; first += sbk::kColliderBatch) {
        const int m = (int)std::min<int32_t>(sbk::kColliderBatch, count - first);
        sbk::ColliderBatch B;
        std::memset(&B, 0, sizeof(B));
        std::memcpy(B.c, colliders + first, (size_t)m * sizeof(sb_collider));
        hipLaunchKernelGGL(sbk::collide_kernel, grid, dim3(sbk::kCollideLanes), 0, s->stream, s->d_pos3.p, s->d_vel.p, (const float *)s->d_wf.p, n, m, B);
        HIP_CHECK(hipGetLastError());
    }
    return SB_OK;
}

// SPEC.md 2g. collide_validated's launches with the reacting pass in collide_kernel's place -- the same grid, the same statements on x and
// v -- and behind each batch the sums of its colliders: the workgroups' rows are added in row order, by one workgroup for up to
// kReactRowsPerGroup rows, else in TWO LEVELS (a workgroup per kReactRowsPerGroup rows, then one over those: 256^3 is 16 384 rows, then
// 256), and the last level writes the batch's records into the mapped pinned result, in stream order. The event behind the last batch
// is what get_collider_reactions_owned waits for. First use allocates the rows (1 KiB + 4 bytes per workgroup, and per first-level
// workgroup) and the result.
int collide_reactions_validated(sb_solver *s, const sb_collider *colliders, int32_t count) {
    int rc = set_device(s); if (rc) return rc;
    const int64_t n = s->n_local, lanes = n / sbk::kCollidePerLane + n % sbk::kCollidePerLane;
    const int n_rows = (int)((lanes + sbk::kCollideLanes - 1) / sbk::kCollideLanes);
    const int n_rows1 = n_rows > sbk::kReactRowsPerGroup ? (n_rows + sbk::kReactRowsPerGroup - 1) / sbk::kReactRowsPerGroup : 0;
    if (!s->h_react.p) {      // keyed on what is made last (device_handles.hpp)
        s->d_react_rows.alloc((size_t)sbk::kReactRow * (size_t)n_rows, s->dev_bytes);
        s->d_react_masks.alloc((size_t)n_rows, s->dev_bytes);
        s->d_react_rows1.alloc((size_t)sbk::kReactRow * (size_t)n_rows1, s->dev_bytes);
        s->d_react_masks1.alloc((size_t)n_rows1, s->dev_bytes);
        s->ev_react.create(hipEventDisableTiming | hipEventReleaseToSystem);       // the records are host memory
        s->h_react.alloc((size_t)SB_COLLIDE_REACTIONS_MAX * sbk::kReactSlots, /*mapped=*/true);
    }
    flush_deferred(s);
    for (int32_t first = 0; first < count; first += sbk::kColliderBatch) {
        const int m = (int)std::min<int32_t>(sbk::kColliderBatch, count - first);
        if (n_rows) {
            sbk::ColliderBatch B;
            std::memset(&B, 0, sizeof(B));
            std::memcpy(B.c, colliders + first, (size_t)m * sizeof(sb_collider));
            hipLaunchKernelGGL(sbk::collide_react_kernel, dim3((unsigned)n_rows), dim3(sbk::kCollideLanes), 0, s->stream, s->d_pos3.p, s->d_vel.p, (const float *)s->d_wf.p, n,
                               s->n_owned, m, B, s->d_react_rows.p, s->d_react_masks.p);
        }
        double *out = s->h_react.dev + (size_t)first * sbk::kReactSlots;
        if (n_rows1) {
            hipLaunchKernelGGL(sbk::collide_react_final_kernel, dim3((unsigned)n_rows1), dim3(sbk::kReactFinalLanes), 0, s->stream, (const double *)s->d_react_rows.p,
                               (const uint32_t *)s->d_react_masks.p, n_rows, sbk::kReactRowsPerGroup, s->d_react_rows1.p, s->d_react_masks1.p, m);
            hipLaunchKernelGGL(sbk::collide_react_final_kernel, dim3(1), dim3(sbk::kReactFinalLanes), 0, s->stream, (const double *)s->d_react_rows1.p,
                               (const uint32_t *)s->d_react_masks1.p, n_rows1, n_rows1, out, (uint32_t *)nullptr, m);
        } else
            hipLaunchKernelGGL(sbk::collide_react_final_kernel, dim3(1), dim3(sbk::kReactFinalLanes), 0, s->stream, (const double *)s->d_react_rows.p,
                               (const uint32_t *)s->d_react_masks.p, n_rows, n_rows, out, (uint32_t *)nullptr, m);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipEventRecord(s->ev_react, s->stream));
    return SB_OK;
}

int get_collider_reactions_owned(sb_solver *s, sb_collider_reaction *out, int32_t count) {
    int rc = set_device(s); if (rc) return rc;
    if (!s->h_react.p) return fail(SB_ERR_STATE, "sb_group_get_collider_reactions: this rank holds no reactions");
    HIP_CHECK(hipEventSynchronize(s->ev_react));       // the collide launches and their sums: nothing else is completed
    std::memcpy(out, s->h_react.p, (size_t)count * sizeof(sb_collider_reaction));
    return SB_OK;
}

}  // namespace sbi
