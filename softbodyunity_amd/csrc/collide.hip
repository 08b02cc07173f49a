// collide.hip — collider contacts between two ticks (sb_group_collide, SPEC.md 2f): the validation of the list and the launches of the one
// pass (collide_kernels.hip.hpp: no other unit includes it), a batch of records per launch, in list order. The group's entry point
// (group.hip) validates once and hands the same list to every rank.
#include "solver_internal.hpp"
#include "collide_kernels.hip.hpp"

using namespace sbi;

static_assert(sizeof(sb_collider) == 128, "sb_collider is 128 bytes (include/softbody_group.h)");
static_assert(sizeof(sbk::ColliderRec) == sizeof(sb_collider) && offsetof(sbk::ColliderRec, a) == offsetof(sb_collider, a) &&
                  offsetof(sbk::ColliderRec, rot) == offsetof(sb_collider, rot) && offsetof(sbk::ColliderRec, half) == offsetof(sb_collider, half) &&
                  offsetof(sbk::ColliderRec, radius) == offsetof(sb_collider, radius) && offsetof(sbk::ColliderRec, lin) == offsetof(sb_collider, lin) &&
                  offsetof(sbk::ColliderRec, friction) == offsetof(sb_collider, friction) && offsetof(sbk::ColliderRec, reserved) == offsetof(sb_collider, reserved),
              "ColliderRec is sb_collider");
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

}  // namespace sbi
