// placement.hip — placement between two ticks (sb_group_place, SPEC.md 2d): the validation of the struct, the first-use upload of the
// reference pose of every local particle, and the launch of the one pass (placement_kernels.hip.hpp: no other unit includes it). The
// group's entry point (group.hip) validates once and hands the same struct to every rank.
#include "solver_internal.hpp"
#include "placement_kernels.hip.hpp"

using namespace sbi;

static_assert(sizeof(sb_placement) == 92, "sb_placement is 92 bytes (include/softbody_group.h)");
static_assert(sizeof(sbk::PlaceMap) == sizeof(sb_placement) - 2 * sizeof(uint32_t) && offsetof(sb_placement, m) == 2 * sizeof(uint32_t),
              "PlaceMap is sb_placement behind its flags and reserved words");

namespace sbi {

// The struct alone, before anything is touched (SPEC.md 2d, "Errors"): needs neither a group nor a device.
int validate_placement(const char *who, const sb_placement *p) {
    const std::string W = who;
    if (!p) return fail(SB_ERR_INVALID_ARG, W + ": null placement");
    if (p->flags & ~(uint32_t)(SB_PLACE_FROM_REFERENCE | SB_PLACE_SET_VELOCITY | SB_PLACE_KEEP_PINNED)) return fail(SB_ERR_INVALID_ARG, W + ": unknown flag bit");
    if (p->reserved != 0) return fail(SB_ERR_INVALID_ARG, W + ": reserved must be 0");
    const float *f = p->m;      // m, from, to, lin, ang: 21 floats side by side (the static_assert above)
    for (size_t i = 0; i < sizeof(sbk::PlaceMap) / sizeof(float); ++i)
        if (!std::isfinite(f[i])) return fail(SB_ERR_INVALID_ARG, W + ": NaN or infinite value in m, from, to, lin or ang");
    return SB_OK;
}

namespace {

// First SB_PLACE_FROM_REFERENCE: the reference pose of every local particle in device order. The owned part is what body state keeps
// (on the host until its own first POSE query, on the device afterwards: either serves), the ghosts' part what sb_finalize kept for this.
void upload_place_ref(sb_solver *s) {
    DevBuf<float> d;
    d.alloc((size_t)s->n_local * 3, s->dev_bytes);
    const size_t owned = (size_t)s->n_owned * 3;
    try {
        if (owned && !s->ref_pose.empty()) HIP_CHECK(hipMemcpy(d.p, s->ref_pose.data(), owned * sizeof(float), hipMemcpyHostToDevice));
        else if (owned) HIP_CHECK(hipMemcpyAsync(d.p, s->d_ref_pose.p, owned * sizeof(float), hipMemcpyDeviceToDevice, s->stream));      // (in stream order before the pass)
        if (!s->ref_pose_ghost.empty()) HIP_CHECK(hipMemcpy(d.p + owned, s->ref_pose_ghost.data(), s->ref_pose_ghost.size() * sizeof(float), hipMemcpyHostToDevice));
    } catch (...) {
        s->dev_bytes -= (int64_t)(d.count * sizeof(float));
        throw;
    }
    s->d_place_ref = std::move(d);
    std::vector<float>().swap(s->ref_pose_ghost);
}

template <bool R, bool V, bool K>
void launch_place(sb_solver *s, const sbk::PlaceMap &M) {
    const int64_t n = s->n_local, lanes = n / sbk::kPlacePerLane + n % sbk::kPlacePerLane;
    hipLaunchKernelGGL((sbk::place_kernel<R, V, K>), dim3((unsigned)((lanes + sbk::kPlaceLanes - 1) / sbk::kPlaceLanes)), dim3(sbk::kPlaceLanes), 0, s->stream,
                       s->d_pos3.p, s->d_vel.p, (const float *)s->d_place_ref.p, (const float *)s->d_wf.p, n, M);
    HIP_CHECK(hipGetLastError());
}

}  // namespace

// The rank path: a validated placement applied to every particle this rank holds, ghosts included -- the same arithmetic on a ghost gives
// its owner's bits, so no exchange follows. Completes the tick first, which lands pending kinematic targets (positions in the old frame,
// mapped with the rest); an identity map does so too: the ranks of a group stay in the same tick state. Asynchronous.
int place_validated(sb_solver *s, const sb_placement &p) {
    int rc = set_device(s); if (rc) return rc;
    const bool ref = (p.flags & SB_PLACE_FROM_REFERENCE) != 0, keep = (p.flags & SB_PLACE_KEEP_PINNED) != 0;
    const bool setv = ref || (p.flags & SB_PLACE_SET_VELOCITY) != 0;
    if (ref && !s->d_place_ref.p && s->n_local > 0) upload_place_ref(s);
    flush_deferred(s);
    if (s->n_local == 0) return SB_OK;
    sbk::PlaceMap M;
    std::memcpy(&M, p.m, sizeof(M));
    if (ref) { if (keep) launch_place<true, true, true>(s, M); else launch_place<true, true, false>(s, M); }
    else if (setv) { if (keep) launch_place<false, true, true>(s, M); else launch_place<false, true, false>(s, M); }
    else { if (keep) launch_place<false, false, true>(s, M); else launch_place<false, false, false>(s, M); }
    return SB_OK;
}

}  // namespace sbi
