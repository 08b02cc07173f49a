// distance_field.hip — contacts with signed-distance volumes between two ticks (sb_group_set_distance_field,
// sb_group_collide_distance_field; SPEC.md 2i): the validation of a descriptor with its samples and of a pose, the tables a rank keeps on
// its device -- SB_DISTANCE_FIELD_SLOTS of them, each with a lifetime of its own: set, replaced and cleared between any two calls, never
// through the tick's stream -- and the launch of the one pass (distance_field_kernels.hip.hpp: no other unit includes it). The group's
// entry points (group.hip) validate once and hand the same table to every rank.
#include <cmath>
#include "solver_internal.hpp"
#include "distance_field_kernels.hip.hpp"

using namespace sbi;

static_assert(sizeof(sb_distance_field) == 48, "sb_distance_field is 48 bytes (include/softbody_group.h)");
static_assert(offsetof(sb_distance_field, cell) == 12 && offsetof(sb_distance_field, offset) == 24 && offsetof(sb_distance_field, thickness) == 28 &&
                  offsetof(sb_distance_field, flags) == 32 && offsetof(sb_distance_field, reserved) == 36,
              "sb_distance_field's layout");
static_assert(sizeof(sb_distance_field_pose) == 88, "sb_distance_field_pose is 88 bytes (include/softbody_group.h)");
static_assert(offsetof(sb_distance_field_pose, rot) == 12 && offsetof(sb_distance_field_pose, lin) == 48 && offsetof(sb_distance_field_pose, ang) == 60 &&
                  offsetof(sb_distance_field_pose, friction) == 72 && offsetof(sb_distance_field_pose, restitution) == 76 && offsetof(sb_distance_field_pose, reserved) == 80,
              "sb_distance_field_pose's layout");
static_assert((int64_t)SB_DISTANCE_FIELD_MAX_SAMPLES <= INT32_MAX, "the kernel's flat index is an int32");

namespace sbi {

// Slot, descriptor and samples alone, before anything is touched (SPEC.md 2i, "Errors"): needs neither a group nor a device. d may be
// null (a clear): then the slot alone is checked.
int validate_distance_field(const char *who, int32_t slot, const sb_distance_field *d, const float *samples) {
    const std::string W = std::string(who) + ": ";
    if (slot < 0 || slot >= SB_DISTANCE_FIELD_SLOTS) return fail(SB_ERR_INVALID_ARG, W + "slot outside [0, SB_DISTANCE_FIELD_SLOTS)");
    if (!d) return SB_OK;
    if (!samples) return fail(SB_ERR_INVALID_ARG, W + "null samples");
    const int32_t dim[3] = {d->nx, d->ny, d->nz};
    const char *const name[3] = {"nx", "ny", "nz"};
    for (int k = 0; k < 3; ++k)
        if (dim[k] < 2 || dim[k] > SB_DISTANCE_FIELD_MAX_DIM) return fail(SB_ERR_INVALID_ARG, W + name[k] + " outside [2, SB_DISTANCE_FIELD_MAX_DIM]");
    const int64_t count = (int64_t)d->nx * d->ny * d->nz;      // (<= 2^30: no overflow)
    if (count > (int64_t)SB_DISTANCE_FIELD_MAX_SAMPLES) return fail(SB_ERR_INVALID_ARG, W + "nx * ny * nz over SB_DISTANCE_FIELD_MAX_SAMPLES");
    if (d->flags != 0) return fail(SB_ERR_INVALID_ARG, W + "flags must be 0");
    for (int32_t r : d->reserved)
        if (r != 0) return fail(SB_ERR_INVALID_ARG, W + "reserved must be 0");
    const float *f = d->cell;      // cell, offset, thickness: 5 floats side by side (the static_asserts above)
    for (int k = 0; k < 5; ++k)
        if (!std::isfinite(f[k])) return fail(SB_ERR_INVALID_ARG, W + "NaN or infinite value in the descriptor");
    if (!(d->cell[0] > 0.0f && d->cell[1] > 0.0f && d->cell[2] > 0.0f)) return fail(SB_ERR_INVALID_ARG, W + "cell must be > 0");
    if (!(d->offset >= 0.0f)) return fail(SB_ERR_INVALID_ARG, W + "offset must be >= 0");
    if (!(d->thickness > 0.0f)) return fail(SB_ERR_INVALID_ARG, W + "thickness must be > 0");
    for (int64_t i = 0; i < count; ++i)
        if (!std::isfinite(samples[i])) return fail(SB_ERR_INVALID_ARG, W + "NaN or infinite sample at index " + std::to_string(i));
    return SB_OK;
}

int validate_distance_field_pose(const char *who, int32_t slot, const sb_distance_field_pose *p) {
    const std::string W = std::string(who) + ": ";
    if (!p) return fail(SB_ERR_INVALID_ARG, W + "null pose");
    if (slot < 0 || slot >= SB_DISTANCE_FIELD_SLOTS) return fail(SB_ERR_INVALID_ARG, W + "slot outside [0, SB_DISTANCE_FIELD_SLOTS)");
    const float *f = p->a;      // a, rot, lin, ang, friction, restitution: 20 floats side by side (the static_asserts above)
    for (size_t k = 0; k < offsetof(sb_distance_field_pose, reserved) / sizeof(float); ++k)
        if (!std::isfinite(f[k])) return fail(SB_ERR_INVALID_ARG, W + "NaN or infinite value in the pose");
    if (p->friction < 0.0f) return fail(SB_ERR_INVALID_ARG, W + "negative friction");
    if (p->restitution < 0.0f || p->restitution > 1.0f) return fail(SB_ERR_INVALID_ARG, W + "restitution outside [0, 1]");
    for (int32_t r : p->reserved)
        if (r != 0) return fail(SB_ERR_INVALID_ARG, W + "reserved must be 0");
    return SB_OK;
}

// The pass of the slot's table before, if one may still be running: its own event, nothing else of the device
static void distance_field_wait_for_reader(sb_solver::DistanceFieldTable &T) {
    if (!T.in_flight) return;
    HIP_CHECK(hipEventSynchronize(T.ev_read));
    T.in_flight = false;
}

// The rank path of sb_group_set_distance_field for a validated table. The tick's stream is not touched -- a held-back last kernel stays
// held back -- and nothing is ordered behind the tick: the copy is complete when the call returns (so the caller's arrays are free, and
// the next pass, launched later on the rank's stream, needs no event to find the table written). A table of the same size is written
// over the old one; any other size releases it first. Either way only behind the last pass that read the slot.
int set_distance_field_validated(sb_solver *s, int32_t slot, const sb_distance_field &d, const float *samples) {
    int rc = set_device(s); if (rc) return rc;
    sb_solver::DistanceFieldTable &T = s->df[slot];
    const size_t count = (size_t)d.nx * (size_t)d.ny * (size_t)d.nz;
    T.ev_read.create(hipEventDisableTiming);
    distance_field_wait_for_reader(T);
    T.set = false;                           // (a failure below leaves no table in force)
    if (T.d.count != count) {
        s->dev_bytes -= (int64_t)(T.d.count * sizeof(float));
        T.d.free();
        T.d.alloc(count, s->dev_bytes);
    }
    HIP_CHECK(hipMemcpy(T.d.p, samples, count * sizeof(float), hipMemcpyHostToDevice));
    T.desc = d;
    T.set = true;
    return SB_OK;
}

int clear_distance_field(sb_solver *s, int32_t slot) {
    int rc = set_device(s); if (rc) return rc;
    sb_solver::DistanceFieldTable &T = s->df[slot];
    distance_field_wait_for_reader(T);
    T.set = false;
    s->dev_bytes -= (int64_t)(T.d.count * sizeof(float));
    T.d.free();
    return SB_OK;
}

// The rank path of sb_group_collide_distance_field with a table in the slot: every particle this rank holds, ghosts included -- the same
// arithmetic on a ghost gives its owner's bits, so no exchange follows. Completes the tick first, which lands pending kinematic targets.
// Descriptor and pose travel as kernel arguments. Records the event a later set or clear of the slot waits for. Allocates nothing.
// Asynchronous.
int collide_distance_field_validated(sb_solver *s, int32_t slot, const sb_distance_field_pose &p) {
    int rc = set_device(s); if (rc) return rc;
    flush_deferred(s);
    sb_solver::DistanceFieldTable &T = s->df[slot];
    if (s->n_local == 0 || !T.set) return SB_OK;
    const sb_distance_field &d = T.desc;
    sbk::DistanceFieldArgs D;
    for (int c = 0; c < 3; ++c) { D.a[c] = p.a[c]; D.cell[c] = d.cell[c]; D.lin[c] = p.lin[c]; D.ang[c] = p.ang[c]; }
    for (int c = 0; c < 9; ++c) D.rot[c] = p.rot[c];
    D.nx = d.nx; D.ny = d.ny; D.nz = d.nz;
    D.offset = d.offset; D.thickness = d.thickness;
    D.friction = p.friction; D.restitution = p.restitution;
    const int64_t n = s->n_local, lanes = n / sbk::kDistanceFieldPerLane + n % sbk::kDistanceFieldPerLane;
    const dim3 grid((unsigned)((lanes + sbk::kDistanceFieldLanes - 1) / sbk::kDistanceFieldLanes));
    hipLaunchKernelGGL(sbk::distance_field_kernel, grid, dim3(sbk::kDistanceFieldLanes), 0, s->stream, s->d_pos3.p, s->d_vel.p, (const float *)s->d_wf.p, n, D, (const float *)T.d.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(T.ev_read, s->stream));
    T.in_flight = true;
    return SB_OK;
}

}  // namespace sbi
