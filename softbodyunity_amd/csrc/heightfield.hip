// heightfield.hip — contacts with a terrain heightfield between two ticks (sb_group_set_heightfield, sb_group_collide_heightfield; SPEC.md
// 2h): the validation of a descriptor and its heights, the table a rank keeps on its device -- with a lifetime of its own: set, replaced
// and cleared between any two calls, never through the tick's stream -- and the launch of the one pass (heightfield_kernels.hip.hpp: no
// other unit includes it). The group's entry points (group.hip) validate once and hand the same table to every rank.
#include <cfloat>
#include <cmath>
#include "solver_internal.hpp"
#include "heightfield_kernels.hip.hpp"

using namespace sbi;

static_assert(sizeof(sb_heightfield) == 80, "sb_heightfield is 80 bytes (include/softbody_group.h)");
static_assert(offsetof(sb_heightfield, rot) == 12 && offsetof(sb_heightfield, cell) == 48 && offsetof(sb_heightfield, nx) == 56 && offsetof(sb_heightfield, thickness) == 64 &&
                  offsetof(sb_heightfield, flags) == 68 && offsetof(sb_heightfield, reserved) == 72,
              "sb_heightfield's layout");

namespace sbi {

// Descriptor and heights alone, before anything is touched (SPEC.md 2h, "Errors"): needs neither a group nor a device.
int validate_heightfield(const char *who, const sb_heightfield *d, const float *heights) {
    const std::string W = std::string(who) + ": ";
    if (!heights) return fail(SB_ERR_INVALID_ARG, W + "null heights");
    if (d->nx < 2 || d->nx > SB_HEIGHTFIELD_MAX_SAMPLES) return fail(SB_ERR_INVALID_ARG, W + "nx outside [2, SB_HEIGHTFIELD_MAX_SAMPLES]");
    if (d->nz < 2 || d->nz > SB_HEIGHTFIELD_MAX_SAMPLES) return fail(SB_ERR_INVALID_ARG, W + "nz outside [2, SB_HEIGHTFIELD_MAX_SAMPLES]");
    if (d->flags != 0) return fail(SB_ERR_INVALID_ARG, W + "flags must be 0");
    for (int32_t r : d->reserved)
        if (r != 0) return fail(SB_ERR_INVALID_ARG, W + "reserved must be 0");
    const float *f = d->a;      // a, rot, cell: 14 floats side by side (the static_asserts above)
    for (size_t k = 0; k < offsetof(sb_heightfield, nx) / sizeof(float); ++k)
        if (!std::isfinite(f[k])) return fail(SB_ERR_INVALID_ARG, W + "NaN or infinite value in the descriptor");
    if (!std::isfinite(d->thickness)) return fail(SB_ERR_INVALID_ARG, W + "NaN or infinite value in the descriptor");
    if (!(d->cell[0] > 0.0f && d->cell[1] > 0.0f)) return fail(SB_ERR_INVALID_ARG, W + "cell must be > 0");
    if (!(d->thickness > 0.0f)) return fail(SB_ERR_INVALID_ARG, W + "thickness must be > 0");
    const int64_t count = (int64_t)d->nx * d->nz;
    for (int64_t i = 0; i < count; ++i)
        if (!std::isfinite(heights[i])) return fail(SB_ERR_INVALID_ARG, W + "NaN or infinite height at sample " + std::to_string(i));
    return SB_OK;
}

int validate_heightfield_call(const char *who, float friction, float restitution) {
    const std::string W = std::string(who) + ": ";
    if (!std::isfinite(friction) || !std::isfinite(restitution)) return fail(SB_ERR_INVALID_ARG, W + "NaN or infinite value");
    if (friction < 0.0f) return fail(SB_ERR_INVALID_ARG, W + "negative friction");
    if (restitution < 0.0f || restitution > 1.0f) return fail(SB_ERR_INVALID_ARG, W + "restitution outside [0, 1]");
    return SB_OK;
}

// No finite rounded height of the table exceeds this (heightfield_kernels.hip.hpp, at heightfield_locate, has the argument): the largest
// sample plus 2^-19 of the largest magnitude plus 2^-140, in binary64 (exact to 2^-53 of a sum the slack dwarfs), rounded UP to binary32.
float heightfield_top(const float *heights, int64_t count) {
    double hmax = -INFINITY, mag = 0.0;
    for (int64_t i = 0; i < count; ++i) {
        hmax = std::max(hmax, (double)heights[i]);
        mag = std::max(mag, std::fabs((double)heights[i]));
    }
    const double top = hmax + std::ldexp(mag, -19) + std::ldexp(1.0, -140);
    if (top >= (double)FLT_MAX) return INFINITY;
    float t = (float)top;
    if ((double)t < top) t = std::nextafterf(t, INFINITY);
    return t;
}

// The pass of the table before, if one may still be running: its own event, nothing else of the device
static void heightfield_wait_for_reader(sb_solver *s) {
    if (!s->hf_in_flight) return;
    HIP_CHECK(hipEventSynchronize(s->ev_hf_read));
    s->hf_in_flight = false;
}

// The rank path of sb_group_set_heightfield for a validated table. The tick's stream is not touched -- a held-back last kernel stays held
// back -- and nothing is ordered behind the tick: the copy is complete when the call returns (so the caller's arrays are free, and the
// next pass, launched later on the rank's stream, needs no event to find the table written). A table of the same size is written over
// the old one; any other size releases it first. Either way only behind the last pass that read it.
int set_heightfield_validated(sb_solver *s, const sb_heightfield &d, const float *heights, float top) {
    int rc = set_device(s); if (rc) return rc;
    const size_t count = (size_t)d.nx * (size_t)d.nz;
    s->ev_hf_read.create(hipEventDisableTiming);
    heightfield_wait_for_reader(s);
    s->hf_set = false;                       // (a failure below leaves no table in force)
    if (s->d_hf.count != count) {
        s->dev_bytes -= (int64_t)(s->d_hf.count * sizeof(float));
        s->d_hf.free();
        s->d_hf.alloc(count, s->dev_bytes);
    }
    HIP_CHECK(hipMemcpy(s->d_hf.p, heights, count * sizeof(float), hipMemcpyHostToDevice));
    s->hf_desc = d;
    s->hf_top = top;
    s->hf_set = true;
    return SB_OK;
}

int clear_heightfield(sb_solver *s) {
    int rc = set_device(s); if (rc) return rc;
    heightfield_wait_for_reader(s);
    s->hf_set = false;
    s->dev_bytes -= (int64_t)(s->d_hf.count * sizeof(float));
    s->d_hf.free();
    return SB_OK;
}

// The rank path of sb_group_collide_heightfield with a table set: every particle this rank holds, ghosts included -- the same arithmetic
// on a ghost gives its owner's bits, so no exchange follows. Completes the tick first, which lands pending kinematic targets. The
// descriptor travels as kernel arguments. Records the event a later set or clear waits for. Allocates nothing. Asynchronous.
int collide_heightfield_validated(sb_solver *s, float friction, float restitution) {
    int rc = set_device(s); if (rc) return rc;
    flush_deferred(s);
    if (s->n_local == 0 || !s->hf_set) return SB_OK;
    const sb_heightfield &d = s->hf_desc;
    sbk::HeightfieldArgs H;
    for (int c = 0; c < 3; ++c) H.a[c] = d.a[c];
    for (int c = 0; c < 9; ++c) H.rot[c] = d.rot[c];
    H.cell[0] = d.cell[0]; H.cell[1] = d.cell[1];
    H.nx = d.nx; H.nz = d.nz;
    H.thickness = d.thickness; H.top = s->hf_top;
    H.friction = friction; H.restitution = restitution;
    const int64_t n = s->n_local, lanes = n / sbk::kHeightfieldPerLane + n % sbk::kHeightfieldPerLane;
    const dim3 grid((unsigned)((lanes + sbk::kHeightfieldLanes - 1) / sbk::kHeightfieldLanes));
    hipLaunchKernelGGL(sbk::heightfield_kernel, grid, dim3(sbk::kHeightfieldLanes), 0, s->stream, s->d_pos3.p, s->d_vel.p, (const float *)s->d_wf.p, n, H, (const float *)s->d_hf.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(s->ev_hf_read, s->stream));
    s->hf_in_flight = true;
    return SB_OK;
}

}  // namespace sbi
