// distance_field_validate_san.cpp — the host code that validates and sizes a signed-distance table and a pose (SPEC.md 2i:
// validate_distance_field, validate_distance_field_pose in softbodyunity_amd/csrc/distance_field.hip), driven without a group and without
// a device under AddressSanitizer and UndefinedBehaviorSanitizer. tests/test_distance_field_sanitize.py builds the unit with the
// sanitizers on its host side, links it with this file and runs the program; it needs no GPU and touches none: only the two validators are called, and what they need
// of the runtime is restated below. Every array handed in is exactly as long as the descriptor says, so a read past the end is reported.
// Prints `DISTANCE FIELD VALIDATE OK <refusals>`.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
#include "solver_internal.hpp"

namespace sbi {
static std::string g_err;
int fail(int code, const std::string &msg) { g_err = msg; return code; }
const char *last_error_text() { return g_err.c_str(); }
int set_device(const sb_solver *) { return SB_ERR_NO_DEVICE; }      // (the rank paths of the unit are linked, never called)
void flush_deferred(sb_solver *) {}
}  // namespace sbi

using namespace sbi;

static int refusals = 0;

static void expect(int rc, int want, const char *word, const char *what) {
    if (rc != want || (word && !std::strstr(last_error_text(), word))) {
        std::fprintf(stderr, "%s: returned %d (wanted %d), last error `%s` (wanted `%s`)\n", what, rc, want, last_error_text(), word ? word : "");
        std::exit(1);
    }
    refusals += rc != SB_OK;
}

static sb_distance_field good(int nx, int ny, int nz) {
    sb_distance_field d;
    std::memset(&d, 0, sizeof d);
    d.nx = nx; d.ny = ny; d.nz = nz;
    d.cell[0] = 0.5f; d.cell[1] = 0.25f; d.cell[2] = 2.0f;
    d.offset = 0.125f; d.thickness = 0.75f;
    return d;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const char *W = "sb_group_set_distance_field";
    // tables of every small shape, each in a heap block of exactly nx ny nz floats
    const int dims[][3] = {{2, 2, 2}, {2, 3, 2}, {3, 2, 4}, {9, 5, 17}, {1024, 2, 2}, {2, 1024, 2}, {2, 2, 1024}, {64, 64, 64}};
    for (const auto &n : dims) {
        sb_distance_field d = good(n[0], n[1], n[2]);
        const size_t count = (size_t)n[0] * n[1] * n[2];
        std::vector<float> s(count);
        for (size_t i = 0; i < count; ++i) s[i] = (float)(i % 97) - 48.0f;
        for (int slot = 0; slot < SB_DISTANCE_FIELD_SLOTS; ++slot) expect(validate_distance_field(W, slot, &d, s.data()), SB_OK, nullptr, "a good table");
        s[count - 1] = nan;
        expect(validate_distance_field(W, 0, &d, s.data()), SB_ERR_INVALID_ARG, ("index " + std::to_string(count - 1)).c_str(), "NaN in the last sample");
        s[count - 1] = 0.0f; s[0] = -inf;
        expect(validate_distance_field(W, 0, &d, s.data()), SB_ERR_INVALID_ARG, "index 0", "-inf in the first sample");
    }
    // what is refused before a sample is read: one float stands for the array, so any read beyond it is reported
    std::vector<float> one(1, 0.0f);
    for (int slot : {-1, (int)SB_DISTANCE_FIELD_SLOTS, INT32_MAX, INT32_MIN}) {
        sb_distance_field d = good(2, 2, 2);
        expect(validate_distance_field(W, slot, &d, one.data()), SB_ERR_INVALID_ARG, "slot outside", "a bad slot");
        expect(validate_distance_field(W, slot, nullptr, nullptr), SB_ERR_INVALID_ARG, "slot outside", "a bad slot of a clear");
    }
    expect(validate_distance_field(W, 3, nullptr, nullptr), SB_OK, nullptr, "a clear");
    { sb_distance_field d = good(2, 2, 2); expect(validate_distance_field(W, 0, &d, nullptr), SB_ERR_INVALID_ARG, "null samples", "null samples"); }
    for (int k = 0; k < 3; ++k)
        for (int v : {1, 0, -3, SB_DISTANCE_FIELD_MAX_DIM + 1, INT32_MAX, INT32_MIN}) {
            sb_distance_field d = good(2, 2, 2);
            (k == 0 ? d.nx : k == 1 ? d.ny : d.nz) = v;
            expect(validate_distance_field(W, 0, &d, one.data()), SB_ERR_INVALID_ARG, "outside [2, SB_DISTANCE_FIELD_MAX_DIM]", "a bad dimension");
        }
    for (const auto &n : {std::vector<int>{1024, 1024, 129}, {1024, 1024, 1024}, {513, 512, 512}}) {       // the product: up to 2^30, no overflow
        sb_distance_field d = good(n[0], n[1], n[2]);
        expect(validate_distance_field(W, 0, &d, one.data()), SB_ERR_INVALID_ARG, "over SB_DISTANCE_FIELD_MAX_SAMPLES", "too many samples");
    }
    for (int k = 0; k < 3; ++k)
        for (float v : {nan, inf, -inf}) {
            sb_distance_field d = good(2, 2, 2);
            d.cell[k] = v;
            expect(validate_distance_field(W, 0, &d, one.data()), SB_ERR_INVALID_ARG, "NaN or infinite value in the descriptor", "a bad float");
        }
    for (float v : {nan, inf, -inf}) {
        sb_distance_field d = good(2, 2, 2); d.offset = v;
        expect(validate_distance_field(W, 0, &d, one.data()), SB_ERR_INVALID_ARG, "NaN or infinite value in the descriptor", "a bad offset");
        d = good(2, 2, 2); d.thickness = v;
        expect(validate_distance_field(W, 0, &d, one.data()), SB_ERR_INVALID_ARG, "NaN or infinite value in the descriptor", "a bad thickness");
    }
    for (int k = 0; k < 3; ++k) {
        sb_distance_field d = good(2, 2, 2); d.cell[k] = -0.0f;
        expect(validate_distance_field(W, 0, &d, one.data()), SB_ERR_INVALID_ARG, "cell must be > 0", "a zero cell");
        d = good(2, 2, 2); d.reserved[k] = 1;
        expect(validate_distance_field(W, 0, &d, one.data()), SB_ERR_INVALID_ARG, "reserved", "a reserved word");
    }
    { sb_distance_field d = good(2, 2, 2); d.offset = -1e-30f; expect(validate_distance_field(W, 0, &d, one.data()), SB_ERR_INVALID_ARG, "offset must be >= 0", "a negative offset"); }
    { sb_distance_field d = good(2, 2, 2); d.thickness = 0.0f; expect(validate_distance_field(W, 0, &d, one.data()), SB_ERR_INVALID_ARG, "thickness must be > 0", "no thickness"); }
    { sb_distance_field d = good(2, 2, 2); d.flags = 0x80000000u; expect(validate_distance_field(W, 0, &d, one.data()), SB_ERR_INVALID_ARG, "flags", "flags"); }
    // poses: a heap copy of exactly 88 bytes
    const char *C = "sb_group_collide_distance_field";
    std::vector<sb_distance_field_pose> p(1);
    std::memset(p.data(), 0, sizeof p[0]);
    p[0].rot[0] = p[0].rot[4] = p[0].rot[8] = 1.0f; p[0].friction = 0.5f; p[0].restitution = 1.0f;
    const sb_distance_field_pose ok = p[0];
    expect(validate_distance_field_pose(C, 0, p.data()), SB_OK, nullptr, "a good pose");
    expect(validate_distance_field_pose(C, 0, nullptr), SB_ERR_INVALID_ARG, "null pose", "a null pose");
    expect(validate_distance_field_pose(C, SB_DISTANCE_FIELD_SLOTS, p.data()), SB_ERR_INVALID_ARG, "slot outside", "a bad slot");
    for (int k = 0; k < 20; ++k)
        for (float v : {nan, inf, -inf}) {
            p[0] = ok;
            float *f = reinterpret_cast<float *>(p.data());     // a, rot, lin, ang, friction, restitution side by side (the unit asserts the layout)
            f[k] = v;
            expect(validate_distance_field_pose(C, 0, p.data()), SB_ERR_INVALID_ARG, "NaN or infinite value in the pose", "a bad float");
        }
    p[0] = ok; p[0].friction = -0.125f; expect(validate_distance_field_pose(C, 0, p.data()), SB_ERR_INVALID_ARG, "negative friction", "friction");
    p[0] = ok; p[0].restitution = 1.0f + 1.2e-7f; expect(validate_distance_field_pose(C, 0, p.data()), SB_ERR_INVALID_ARG, "restitution outside", "restitution");
    p[0] = ok; p[0].reserved[1] = -1; expect(validate_distance_field_pose(C, 0, p.data()), SB_ERR_INVALID_ARG, "reserved", "a reserved word");
    std::printf("DISTANCE FIELD VALIDATE OK %d\n", refusals);
    return 0;
}
