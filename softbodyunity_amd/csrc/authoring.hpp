// authoring.hpp — the mesh a host authors before finalize: ONE type behind sb_set_* (a solver) and sb_group_set_* (a group), the argument
// checks and copies of both families, the planner's view of it, and the cut of a rank's window under sharded authoring. Host only (g++,
// like plan.cpp): no HIP header, no hip* call; errors come back as a Status for the entry points to record.
//
// No reference counterpart exists (/root/reference/README.md:1 is the whole reference tree).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/softbody.h"
#include "plan.hpp"

namespace sbi {

struct Status {                 // SB_OK, or an error code with the text sb_last_error is to give
    int code = SB_OK;
    std::string text;
};

// The three constraint kinds, in the order of every [3] array of the plugin: the single source of each kind's strides.
struct ConstraintKind { const char *name; int nv, nrest; };      // vertices per constraint, rest values per constraint
constexpr ConstraintKind kKinds[3] = {{"distance", 2, 1}, {"volume", 4, 1}, {"bending", 4, 2}};

struct AuthoredMesh {
    bool group = false;         // authored through sb_group_*: the two texts that name the other family's calls follow it
    int32_t n = 0;
    std::vector<float> pos, vel, invm, rest;        // rest: empty = the rest pose is pos
    struct Constraints {
        std::vector<int32_t> idx;                   // kKinds[t].nv particles per constraint
        std::vector<float> rest;                    // kKinds[t].nrest values per constraint
        float compliance = 0;
    } kind[3];
    float plane[4] = {0, 1, 0, 0};
    int32_t plane_on = 0;

    int64_t count(int t) const { return (int64_t)(kind[t].rest.size() / (size_t)kKinds[t].nrest); }
    const std::vector<float> &rest_or_pos() const { return rest.empty() ? pos : rest; }

    // What the authoring entry points do once their handle is known to be there and not finalized; `who` is the entry point's name.
    Status set_particles(const char *who, const float *pos_xyz, const float *vel_xyz, const float *inv_mass, int32_t count);
    Status set_rest_positions(const char *who, const float *rest_xyz, int32_t count);
    Status set_constraints(int t, const char *who, const int32_t *idx, const float *rest_values, int32_t m, float compliance);
    Status set_ground_plane(const char *who, float nx, float ny, float nz, float d, int32_t enabled);

    // What is read after finalize stays -- n, the inverse masses (kinematic targets), compliances and plane (tick parameters) --, the
    // rest goes (rest values of a 50M-constraint mesh are not kept in host memory): in place, or as a copy of a mesh others still read.
    void release_bulk();
    AuthoredMesh without_bulk() const;
};

sbp::Input make_input(const AuthoredMesh &m);        // (points into m)

// A rank's window of the whole mesh under sharded authoring: the particles whose rest position c satisfies lo <= c < hi on every axis
// (compared in double), the constraints whose particles are all inside, in the whole mesh's order and renumbered; `gid` = the window's
// particles in the whole mesh's numbering, ascending. The box is the caller's (sb_domain_window).
struct Window {
    AuthoredMesh mesh;
    std::vector<int32_t> gid;
};
Window cut_window(const AuthoredMesh &whole, const double lo[3], const double hi[3]);

}  // namespace sbi
