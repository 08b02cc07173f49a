// body_state.hip — SPEC.md §6f: the body's mass centre, momenta and best-fit rotation. The mass-weighted sums are reduced on the device
// (body_state_kernels.hip.hpp: no other unit includes it), one rank's share per call; everything derived from them -- a 3x3 symmetric
// eigenproblem, a 3x3 polar factor -- is host arithmetic in binary64 and a pure function of the 32 sums (sb_group_body_state_from_sums).
// The group's entry point that adds the ranks' sums is in group.hip.
#include "solver_internal.hpp"
#include "body_state_kernels.hip.hpp"

using namespace sbi;

static_assert(SB_BODY_POSE == sbk::kBodyPose && SB_BODY_MOTION == sbk::kBodyMotion, "the kernels' template argument is the ABI's `what`");
static_assert(sizeof(((sb_body_state *)nullptr)->sums) == sbk::kBodySums * sizeof(double), "sb_body_state.sums is one row of the reduction");

namespace sbi {

// The sums of the particles this rank owns, on what sb_get_positions (POSE alone: a peek where that peeks) or sb_get_velocities (MOTION:
// the tick's held-back last kernel is completed first) would return now. counts = dynamic, pinned.
int get_body_sums_owned(sb_solver *s, uint32_t what, double sums[32], int64_t counts[2]) {
    int rc = set_device(s); if (rc) return rc;
    const bool pose = (what & SB_BODY_POSE) != 0, motion = (what & SB_BODY_MOTION) != 0;
    // first use: the reference pose in device order (the host copy sb_finalize kept is given back once it is on the device), the
    // workgroups' rows and the pinned result -- each block keyed on what it makes last (device_handles.hpp)
    if (pose && !s->d_ref_pose.p) {
        s->d_ref_pose.upload(s->ref_pose, s->dev_bytes);
        if (s->d_ref_pose.p) std::vector<float>().swap(s->ref_pose);
    }
    if (!s->h_body.p) {
        s->d_body_partials.alloc((size_t)sbk::kBodyRow * sbk::kBodyMaxGroups, s->dev_bytes);
        s->h_body.alloc(sbk::kBodyRow, /*mapped=*/true);
    }
    if (motion) flush_deferred(s);       // velocities exist only once the tick is complete
    const float *xyz = tick_end_positions(s);
    const int64_t count = s->n_owned;
    const int groups = (int)std::min<int64_t>((count + sbk::kBodyLanes - 1) / sbk::kBodyLanes, sbk::kBodyMaxGroups);
    if (groups) {
        const dim3 grid((unsigned)groups), block(sbk::kBodyLanes);
        if (pose && motion)
            hipLaunchKernelGGL(sbk::body_sums_partial_kernel<3u>, grid, block, 0, s->stream, xyz, (const float *)s->d_vel.p, (const float *)s->d_ref_pose.p, (const float *)s->d_wf.p, count, s->d_body_partials.p);
        else if (pose)
            hipLaunchKernelGGL(sbk::body_sums_partial_kernel<1u>, grid, block, 0, s->stream, xyz, (const float *)nullptr, (const float *)s->d_ref_pose.p, (const float *)s->d_wf.p, count, s->d_body_partials.p);
        else
            hipLaunchKernelGGL(sbk::body_sums_partial_kernel<2u>, grid, block, 0, s->stream, xyz, (const float *)s->d_vel.p, (const float *)nullptr, (const float *)s->d_wf.p, count, s->d_body_partials.p);
    }
    hipLaunchKernelGGL(sbk::body_sums_final_kernel, dim3(1), dim3(sbk::kBodyFinalLanes), 0, s->stream, (const double *)s->d_body_partials.p, groups, s->h_body.dev);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s->stream));
    check_peer_error(s);
    for (int k = 0; k < sbk::kBodySums; ++k) sums[k] = s->h_body.p[k];
    std::memcpy(counts, s->h_body.p + sbk::kBodySums, 2 * sizeof(int64_t));
    return SB_OK;
}

namespace {

bool body_slot_requested(uint32_t what, int k) {
    const bool p = (what & SB_BODY_POSE) != 0, m = (what & SB_BODY_MOTION) != 0;
    return k <= 3 ? true : k <= 6 ? p : k <= 12 ? true : k <= 21 ? p : k <= 28 ? m : false;
}

// One Jacobi rotation's (c, s) from zeta = (a_qq - a_pp) / (2 a_pq): the smaller root t of t^2 + 2 zeta t - 1
void jacobi_cs(double zeta, double &c, double &s) {
    const double az = std::fabs(zeta);
    double t = az > 1e150 ? 0.5 / az : 1.0 / (az + std::sqrt(1.0 + zeta * zeta));
    if (zeta < 0.0) t = -t;
    c = 1.0 / std::sqrt(1.0 + t * t);
    s = t * c;
}

// Symmetric 3x3: eigenvalues lam and eigenvectors (columns of V) by cyclic Jacobi; at most kSweeps sweeps, so it ends on NaN too.
constexpr int kSweeps = 40;
void sym_eig3(const double A[3][3], double lam[3], double V[3][3]) {
    double a[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { a[i][j] = A[i][j]; V[i][j] = i == j ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
        const double off = std::fabs(a[0][1]) + std::fabs(a[0][2]) + std::fabs(a[1][2]);
        const double diag = std::fabs(a[0][0]) + std::fabs(a[1][1]) + std::fabs(a[2][2]);
        if (off <= 0x1p-70 * diag) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (a[p][q] == 0.0) continue;
                double c, s;
                jacobi_cs((a[q][q] - a[p][p]) / (2.0 * a[p][q]), c, s);
                for (int k = 0; k < 3; ++k) { const double u = a[k][p], v = a[k][q]; a[k][p] = c * u - s * v; a[k][q] = s * u + c * v; }      // A J
                for (int k = 0; k < 3; ++k) { const double u = a[p][k], v = a[q][k]; a[p][k] = c * u - s * v; a[q][k] = s * u + c * v; }      // J^T (A J)
                for (int k = 0; k < 3; ++k) { const double u = V[k][p], v = V[k][q]; V[k][p] = c * u - s * v; V[k][q] = s * u + c * v; }
            }
    }
    for (int i = 0; i < 3; ++i) lam[i] = a[i][i];
}

void cross(const double a[3], const double b[3], double o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

// SPEC.md §6f: the rotation factor of the polar decomposition of G (row-major), det = +1, Kabsch where det(G) < 0. One-sided Jacobi:
// G V = U diag(sigma) with the columns of G V made orthogonal -- small singular values keep their relative accuracy, which a planar
// reference pose (sigma_3 = 0) and the rank test need. With sigma_1 >= sigma_2 the two leading pairs (u_1, v_1), (u_2, v_2) fix the
// answer: R = u_1 v_1^T + u_2 v_2^T + (u_1 x u_2)(v_1 x v_2)^T is the polar factor where det(G) > 0, its Kabsch correction where
// det(G) < 0 (the third pair enters with the sign that makes both frames right-handed) and the one proper rotation that fits where
// sigma_3 = 0. -> false: rank below 2 (sigma_2 <= 1e-12 sigma_1), R untouched. A non-finite G gives a NaN R.
bool polar_rotation(const double G[9], double R[3][3]) {
    double U[3][3], V[3][3];
    double big = 0.0;
    bool finite = true;
    for (int k = 0; k < 9; ++k) { big = std::fmax(big, std::fabs(G[k])); finite = finite && std::isfinite(G[k]); }
    if (!finite) {      // no frame fits a pose that is not finite: the answer is not a number either (and not the identity of a degenerate pose)
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R[i][j] = std::numeric_limits<double>::quiet_NaN();
        return true;
    }
    int e = 0;
    if (big > 0.0) (void)std::frexp(big, &e);      // scale by a power of two: squares of the entries neither overflow nor vanish
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { U[i][j] = std::ldexp(G[3 * i + j], -e); V[i][j] = i == j ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (int i = 0; i < 3; ++i) { alpha += U[i][p] * U[i][p]; beta += U[i][q] * U[i][q]; gamma += U[i][p] * U[i][q]; }
                if (gamma == 0.0 || std::fabs(gamma) <= 0x1p-53 * std::sqrt(alpha * beta)) continue;
                rotated = true;
                double c, s;
                jacobi_cs((beta - alpha) / (2.0 * gamma), c, s);
                for (int i = 0; i < 3; ++i) { const double u = U[i][p], v = U[i][q]; U[i][p] = c * u - s * v; U[i][q] = s * u + c * v; }
                for (int i = 0; i < 3; ++i) { const double u = V[i][p], v = V[i][q]; V[i][p] = c * u - s * v; V[i][q] = s * u + c * v; }
            }
        if (!rotated) break;
    }
    double sigma[3];
    for (int j = 0; j < 3; ++j) sigma[j] = std::sqrt(U[0][j] * U[0][j] + U[1][j] * U[1][j] + U[2][j] * U[2][j]);
    int a = 0;
    for (int j = 1; j < 3; ++j) if (sigma[j] > sigma[a]) a = j;
    int b = a == 0 ? 1 : 0;
    for (int j = 0; j < 3; ++j) if (j != a && sigma[j] > sigma[b]) b = j;
    if (sigma[b] <= 1e-12 * sigma[a]) return false;
    double u1[3], u2[3], u3[3], v1[3], v2[3], v3[3];
    for (int i = 0; i < 3; ++i) { u1[i] = U[i][a] / sigma[a]; u2[i] = U[i][b] / sigma[b]; v1[i] = V[i][a]; v2[i] = V[i][b]; }
    cross(u1, u2, u3); cross(v1, v2, v3);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R[i][j] = (u1[i] * v1[j] + u2[i] * v2[j]) + u3[i] * v3[j];
    return true;
}

// unit quaternion (x, y, z, w), w >= 0, of a rotation matrix (the branch with the largest divisor)
void quaternion_of(const double R[3][3], double q[4]) {
    const double tr = R[0][0] + R[1][1] + R[2][2];
    if (tr > 0.0) {
        const double S = 2.0 * std::sqrt(tr + 1.0);
        q[3] = 0.25 * S; q[0] = (R[2][1] - R[1][2]) / S; q[1] = (R[0][2] - R[2][0]) / S; q[2] = (R[1][0] - R[0][1]) / S;
    } else if (R[0][0] > R[1][1] && R[0][0] > R[2][2]) {
        const double S = 2.0 * std::sqrt(1.0 + R[0][0] - R[1][1] - R[2][2]);
        q[3] = (R[2][1] - R[1][2]) / S; q[0] = 0.25 * S; q[1] = (R[0][1] + R[1][0]) / S; q[2] = (R[0][2] + R[2][0]) / S;
    } else if (R[1][1] > R[2][2]) {
        const double S = 2.0 * std::sqrt(1.0 + R[1][1] - R[0][0] - R[2][2]);
        q[3] = (R[0][2] - R[2][0]) / S; q[0] = (R[0][1] + R[1][0]) / S; q[1] = 0.25 * S; q[2] = (R[1][2] + R[2][1]) / S;
    } else {
        const double S = 2.0 * std::sqrt(1.0 + R[2][2] - R[0][0] - R[1][1]);
        q[3] = (R[1][0] - R[0][1]) / S; q[0] = (R[0][2] + R[2][0]) / S; q[1] = (R[1][2] + R[2][1]) / S; q[2] = 0.25 * S;
    }
    const double len = std::sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
    for (int k = 0; k < 4; ++k) q[k] /= len;
    if (q[3] < 0.0) for (int k = 0; k < 4; ++k) q[k] = -q[k];
}

}  // namespace

// SPEC.md §6f "Derived values": every field of *out from the 32 sums; slots and fields `what` did not ask for are 0, the rotation identity.
void body_state_derive(const double sums[32], int64_t n_dynamic, int64_t n_pinned, uint32_t what, sb_body_state *out) {
    sb_body_state o;
    std::memset(&o, 0, sizeof o);
    o.n_dynamic = n_dynamic; o.n_pinned = n_pinned; o.what = what;
    o.rotation[3] = 1.0;
    for (int k = 0; k < 32; ++k) o.sums[k] = body_slot_requested(what, k) ? sums[k] : 0.0;
    if (n_dynamic == 0) { o.flags = SB_BODY_NO_MASS; std::memset(o.sums, 0, sizeof o.sums); *out = o; return; }
    const bool pose = (what & SB_BODY_POSE) != 0, motion = (what & SB_BODY_MOTION) != 0;
    const double *S = o.sums;
    const double M = S[0];
    o.mass = M;
    for (int c = 0; c < 3; ++c) o.com[c] = S[1 + c] / M;
    const double *x = o.com;
    o.second_moment[0] = S[7] - M * x[0] * x[0]; o.second_moment[1] = S[8] - M * x[1] * x[1]; o.second_moment[2] = S[9] - M * x[2] * x[2];
    o.second_moment[3] = S[10] - M * x[0] * x[1]; o.second_moment[4] = S[11] - M * x[0] * x[2]; o.second_moment[5] = S[12] - M * x[1] * x[2];
    if (pose) {
        for (int c = 0; c < 3; ++c) o.ref_com[c] = S[4 + c] / M;
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) o.apq[3 * i + j] = S[13 + 3 * i + j] - M * x[i] * o.ref_com[j];
        double R[3][3];
        if (polar_rotation(o.apq, R)) quaternion_of(R, o.rotation);
        else o.flags |= SB_BODY_DEGENERATE_POSE;
    }
    if (motion) {
        for (int c = 0; c < 3; ++c) { o.momentum[c] = S[22 + c]; o.velocity[c] = S[22 + c] / M; }
        double xp[3];
        cross(x, o.momentum, xp);
        for (int c = 0; c < 3; ++c) o.angular_momentum[c] = S[25 + c] - xp[c];
        o.kinetic_energy = 0.5 * S[28];
        const double *C = o.second_moment;
        const double tr = (C[0] + C[1]) + C[2];
        const double I[3][3] = {{tr - C[0], -C[3], -C[4]}, {-C[3], tr - C[1], -C[5]}, {-C[4], -C[5], tr - C[2]}};
        double lam[3], V[3][3];
        sym_eig3(I, lam, V);
        const double lmax = std::fmax(lam[0], std::fmax(lam[1], lam[2])), lmin = std::fmin(lam[0], std::fmin(lam[1], lam[2]));
        const bool nan = lam[0] != lam[0] || lam[1] != lam[1] || lam[2] != lam[2];      // (fmin / fmax drop a NaN: it must propagate instead)
        if (!nan && lmin <= 1e-12 * lmax) o.flags |= SB_BODY_DEGENERATE_INERTIA;
        else {
            double y[3];       // omega = V diag(1 / lam) V^T L
            for (int k = 0; k < 3; ++k) y[k] = ((V[0][k] * o.angular_momentum[0] + V[1][k] * o.angular_momentum[1]) + V[2][k] * o.angular_momentum[2]) / lam[k];
            for (int c = 0; c < 3; ++c) o.angular_velocity[c] = (V[c][0] * y[0] + V[c][1] * y[1]) + V[c][2] * y[2];
        }
    }
    *out = o;
}

}  // namespace sbi

extern "C" {

int sb_group_body_state_from_sums(const double sums[32], int64_t n_dynamic, int64_t n_pinned, uint32_t what, sb_body_state *out) {
    if (!sums || !out) return fail(SB_ERR_INVALID_ARG, "sb_group_body_state_from_sums: null argument");
    if (what == 0 || (what & ~(SB_BODY_POSE | SB_BODY_MOTION))) return fail(SB_ERR_INVALID_ARG, "sb_group_body_state_from_sums: `what` must be SB_BODY_POSE, SB_BODY_MOTION or both");
    if (n_dynamic < 0 || n_pinned < 0) return fail(SB_ERR_INVALID_ARG, "sb_group_body_state_from_sums: negative count");
    body_state_derive(sums, n_dynamic, n_pinned, what, out);
    return SB_OK;
}

}  // extern "C"
