// AddressSanitizer / UBSan driver for the host authoring unit (softbodyunity_amd/csrc/authoring.cpp): the setters behind sb_set_* and
// sb_group_set_*, and the window cut of sharded authoring, over a CORPUS tests/test_sanitizers.py writes: whole meshes with boxes and the
// window each box must give (computed there with numpy), and malformed setter calls with the code and text they must come back with.
// Everything is compared exactly: integers equal, floats bit for bit. CPU only; links authoring.cpp and plan.cpp (its host threads).
//
// Corpus, a sequence of records, each led by an int32 tag:
//   1 (window case): int32 n, has_rest, m[3], n_boxes; float compliance[3], plane[4]; int32 plane_on; then the ARRAYS of the mesh:
//       float pos[3n], vel[3n], invm[n], rest[3n] (if has_rest); per kind idx[m nv], rest values[m nrest];
//     per box: double lo[3], hi[3]; int32 n_w, m_w[3]; int32 gid[n_w]; the window's ARRAYS in the same layout.
//   2 (setter case): int32 group, n_pre, op (0 particles, 1 rest positions, 2 + kind constraints, 5 ground plane), count, null_pointers,
//       expected code; float compliance, plane[4]; the call's arrays (absent with null_pointers): op 0 pos[3 count], invm[count]; op 1
//       rest[3 count]; op 2 + kind idx[count nv], rest values[count nrest]; then two strings (int32 length, bytes): who, expected text.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "authoring.hpp"

namespace {

FILE *f;

template <class T> std::vector<T> rd(size_t count) {
    std::vector<T> v(count);
    if (count && std::fread(v.data(), sizeof(T), count, f) != count) { std::fprintf(stderr, "truncated corpus\n"); std::exit(2); }
    return v;
}
std::string rd_string() { const int32_t len = rd<int32_t>(1)[0]; const std::vector<char> c = rd<char>((size_t)len); return std::string(c.begin(), c.end()); }

template <class T> bool same(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

struct Arrays {       // a mesh's arrays as the corpus holds them
    std::vector<float> pos, vel, invm, rest;
    std::vector<int32_t> idx[3];
    std::vector<float> restv[3];
};
Arrays rd_arrays(int32_t n, bool has_rest, const int32_t m[3]) {
    Arrays a;
    a.pos = rd<float>(3 * (size_t)n); a.vel = rd<float>(3 * (size_t)n); a.invm = rd<float>((size_t)n);
    if (has_rest) a.rest = rd<float>(3 * (size_t)n);
    for (int t = 0; t < 3; ++t) { a.idx[t] = rd<int32_t>((size_t)m[t] * sbi::kKinds[t].nv); a.restv[t] = rd<float>((size_t)m[t] * sbi::kKinds[t].nrest); }
    return a;
}
bool same(const sbi::AuthoredMesh &m, const Arrays &a) {
    bool ok = same(m.pos, a.pos) && same(m.vel, a.vel) && same(m.invm, a.invm) && same(m.rest, a.rest);
    for (int t = 0; t < 3; ++t) ok = ok && same(m.kind[t].idx, a.idx[t]) && same(m.kind[t].rest, a.restv[t]);
    return ok;
}

#define REQUIRE(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "record %d: ", record); std::fprintf(stderr, __VA_ARGS__); std::fputc('\n', stderr); return false; } } while (0)

int record = 0, boxes = 0, empty_windows = 0, setter_cases = 0;

bool window_case() {
    const std::vector<int32_t> h = rd<int32_t>(6);
    const int32_t n = h[0], m[3] = {h[2], h[3], h[4]};
    const bool has_rest = h[1] != 0;
    const std::vector<float> compliance = rd<float>(3), plane = rd<float>(4);
    const int32_t plane_on = rd<int32_t>(1)[0];
    const Arrays A = rd_arrays(n, has_rest, m);
    // the whole mesh, authored through the setters
    sbi::AuthoredMesh whole;
    sbi::Status st = whole.set_particles("set_particles", A.pos.data(), A.vel.data(), A.invm.data(), n);
    REQUIRE(st.code == SB_OK, "set_particles: %s", st.text.c_str());
    if (has_rest) { st = whole.set_rest_positions("set_rest_positions", A.rest.data(), n); REQUIRE(st.code == SB_OK, "set_rest_positions: %s", st.text.c_str()); }
    for (int t = 0; t < 3; ++t) {
        st = whole.set_constraints(t, sbi::kKinds[t].name, A.idx[t].data(), A.restv[t].data(), m[t], compliance[(size_t)t]);
        REQUIRE(st.code == SB_OK, "set_constraints: %s", st.text.c_str());
    }
    st = whole.set_ground_plane("set_ground_plane", plane[0], plane[1], plane[2], plane[3], plane_on);
    REQUIRE(st.code == SB_OK, "set_ground_plane: %s", st.text.c_str());
    REQUIRE(same(whole, A) && whole.n == n, "the setters did not keep the arrays they were given");
    const sbp::Input in = sbi::make_input(whole);
    REQUIRE(in.n == n && in.rest == (has_rest ? whole.rest : whole.pos).data() && in.m_d == m[0] && in.m_v == m[1] && in.m_b == m[2] &&
            in.dist_ij == whole.kind[0].idx.data() && in.vol == whole.kind[1].idx.data() && in.bend == whole.kind[2].idx.data() && !in.global_id, "make_input");
    for (int32_t b = 0; b < h[5]; ++b, ++boxes) {
        const std::vector<double> box = rd<double>(6);
        const std::vector<int32_t> wh = rd<int32_t>(4);
        const int32_t mw[3] = {wh[1], wh[2], wh[3]};
        const std::vector<int32_t> gid = rd<int32_t>((size_t)wh[0]);
        const Arrays W = rd_arrays(wh[0], has_rest, mw);
        const sbi::Window w = sbi::cut_window(whole, &box[0], &box[3]);
        REQUIRE(same(w.gid, gid), "box %d: %zu particles in the window, %zu expected (or other ids)", b, w.gid.size(), gid.size());
        REQUIRE(w.mesh.n == wh[0] && same(w.mesh, W), "box %d: the window's arrays differ", b);
        for (int t = 0; t < 3; ++t) REQUIRE(w.mesh.count(t) == mw[t] && std::memcmp(&w.mesh.kind[t].compliance, &compliance[(size_t)t], 4) == 0, "box %d: kind %d", b, t);
        REQUIRE(std::memcmp(w.mesh.plane, plane.data(), 16) == 0 && w.mesh.plane_on == (plane_on ? 1 : 0), "box %d: ground plane", b);
        if (gid.empty()) ++empty_windows;
    }
    // what outlives finalize, in place and as a copy
    const sbi::AuthoredMesh kept = whole.without_bulk();
    whole.release_bulk();
    for (const sbi::AuthoredMesh *k : {&kept, static_cast<const sbi::AuthoredMesh *>(&whole)}) {
        REQUIRE(k->n == n && same(k->invm, A.invm) && k->pos.empty() && k->vel.empty() && k->rest.empty() && k->plane_on == (plane_on ? 1 : 0), "release_bulk / without_bulk");
        for (int t = 0; t < 3; ++t) REQUIRE(k->kind[t].idx.empty() && k->kind[t].rest.empty() && std::memcmp(&k->kind[t].compliance, &compliance[(size_t)t], 4) == 0, "release_bulk / without_bulk: kind %d", t);
    }
    return true;
}

bool setter_case() {
    const std::vector<int32_t> h = rd<int32_t>(6);
    const int32_t n_pre = h[1], op = h[2], count = h[3], expected = h[5];
    const bool nulls = h[4] != 0;
    const float compliance = rd<float>(1)[0];
    const std::vector<float> plane = rd<float>(4);
    const size_t c = nulls || count < 0 ? 0 : (size_t)count;
    std::vector<float> fa, fb;
    std::vector<int32_t> ia;
    if (op == 0) { fa = rd<float>(3 * c); fb = rd<float>(c); }
    else if (op == 1) fa = rd<float>(3 * c);
    else if (op < 5) { ia = rd<int32_t>(c * sbi::kKinds[op - 2].nv); fa = rd<float>(c * sbi::kKinds[op - 2].nrest); }
    const std::string who = rd_string(), text = rd_string();
    sbi::AuthoredMesh m;
    m.group = h[0] != 0;
    if (n_pre > 0) {
        const std::vector<float> p(3 * (size_t)n_pre, 0.0f), w((size_t)n_pre, 1.0f);
        REQUIRE(m.set_particles("pre", p.data(), nullptr, w.data(), n_pre).code == SB_OK, "could not set %d particles first", n_pre);
    }
    // (a vector's data() may be non-null when it is empty: the null cases pass nullptr itself)
    sbi::Status st;
    if (op == 0) st = m.set_particles(who.c_str(), nulls ? nullptr : fa.data(), nullptr, nulls ? nullptr : fb.data(), count);
    else if (op == 1) st = m.set_rest_positions(who.c_str(), nulls ? nullptr : fa.data(), count);
    else if (op < 5) st = m.set_constraints(op - 2, who.c_str(), nulls ? nullptr : ia.data(), nulls ? nullptr : fa.data(), count, compliance);
    else st = m.set_ground_plane(who.c_str(), plane[0], plane[1], plane[2], plane[3], 1);
    REQUIRE(st.code == expected && st.text == text, "%s: code %d \"%s\", expected %d \"%s\"", who.c_str(), st.code, st.text.c_str(), expected, text.c_str());
    if (expected != SB_OK)       // a refused call changes nothing
        REQUIRE(m.n == n_pre && m.rest.empty() && m.count(0) + m.count(1) + m.count(2) == 0 && m.plane_on == 0, "%s changed the mesh although it failed", who.c_str());
    ++setter_cases;
    return true;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: authoring_san <corpus>\n"); return 2; }
    f = std::fopen(argv[1], "rb");
    if (!f) { std::perror("corpus"); return 2; }
    int32_t tag;
    while (std::fread(&tag, sizeof tag, 1, f) == 1) {
        ++record;
        if (tag != 1 && tag != 2) { std::fprintf(stderr, "record %d: unknown tag %d\n", record, tag); return 2; }
        if (!(tag == 1 ? window_case() : setter_case())) return 1;
    }
    std::fclose(f);
    std::printf("SANITIZE OK records %d boxes %d empty %d setter cases %d\n", record, boxes, empty_windows, setter_cases);
    return 0;
}
