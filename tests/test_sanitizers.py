"""AddressSanitizer + UBSan over the host-side native code (the planner, the table builder, the authoring unit and the C oracle), and
ThreadSanitizer over the host threads of the planner and the table builder. GPU sanitizers are not available on the pool, so this is the CPU
build only: tests/sanitize/plan_san.cpp drives plan.cpp and tables_host.cpp directly, tests/sanitize/authoring_san.cpp authoring.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "softbodyunity_amd", "csrc")
# the planner and the host table builder; the HIP headers only give kernel_types.hpp its vector types, no HIP library is linked
HOST_UNITS = [os.path.join(CSRC, "plan.cpp"), os.path.join(CSRC, "tables_host.cpp")]
HOST_FLAGS = ["-Wno-attributes", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]


def test_planner_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "plan_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-pthread", *SAN, *HOST_FLAGS, os.path.join(ROOT, "tests", "sanitize", "plan_san.cpp"),
                           *HOST_UNITS, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", SB_PLAN_THREADS="4")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and "SANITIZE OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_planner_threads_under_tsan(tmp_path):
    # the planner splits its phases over host threads (plan.cpp parallel_chunks): no data race, and the same plan for any
    # thread count (checked bit for bit by tests/test_plan.py::test_plan_is_independent_of_the_thread_count)
    exe = str(tmp_path / "plan_tsan")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-pthread", "-fsanitize=thread", "-g", "-O1", *HOST_FLAGS,
                           os.path.join(ROOT, "tests", "sanitize", "plan_san.cpp"), *HOST_UNITS, "-o", exe])
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1", SB_PLAN_THREADS="4")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=900)
    assert out.returncode == 0 and "SANITIZE OK" in out.stdout and "WARNING: ThreadSanitizer" not in out.stderr, out.stdout[-2000:] + out.stderr[-4000:]


def test_oracle_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "oracle_san")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", *SAN, "-ffp-contract=off", "-fopenmp", "-I", os.path.join(ROOT, "oracle"),
                           os.path.join(ROOT, "tests", "sanitize", "oracle_san.c"), "-lm", "-o", exe])   # includes oracle.c
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", OMP_NUM_THREADS="2")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and "SANITIZE OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_planner_on_the_fuzz_corpus_under_asan_ubsan(tmp_path):
    """The degenerate meshes of tests/fuzz/fuzz_plan.py (a point, a line, no constraints, complete graphs, NaN ...) through plan.cpp under ASan + UBSan."""
    import sys
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests", "fuzz")); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, ROOT)
    import fuzz_plan
    corpus = tmp_path / "corpus.bin"
    with open(corpus, "wb") as f:
        for seed in range(250):
            sc = fuzz_plan.make_scenario(seed)
            m = sc["_mesh"]
            np.array([m.n, len(m.dist_rest), len(m.vol_rest), len(m.bend_rest), sc["world"], sc["tile"], sc["partition"], -1, 0, 0, 0, 0], np.int32).tofile(f)
            np.ascontiguousarray(m.rest_pos, np.float32).tofile(f)
            for a in (m.dist_ij, m.vol_ijkl, m.bend_ijkl):
                np.ascontiguousarray(a, np.int32).tofile(f)
        # ranks' windows (sharded authoring): domain + whole-mesh ids, cut as the group host cuts them
        import fuzz_windows
        from softbodyunity_amd import native
        n_windows = 0
        for seed in range(40):
            sc = fuzz_windows.make_scenario(seed)
            rest, ij, W = sc["_rest"], sc["_ij"], sc["world"]
            dom = native.domain_from_mesh(rest, ij)
            for r in range(W):
                lo, hi = native.domain_window(dom, r, W, sc["dims"], sc["tile"])
                gid = np.nonzero(np.all((rest >= np.array(lo)) & (rest < np.array(hi)), axis=1))[0].astype(np.int32)
                if len(gid) == 0:
                    continue
                new = -np.ones(len(rest), np.int64); new[gid] = np.arange(len(gid))
                wij = new[ij[np.all(new[ij] >= 0, axis=1)]].astype(np.int32)
                # (in the order plan_corpus_san.cpp reads a window: header, domain, whole-mesh ids, then the mesh)
                np.array([len(gid), len(wij), 0, 0, W, sc["tile"], 1, r, *sc["dims"], 0], np.int32).tofile(f)
                np.array([dom.n_global, *dom.lo, *dom.hi, dom.spacing, dom.fill], np.float64).tofile(f)
                gid.tofile(f)
                np.ascontiguousarray(rest[gid], np.float32).tofile(f)
                wij.tofile(f); np.zeros(0, np.int32).tofile(f); np.zeros(0, np.int32).tofile(f)
                n_windows += 1
    exe = str(tmp_path / "plan_corpus_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-pthread", *SAN, *HOST_FLAGS, os.path.join(ROOT, "tests", "sanitize", "plan_corpus_san.cpp"),
                           *HOST_UNITS, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", SB_PLAN_THREADS="4")
    out = subprocess.run([exe, str(corpus)], capture_output=True, text=True, env=env, timeout=900)
    assert out.returncode == 0 and f"SANITIZE OK entries {250 + n_windows}" in out.stdout and n_windows > 100, out.stdout[-2000:] + out.stderr[-4000:]


# ---- the authoring unit (authoring.cpp): setters and the window cut -------------------------------------------------------------------------

_KIND_NV, _KIND_NREST = (2, 4, 4), (1, 1, 2)


def _numpy_cut(mesh, lo, hi):
    """One rank's window of `mesh` (pos, vel, invm, rest or None, idx[3], restv[3]) as sb_group_finalize hands it over: the particles whose
    REST position (their position when no rest pose was given) lies in [lo, hi) on every axis, compared in double; their masses, velocities
    and positions; the constraints whose particles are all inside, in the whole mesh's order, renumbered, with their rest values."""
    import numpy as np
    pos, vel, invm, rest, idx, restv = mesh
    rp = (pos if rest is None else rest).astype(np.float64)
    gid = np.nonzero(np.all((rp >= np.array(lo)) & (rp < np.array(hi)), axis=1))[0].astype(np.int32)
    new = -np.ones(len(pos), np.int64); new[gid] = np.arange(len(gid))
    widx, wrestv = [], []
    for t in range(3):
        keep = np.all(new[idx[t]] >= 0, axis=1) if len(idx[t]) else np.zeros(0, bool)
        widx.append(new[idx[t][keep]].astype(np.int32).reshape(-1, _KIND_NV[t]))
        wrestv.append(restv[t][keep])
    return gid, (pos[gid], vel[gid], invm[gid], None if rest is None else rest[gid], widx, wrestv)


def _write_arrays(f, mesh):
    import numpy as np
    pos, vel, invm, rest, idx, restv = mesh
    for a in (pos, vel, invm) + (() if rest is None else (rest,)):
        np.ascontiguousarray(a, np.float32).tofile(f)
    for t in range(3):
        np.ascontiguousarray(idx[t], np.int32).tofile(f); np.ascontiguousarray(restv[t], np.float32).tofile(f)


def _write_window_case(f, mesh, boxes, compliance=(0.0, 0.0, 0.0), plane=(0.0, 1.0, 0.0, 0.0), plane_on=0):
    import numpy as np
    pos, vel, invm, rest, idx, restv = mesh
    np.array([1, len(pos), rest is not None, *(len(i) for i in idx), len(boxes)], np.int32).tofile(f)
    np.array([*compliance, *plane], np.float32).tofile(f); np.array([plane_on], np.int32).tofile(f)
    _write_arrays(f, mesh)
    sizes = []
    for lo, hi in boxes:
        gid, win = _numpy_cut(mesh, lo, hi)
        np.array([*lo, *hi], np.float64).tofile(f)
        np.array([len(gid), *(len(i) for i in win[4])], np.int32).tofile(f)
        gid.tofile(f)
        _write_arrays(f, win)
        sizes.append(len(gid))
    return sizes


def _mesh_tuple(m, rest_given):
    import numpy as np
    return (m.pos, m.vel, m.inv_mass, m.rest_pos if rest_given else None, [np.asarray(m.dist_ij).reshape(-1, 2), np.asarray(m.vol_ijkl).reshape(-1, 4), np.asarray(m.bend_ijkl).reshape(-1, 4)],
            [np.asarray(m.dist_rest).reshape(-1, 1), np.asarray(m.vol_rest).reshape(-1, 1), np.asarray(m.bend_rest).reshape(-1, 2)])


# (op, who, group, n_pre, count, null pointers, compliance, expected code, expected text) -- the texts are the entry points' of the commit
# before the setters moved into authoring.cpp, kept here as data; ops: 0 particles, 1 rest positions, 2 + kind constraints, 5 ground plane
_INVALID, _STATE = -1, -2


def _setter_cases():
    nan = float("nan")
    cases = []
    for grp, pre in ((0, "sb_"), (1, "sb_group_")):
        who = pre + "set_particles"
        cases += [(0, who, grp, 0, 3, 0, 0.0, _INVALID, who + ": inverse mass must be >= 0", {"invm": [1.0, -0.5, 1.0]}),
                  (0, who, grp, 0, 3, 0, 0.0, _INVALID, who + ": inverse mass must be >= 0", {"invm": [1.0, 1.0, nan]}),
                  (0, who, grp, 0, 3, 1, 0.0, _INVALID, who + ": bad argument", {}),
                  (0, who, grp, 0, 0, 0, 0.0, _INVALID, who + ": bad argument", {}),
                  (0, who, grp, 0, 3, 0, 0.0, 0, "", {"invm": [1.0, 0.0, 2.0]})]
        who = pre + "set_rest_positions"
        differs = ": bad argument (n differs from sb_group_set_particles?)" if grp else ": n differs from sb_set_particles"
        cases += [(1, who, grp, 4, 3, 0, 0.0, _INVALID, who + differs, {}),
                  (1, who, grp, 4, 5, 0, 0.0, _INVALID, who + differs, {}),
                  (1, who, grp, 4, 4, 1, 0.0, _INVALID, who + (differs if grp else ": bad argument"), {}),
                  (1, who, grp, 4, 4, 0, 0.0, 0, "", {})]
        for t, name in enumerate(("distance", "volume", "bending")):
            who = f"{pre}set_{name}_constraints"
            good = list(range(_KIND_NV[t]))
            cases += [(2 + t, who, grp, 4, 1, 0, nan, _INVALID, who + ": compliance must be >= 0", {"idx": good}),
                      (2 + t, who, grp, 4, 1, 0, -1.0, _INVALID, who + ": compliance must be >= 0", {"idx": good}),
                      (2 + t, who, grp, 4, 1, 0, 0.0, _INVALID, who + ": particle index out of range", {"idx": good[:-1] + [4]}),
                      (2 + t, who, grp, 4, 1, 0, 0.0, _INVALID, who + ": particle index out of range", {"idx": [-1] + good[1:]}),
                      (2 + t, who, grp, 4, 0, 1, 0.0, 0, "", {}),
                      (2 + t, who, grp, 4, 1, 1, 0.0, _INVALID, who + ": bad argument", {}),
                      (2 + t, who, grp, 4, -1, 1, 0.0, _INVALID, who + ": bad argument", {}),
                      (2 + t, who, grp, 0, 1, 0, 0.0, _STATE, f"{who} before {pre}set_particles", {"idx": good}),
                      (2 + t, who, grp, 4, 1, 0, 0.5, 0, "", {"idx": good})]
        who = pre + "set_ground_plane"
        cases += [(5, who, grp, 0, 0, 0, 0.0, _INVALID, who + ": NaN", {"plane": [0.0, nan, 0.0, 0.0]}),
                  (5, who, grp, 0, 0, 0, 0.0, _INVALID, who + ": NaN", {"plane": [0.0, 1.0, 0.0, nan]}),
                  (5, who, grp, 0, 0, 0, 0.0, 0, "", {"plane": [0.0, 1.0, 0.0, -2.0]})]
    return cases


def _write_setter_case(f, case):
    import numpy as np
    op, who, grp, n_pre, count, nulls, compliance, code, text, data = case
    np.array([2, grp, n_pre, op, count, nulls, code], np.int32).tofile(f)
    np.array([compliance, *data.get("plane", [0.0, 1.0, 0.0, 0.0])], np.float32).tofile(f)
    c = 0 if nulls or count < 0 else count
    if op == 0:
        np.zeros(3 * c, np.float32).tofile(f); np.array(data.get("invm", [1.0] * c), np.float32).tofile(f)
    elif op == 1:
        np.zeros(3 * c, np.float32).tofile(f)
    elif op < 5:
        np.array(data.get("idx", [0] * (c * _KIND_NV[op - 2]))[:c * _KIND_NV[op - 2]], np.int32).tofile(f); np.ones(c * _KIND_NREST[op - 2], np.float32).tofile(f)
    for s in (who, text):
        b = s.encode(); np.array([len(b)], np.int32).tofile(f); f.write(b)


def test_authoring_under_asan_ubsan(tmp_path):
    """authoring.cpp -- the setters behind sb_set_* / sb_group_set_* and the window cut of sharded authoring -- under ASan + UBSan, against
    windows cut here with numpy (every value compared exactly) and the error texts of the entry points."""
    import sys
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests", "fuzz")); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, ROOT)
    import fuzz_windows
    from softbodyunity_amd import native
    from softbodyunity_amd.mesh import from_tet_mesh, jelly_cube
    corpus = tmp_path / "authoring_corpus.bin"
    n_boxes = 0
    with open(corpus, "wb") as f:
        # a 4^3 cube, every mass and rest length its own, the rest pose given and the positions moved so far off it that a cut by position
        # would take other particles: into 2 and into 8 windows
        cube = jelly_cube(4, perturb=0.6, heterogeneous=True)
        cube.vel = np.random.default_rng(5).normal(size=cube.pos.shape).astype(np.float32)
        mesh = _mesh_tuple(cube, True)
        # (sb_domain_window's boxes each hold a body this small whole: halves and octants that overlap by two lattice planes, as windows do)
        big = 1e300
        halves, everything = ((-big, 2.5), (0.5, big)), ((-big, big),)
        for W in (2, 8):
            per_axis = [halves, halves if W == 8 else everything, halves if W == 8 else everything]
            boxes = [((x[0], y[0], z[0]), (x[1], y[1], z[1])) for z in per_axis[2] for y in per_axis[1] for x in per_axis[0]]
            sizes = _write_window_case(f, mesh, boxes, compliance=(1e-6, 0.0, 0.0), plane=(0.0, 1.0, 0.0, -3.0), plane_on=1)
            by_pos = [len(_numpy_cut((cube.pos, cube.vel, cube.inv_mass, None) + mesh[4:], lo, hi)[0]) for lo, hi in boxes]
            assert len(boxes) == W and 0 < min(sizes) and max(sizes) < 64 and sizes != by_pos, (sizes, by_pos)
            n_boxes += W
        # lattice boxes of the window fuzzer (no rest pose given: the cut goes by position), with masses, velocities and rest lengths of their own
        taken, seed = 0, 0
        while taken < 10:
            sc = fuzz_windows.make_scenario(seed); seed += 1
            rest, ij, W = sc["_rest"], sc["_ij"], sc["world"]
            dom = native.domain_from_mesh(rest, ij)
            boxes = [native.domain_window(dom, r, W, sc["dims"], sc["tile"]) for r in range(W)]
            if any(not np.any(np.all((rest >= lo) & (rest < hi), axis=1)) for lo, hi in boxes):
                continue
            rng = np.random.default_rng(1000 + seed)
            mesh = (rest, rng.normal(size=rest.shape).astype(np.float32), rng.uniform(0.0, 2.0, len(rest)).astype(np.float32), None,
                    [ij, np.zeros((0, 4), np.int32), np.zeros((0, 4), np.int32)],
                    [rng.uniform(0.5, 1.5, (len(ij), 1)).astype(np.float32), np.zeros((0, 1), np.float32), np.zeros((0, 2), np.float32)])
            assert min(_write_window_case(f, mesh, boxes, compliance=(float(np.float32(rng.uniform(0, 1e-3))), 0.0, 0.0))) > 0
            n_boxes += W; taken += 1
        # tets and hinges (kinds 1 and 2, two rest values per hinge): a block of 2 x 2 x 2 cells of six tets each, cut by the plane x = 1
        # through its middle -- once keeping the nodes ON the plane (lo inclusive), once not (hi exclusive) --, and a box that holds no particle
        g = np.arange(3, dtype=np.float64)
        nodes = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + np.random.default_rng(9).uniform(-0.1, 0.1, (27, 3)) * [0, 1, 1]
        node = lambda i, j, k: (i * 3 + j) * 3 + k                                                                # noqa: E731
        tets = []
        for i in range(2):
            for j in range(2):
                for k in range(2):
                    c = [node(i + a, j + b, k + d) for a in (0, 1) for b in (0, 1) for d in (0, 1)]      # corner a b d -> c[4a + 2b + d]
                    tets += [[c[0], c[p], c[q], c[7]] for p, q in ((1, 3), (3, 2), (2, 6), (6, 4), (4, 5), (5, 1))]
        tm = from_tet_mesh(nodes, np.array(tets))
        assert len(tm.vol_rest) == 48 and len(tm.bend_rest) > 0 and tm.bend_rest.shape[1] == 2
        tm.pos = (tm.pos + 0.25).astype(np.float32)
        big = 1e300
        boxes = [((-big, -big, -big), (1.0, big, big)), ((1.0, -big, -big), (big, big, big)), ((5.0, 5.0, 5.0), (6.0, 6.0, 6.0))]
        sizes = _write_window_case(f, _mesh_tuple(tm, True), boxes, compliance=(0.0, 1e-7, 1e-2))
        assert sizes == [9, 18, 0], sizes
        n_boxes += 3
        cases = _setter_cases()
        for case in cases:
            _write_setter_case(f, case)
    exe = str(tmp_path / "authoring_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-pthread", *SAN, "-I", CSRC, os.path.join(ROOT, "tests", "sanitize", "authoring_san.cpp"),
                           os.path.join(CSRC, "authoring.cpp"), os.path.join(CSRC, "plan.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", SB_PLAN_THREADS="4")
    out = subprocess.run([exe, str(corpus)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and f"SANITIZE OK records {13 + len(cases)} boxes {n_boxes} empty 1 setter cases {len(cases)}" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
