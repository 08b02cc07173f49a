"""The tables the kernels read, pinned on the CPU: tests/sanitize/tables_digest.cpp plans a fixed corpus, has
softbodyunity_amd/csrc/tables_host.cpp build the tables of every rank and prints one 64-bit digest per case over everything in
HostTables, and over the device bytes the DRIVER sums from the sizes of those tables (the parent's driver digests build_device's
own dev_bytes there, so the golden file pins the sum; tables.hip's own accounting and allocation order are seen by the GPU suite
only); the digests must equal tests/golden/tables_digests.json, whatever the
number of host threads. With --paths the driver also says which branches of the builder each case reached; every branch listed
in REQUIRED_PATHS must be reached by some case.

The golden file is never written from the code under test. A pull request that MEANS to change the tables regenerates it from
its own builder and says so (`--regenerate` without a directory); one that means to leave them alone generates it from the PARENT
commit's sources:

    mkdir /tmp/parent && git archive HEAD~1 softbodyunity_amd/csrc include | tar -x -C /tmp/parent
    python tests/test_tables_digest.py --regenerate /tmp/parent/softbodyunity_amd/csrc

If that directory has no tables_host.cpp, its tables.hip is the build_device that uploads as it goes: it is compiled for the host
with g++, the HIP memory calls it makes renamed to host-memory stand-ins of the driver (-DhipMalloc=sb_host_malloc ...), an
sb_solver is filled by hand and what its device buffers then point at is digested (tables_digest.cpp, TABLES_DIGEST_PARENT).

The file in the tree was generated that way from d89c39c, the parent of the commit that split build_device into a host builder
and an upload.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "softbodyunity_amd", "csrc")
SAN = os.path.join(ROOT, "tests", "sanitize")
GOLDEN = os.path.join(ROOT, "tests", "golden", "tables_digests.json")
# the Makefile's flags for tables_host.cpp: the HIP headers only give kernel_types.hpp its vector types, no HIP library is linked
FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-attributes", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", SAN]
HIP_STAND_INS = {"hipMalloc": "sb_host_malloc", "hipMemcpy": "sb_host_memcpy", "hipMemset": "sb_host_memset", "hipFree": "sb_host_free",
                 "hipExtMallocWithFlags": "sb_host_ext_malloc", "hipHostMalloc": "sb_host_host_malloc", "hipHostFree": "sb_host_host_free"}

REQUIRED_PATHS = {
    "mass_palette", "float_masses", "uniform_mass",
    "boundary_order_t0_w2", "boundary_order_t1_w2", "boundary_order_t0_w8", "boundary_order_t1_w8",
    "multi_member_packs", "run_overflow", "t2_gather_layers",
    "dictionary_slots", "full_slots", "palette_overflow",
    "wave_items_256", "wave_items_512",
    "lane_packed_compact", "lane_packed_full", "wide_packed",
    "tet_slots", "hinge_slots",
    "shared_programs", "unshared_programs",
    "cost_order_one_range", "cost_order_split_ranges", "cost_order_t2_layers",
    "gcolour_type0", "gcolour_type1", "gcolour_type2",
    "fused_unpack", "no_fused_unpack",
    "mailbox_w2", "mailbox_w8",
}
# every switch build_device reads has a case of its own (SB_TUNE_PEER_COARSE only picks the mailbox's allocator: not a table)
REQUIRED_CASES = {"tune_no_mass_palette_w1_t64", "tune_no_uniform_mass_w1_t64", "tune_no_palette_w1_t64", "tune_no_wave_items_w1_t128",
                  "tune_no_lane_pack_w1_t64", "tune_no_cost_order_w1_t128", "tune_no_fused_unpack_w2_t64", "tune_no_wide_slots_w1_t512",
                  "tune_no_shared_programs_w1_t64", "tune_no_pack_w1_t64", "tune_win_dwords_w1_t512", "tune_tile_lanes256_w1_t64",
                  "tune_tile_lanes128_w1_t512"}


def _build(out_dir, csrc=CSRC):
    exe = os.path.join(str(out_dir), "tables_digest")
    driver = os.path.join(SAN, "tables_digest.cpp")
    if os.path.exists(os.path.join(csrc, "tables_host.cpp")):
        cmd = ["g++", *FLAGS, "-I", csrc, driver, os.path.join(csrc, "tables_host.cpp"), os.path.join(csrc, "plan.cpp")]
    else:
        cmd = ["g++", *FLAGS, "-DTABLES_DIGEST_PARENT", *[f"-D{k}={v}" for k, v in HIP_STAND_INS.items()], "-I", csrc, driver,
               "-x", "c++", os.path.join(csrc, "tables.hip"), "-x", "none", os.path.join(csrc, "plan.cpp")]
    subprocess.check_call(cmd + ["-o", exe])
    return exe


def _run(exe, threads, *args):
    out = subprocess.run([exe, *args], capture_output=True, text=True, env=dict(os.environ, SB_PLAN_THREADS=str(threads)), timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    pairs = [line.split() for line in out.stdout.splitlines()]
    assert len({name for name, _ in pairs}) == len(pairs), "duplicate case names"
    return dict(pairs), out.stderr


def test_every_table_of_every_rank_matches_the_golden_digests(tmp_path):
    exe = _build(tmp_path)
    with open(GOLDEN) as f:
        want = json.load(f)
    assert len(want) >= 40 and REQUIRED_CASES <= set(want)
    for threads, args in ((1, ()), (4, ("--paths",))):      # (the host threads read SB_PLAN_THREADS once per process)
        got, err = _run(exe, threads, *args)
        missing, extra = sorted(set(want) - set(got)), sorted(set(got) - set(want))
        different = sorted(name for name in want if name in got and got[name] != want[name])
        assert not (missing or extra or different), f"SB_PLAN_THREADS={threads}: missing {missing}, extra {extra}, different {different}"
    reached = set()
    for line in err.splitlines():
        if line.startswith("paths "):
            reached |= set(line.split()[2:])
    assert not (REQUIRED_PATHS - reached), f"branches of the table builder no case reaches: {sorted(REQUIRED_PATHS - reached)}"


if __name__ == "__main__":
    import tempfile
    assert len(sys.argv) >= 2 and sys.argv[1] == "--regenerate", __doc__
    with tempfile.TemporaryDirectory() as tmp:
        exe = _build(tmp, os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else CSRC)
        digests = _run(exe, 1)[0]
        assert digests == _run(exe, 4)[0], "the digests depend on the thread count"
    with open(GOLDEN, "w") as f:
        json.dump(digests, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(digests)} digests to {GOLDEN}")
