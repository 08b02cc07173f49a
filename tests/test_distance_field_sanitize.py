"""The host code that validates and sizes a signed-distance table and a pose (SPEC.md 2i: validate_distance_field and
validate_distance_field_pose in softbodyunity_amd/csrc/distance_field.hip) under AddressSanitizer and UndefinedBehaviorSanitizer, as a
stand-alone program of its own (tests/sanitize/distance_field_validate_san.cpp, in the way of tests/test_sanitizers.py): the unit is
compiled with the sanitizers on its HOST side alone and linked with the program, which calls the two validators and nothing else -- no
group, no device, no kernel is launched. It hands in arrays exactly as long as the descriptor says, so a read past the end is reported."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "softbodyunity_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]


def test_the_validators_run_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "distance_field_validate_san")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-Wall", "-Wno-unused-result", "-Wno-option-ignored", "-ffp-contract=off", *SAN,
                           "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-x", "hip", os.path.join(CSRC, "distance_field.hip"),
                           os.path.join(ROOT, "tests", "sanitize", "distance_field_validate_san.cpp"), "-fsanitize=address,undefined", "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("DISTANCE FIELD VALIDATE OK "), out.stdout[-1000:] + out.stderr[-3000:]
    assert int(out.stdout.split()[-1]) > 100 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
