"""Previous positions as 8-byte codes against x (softbodyunity_amd/csrc/prev_code.hpp) and the rule that decides which solvers use
them (launch_shape.hpp use_prev_codes), checked on the CPU: tests/sanitize/prev_code_check.cpp, built with AddressSanitizer and
UBSan, round-trips the code bit for bit at the boundaries of its fields, at zeros, denormals, sign changes, infinities and NaNs with
payloads and over more than a million random pairs, compares `fits` with the definition computed in 64-bit arithmetic, and walks the
decision function over its inputs."""
import os
import subprocess

from test_tables_digest import CSRC, FLAGS, SAN


def test_the_previous_position_code_round_trips_and_the_decision_rule_holds(tmp_path):
    exe = os.path.join(str(tmp_path), "prev_code_check")
    subprocess.check_call(["g++", *FLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Werror", "-I", CSRC,
                           os.path.join(SAN, "prev_code_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = dict(line.split() for line in out.stdout.splitlines())
    assert int(got["pairs"]) >= 1_600_000
    assert 0.3 * int(got["pairs"]) < int(got["fitting"]) < 0.9 * int(got["pairs"])      # both outcomes are well covered
    assert int(got["decisions"]) >= 40
