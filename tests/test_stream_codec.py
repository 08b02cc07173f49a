"""The bit layout of the tile constraint stream (softbodyunity_amd/csrc/stream_codec.hpp), checked on the CPU:
tests/sanitize/stream_codec_check.cpp encodes and decodes every form at the corners of its fields -- round trip through the struct
decoders and the single-field accessors -- and compares every encoder and decoder with the expressions the table builder, the tile
kernel and the validator held before the codec existed (transcribed into the driver). The number of points is counted here
independently: the driver may skip none."""
import itertools
import os
import subprocess

from test_tables_digest import CSRC, FLAGS, SAN


def _points():
    counts, local_indices, palette = (0, 1, 256, 1023), (0, 511, 4095, 65535), (0, 7, 255)
    n = len(list(itertools.product(counts, counts, counts, (False, True))))                      # group word
    n += len(list(itertools.product(local_indices[:3], local_indices[:3], palette)))             # dictionary-coded slot: 12-bit indices
    n += len(list(itertools.product(local_indices, local_indices)))                              # index pair of a full slot
    n += len(list(itertools.product(*[local_indices] * 4)))                                      # four-vertex slot
    n += len(list(itertools.product(range(5), (0, 1, 64, 127), (False, True), (0, 2 ** 21 - 1)))) + 1     # wave item, + "2^21 does not fit"
    n += len(list(itertools.product((0, 511), (0, 511), (0, 7)))) + 3                            # lane-pack field, + one range violation per part
    n += 6 * 2 + 1                                                                               # fields of a 16-byte word, two values each, + a full word
    n += 3 * 2 + 1                                                                               # fields of an 8-byte word
    n += 6 * 2                                                                                   # rest-length dword: field x {first, last lane}
    return n


def test_the_stream_codec_round_trips_and_equals_the_parents_expressions(tmp_path):
    exe = os.path.join(str(tmp_path), "stream_codec_check")
    subprocess.check_call(["g++", *FLAGS, "-Werror", "-I", CSRC, os.path.join(SAN, "stream_codec_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = dict(line.split() for line in out.stdout.splitlines())
    assert int(got["points"]) == _points() > 0
