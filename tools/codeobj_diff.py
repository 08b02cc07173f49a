#!/usr/bin/env python3
"""Kernels of two gfx950 assembly listings (hipcc ... --cuda-device-only -S), compared per kernel symbol: the .amdhsa_* descriptor block
line by line and the instruction text (labels kept, comments and directives dropped, the function index inside block labels masked).
The method of profiles/r12_tile_stages_codeobj.txt and r13_prev_code_codeobj.txt.

usage: tools/codeobj_diff.py before.s after.s [--strip-default ARG ...]
  --strip-default: trailing template arguments, in their mangled spelling (e.g. Li0E), that the newer listing spells out behind the
  older one's last argument: a kernel of `after` whose name carries them is matched with the name without them.
Exit status 1 if a kernel of `before` is missing in `after` or differs."""
import re
import sys


def kernels(path):
    """name -> (descriptor lines, instruction lines, figures)"""
    out, text = {}, open(path).read()
    desc = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        desc[m.group(1)] = [ln.strip() for ln in m.group(2).splitlines() if ln.strip()]
    for name in desc:
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, re.S | re.M)
        body = []
        for ln in m.group(1).splitlines():
            ln = ln.split(";")[0].rstrip()
            if not ln.strip() or ln.strip().startswith("."):
                if re.match(r"\.LBB\d+_\d+:", ln.strip()):
                    body.append(re.sub(r"\.LBB\d+_", ".LBB_", ln.strip()))
                continue
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", ln.strip()))
        fig = {}
        for key in ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size", "accum_offset"):
            for ln in desc[name]:
                if ln.startswith(".amdhsa_" + key + " "):
                    fig[key] = ln.split()[1]
        out[name] = (desc[name], body, fig)
    return out


def main():
    args = sys.argv[1:]
    strip = []
    if "--strip-default" in args:
        k = args.index("--strip-default")
        strip, args = args[k + 1:], args[:k]
    before, after = kernels(args[0]), kernels(args[1])
    tail = "".join(strip)
    renamed = {}
    for name in after:
        if tail and (tail + "EEv") in name:
            renamed[name.replace(tail + "EEv", "EEv", 1)] = name
    missing = same = diff_desc = diff_text = 0
    for name, (d0, b0, _) in sorted(before.items()):
        other = name if name in after else renamed.get(name)
        if other is None:
            missing += 1
            print("missing in after:", name)
            continue
        d1, b1, _ = after[other]
        if d0 != d1:
            diff_desc += 1
            print("descriptor differs:", name)
        if b0 != b1:
            diff_text += 1
            print("instruction text differs:", name)
        elif d0 == d1:
            same += 1
    matched = {n if n in after else renamed.get(n) for n in before}
    print(f"kernels: before {len(before)} after {len(after)}")
    print(f"missing in after: {missing}; descriptor differences: {diff_desc}; instruction text differences: {diff_text}; identical: {same}")
    sizes = [len(b) for _, b, _ in before.values()]
    print(f"instructions compared per kernel: {min(sizes)} .. {max(sizes)}")
    print("new kernels (name vgpr sgpr lds private accum_offset):")
    for name, (_, _, f) in sorted(after.items()):
        if name not in matched:
            print(name, f.get("next_free_vgpr"), f.get("next_free_sgpr"), f.get("group_segment_fixed_size"), f.get("private_segment_fixed_size"), f.get("accum_offset"))
    return 1 if missing or diff_desc or diff_text else 0


if __name__ == "__main__":
    sys.exit(main())
