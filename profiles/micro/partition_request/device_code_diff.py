"""Compare the device code of two builds of one .hip file, kernel by kernel.

    hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S FILE.hip -o a.s     (once per tree)
    python device_code_diff.py a.s b.s

A host-only change must leave every kernel as it was: the same set of kernel symbols, each with an identical body and an identical
.amdhsa_ descriptor block.  The order in which the kernels are emitted may differ (template instances follow their first use in host
code) and with it the function index inside local labels (.LBB<index>_<block>), and so do the lines that name __hip_cuid_<hash of the source>.  Prints one line per file pair; exit status 1 on a difference."""
import re
import sys


def kernels(path):
    """{symbol: (body lines, descriptor lines)} of an AMDGPU assembly file"""
    text = open(path).read().split("\n")
    out, name, body = {}, None, []
    desc, in_desc = {}, None
    for line in text:
        if "__hip_cuid_" in line:
            continue
        m = re.match(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$", line)
        if m and not m.group(1).startswith((".L", "__unnamed")):
            name, body = m.group(1), []
            out[name] = body
            continue
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            in_desc = m.group(1)
            desc[in_desc] = []
            name = None
            continue
        if in_desc is not None:
            if re.match(r"^\s*\.end_amdhsa_kernel", line):
                in_desc = None
            else:
                desc[in_desc].append(line.strip())
            continue
        if re.match(r"^\s*\.(section|text|rodata|amdgpu_metadata)", line) or re.match(r"^\s*\.Lfunc_end", line):
            name = None if re.match(r"^\s*\.(section|amdgpu_metadata)", line) else name
        if name is not None:
            # (local labels carry the function's index in the file, .LBB<index>_<block>: the index follows the emission order)
            line = re.sub(r"\bHeader=BB\d+_", "Header=BB_", re.sub(r"\s+", " ", line.strip()))      # (the same index in a comment)
            body.append(re.sub(r"\.L(BB|tmp|func_begin|func_end)\d+_?", r".L\1_", line))
    return {k: (out.get(k, []), desc[k]) for k in desc}


def main(a, b):
    ka, kb = kernels(a), kernels(b)
    only = sorted(set(ka) ^ set(kb))
    differ = sorted(k for k in set(ka) & set(kb) if ka[k] != kb[k])
    print("%s vs %s: %d / %d kernels, %d only in one, %d differ" % (a, b, len(ka), len(kb), len(only), len(differ)))
    for k in only + differ:
        print("   ", k)
    return 1 if only or differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
