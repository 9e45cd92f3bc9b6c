"""Compare the device code of two `hipcc --offload-arch=gfx950 --cuda-device-only -S` outputs kernel by kernel: instruction bodies with
comments and basic-block numbers stripped, and the kernel descriptors (registers, LDS, scratch, argument size).  Needs no GPU.

    python scripts/asm_compare.py parent.s change.s        # prints SAME / DIFF per kernel of the first file, and the new kernels
"""
import re
import sys


def bodies(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z[^:\s]+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur and re.match(r"^\s*\.Lfunc_end", line):
            cur = None
            continue
        if cur:
            code = re.sub(r"\.LBB\d+_\d+", ".LBB", line.split(";")[0]).strip()
            if code:
                out[cur].append(code)
    return out


def descriptors(path):
    text = open(path).read()
    return {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S)}


def main(a_path, b_path):
    a, b = bodies(a_path), bodies(b_path)
    da, db = descriptors(a_path), descriptors(b_path)
    same = True
    for k in sorted(a):
        ok = a[k] == b.get(k) and da.get(k) == db.get(k)
        same = same and ok
        print("%s %s (%d lines)" % ("SAME" if ok else "DIFF", k, len(a[k])))
    for k in sorted(set(b) - set(a)):
        print("NEW  %s (%d lines)" % (k, len(b[k])))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
