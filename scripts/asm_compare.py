"""Compare the device code of two `hipcc --offload-arch=gfx950 --cuda-device-only -S` outputs kernel by kernel: instruction bodies with
comments and basic-block numbers stripped, and the kernel descriptors (registers, LDS, scratch, argument size).  Needs no GPU.

    python scripts/asm_compare.py parent.s change.s        # prints SAME / DIFF per kernel of the first file, and the new kernels
    python scripts/asm_compare.py --work parent.s change.s # next to it the verdict over the instructions that do the work, and the lines
                                                           # that differ

--work: a refactor that hoists code into functions may reorder integer moves or change the signedness of a compare without touching
what the kernel computes or how it touches memory.  WORK-SAME says that the descriptor and the number of instructions are equal and that
the instructions whose mnemonic contains `_f64`, starts with `ds_`, `global_` or `flat_`, or is `s_barrier` are the same sequence,
operands included; WORK-RENAMED that only register names differ in that sequence (those lines are printed after `work`).  The exit
status stays that of the strict comparison.
"""
import difflib
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


def instructions(body):
    """the lines of a body that are instructions: no labels, no directives"""
    return [c for c in body if not c.endswith(":") and not c.startswith(".")]


def work(body):
    def keep(code):
        op = code.split()[0]
        return "_f64" in op or op.startswith(("ds_", "global_", "flat_")) or op == "s_barrier"
    return [c for c in instructions(body) if keep(c)]


def main(argv):
    filtered = "--work" in argv
    a_path, b_path = [v for v in argv if v != "--work"]
    a, b = bodies(a_path), bodies(b_path)
    da, db = descriptors(a_path), descriptors(b_path)
    same = True
    for k in sorted(a):
        ok = a[k] == b.get(k) and da.get(k) == db.get(k)
        same = same and ok
        verdict = "SAME" if ok else "DIFF"
        if filtered and k in b:
            ia, ib = instructions(a[k]), instructions(b[k])
            wa, wb = work(a[k]), work(b[k])
            frame = da.get(k) == db.get(k) and len(ia) == len(ib)
            renamed = frame and [c.split()[0] for c in wa] == [c.split()[0] for c in wb]
            verdict += " WORK-SAME" if frame and wa == wb else " WORK-RENAMED" if renamed else " WORK-DIFF"
            print("%s %s (%d instructions, %d that work; change: %d, %d)" % (verdict, k, len(ia), len(wa), len(ib), len(wb)))
            if renamed:
                for x, y in zip(wa, wb):
                    if x != y:
                        print("    work -%s\n    work +%s" % (x, y))
            if not ok:
                for line in difflib.unified_diff(a[k], b[k], "parent", "change", n=0, lineterm=""):
                    if not line.startswith(("---", "+++", "@@")):
                        print("    " + line)
                if da.get(k) != db.get(k):
                    for line in difflib.unified_diff(da[k].split("\n"), db[k].split("\n"), "parent", "change", n=0, lineterm=""):
                        if not line.startswith(("---", "+++", "@@")):
                            print("    descriptor " + line.strip())
        else:
            print("%s %s (%d lines)" % (verdict, k, len(a[k])))
    for k in sorted(set(b) - set(a)):
        print("NEW  %s (%d lines)" % (k, len(b[k])))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
