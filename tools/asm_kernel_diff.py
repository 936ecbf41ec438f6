"""Compare the instructions of kernels in two assembly listings (hipcc -S --cuda-device-only) of one source file, e.g. before and
after a change that must leave existing instantiations alone.

    python tools/asm_kernel_diff.py parent.s child.s mlp_topk_kernel [--map 'ELi0ENS_6MtArgsEEEvT3_=EEEvNS_6MtArgsE']

Kernels are paired by mangled name (after the optional --map old=new substitutions applied to the child's names, for a kernel that
gained template parameters); block labels are renumbered per kernel, comments and directives dropped.  Prints one line per kernel
of the parent whose name contains the pattern: identical / DIFFERENT (with the first differing lines) / missing.  Exit status 1 if
any differs or is missing."""
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
                continue
            t = line.split(";")[0].rstrip()
            if not t.strip() or t.lstrip().startswith("."):
                if not re.match(r"^\.LBB\d+_\d+:", t):
                    continue
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return out


def main():
    parent, child, pat = sys.argv[1:4]
    maps = [a.split("=", 1) for a in sys.argv[5:]] if len(sys.argv) > 4 and sys.argv[4] == "--map" else []
    kp, kc0 = kernels(parent), kernels(child)
    kc = {}
    for n, b in kc0.items():
        for old, new in maps:
            n = n.replace(old, new)
        kc[n] = b
    bad = 0
    for n, b in kp.items():
        if pat not in n:
            continue
        if n not in kc:
            print("missing  ", n)
            bad = 1
        elif kc[n] == b:
            print("identical", n, len(b), "lines")
        else:
            bad = 1
            print("DIFFERENT", n, len(b), "vs", len(kc[n]), "lines")
            for i, (x, y) in enumerate(zip(b, kc[n])):
                if x != y:
                    print("   first difference at line", i, "\n   <", x, "\n   >", y)
                    break
    return bad


if __name__ == "__main__":
    sys.exit(main())
