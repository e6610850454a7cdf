"""Per-kernel hashes of two gfx950 assembly files (hipcc -S --cuda-device-only of the same unit, e.g. the parent's and this tree's attention.hip):
which kernels compile to the ISA they compiled to before. A kernel's text runs from its label to its kernel descriptor; comments are dropped and the
function-index part of local labels (.LBB<i>_<n>, .Lfunc_end<i>, ...) is normalised, since adding a kernel renumbers the functions behind it.

    python tools/isa_kernel_hashes.py parent.s new.s > profiles/<record>.txt        (exit status 1 if a kernel of the first file changed or is gone)"""
import hashlib
import re
import subprocess
import sys


def kernels(path):
    out, cur, name = {}, None, None
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is None:
            continue
        if ln.startswith(".Lfunc_end") or ".amdhsa_kernel " in ln:  # (the kernel descriptor, which holds the kernarg size, is not ISA)
            if name not in out:
                out[name] = hashlib.sha256("\n".join(cur).encode()).hexdigest()[:16], len(cur)
            cur = None
            continue
        ln = ln.split(";")[0].rstrip()
        if ln.strip() and not ln.strip().startswith((".section", ".p2align")):
            cur.append(re.sub(r"\.L(BB|tmp|func_begin|func_end)(\d+)", r".L\1#", ln))
    return out


def main(a, b):
    ka, kb = kernels(a), kernels(b)
    names = subprocess.run(["c++filt"], input="\n".join(list(ka) + [n for n in kb if n not in ka]), capture_output=True, text=True).stdout.split("\n")
    changed = 0
    print(f"{'parent':16}  {'this tree':16}  {'insns+labels':>12}  kernel")
    for n, pretty in zip(list(ka) + [n for n in kb if n not in ka], names):
        ha, hb = ka.get(n, ("-", 0)), kb.get(n, ("-", 0))
        state = "same" if ha[0] == hb[0] else "NEW" if n not in ka else "CHANGED"
        changed += state == "CHANGED"
        print(f"{ha[0]:16}  {hb[0]:16}  {max(ha[1], hb[1]):12d}  {state:7}  {pretty.replace('(anonymous namespace)::', '')}")
    print(f"{len(ka)} kernels in the parent's unit, {sum(1 for n in kb if n not in ka)} new, {changed} changed")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
