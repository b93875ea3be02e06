"""Compare the gfx950 code objects of two builds (development tool): did a source change alter
the compiled device code?
Usage: python tools/codeobj_diff.py DIR_A DIR_B   (two build/obj/<lib> directories of
_lib.build(out=...)).  Per object: whether the .text bytes match (sha256); if not, the
functions whose disassembly differs or that only one side has; whether function order and the
kernels' metadata notes (kernel_resources.notes) differ.  Exits 1 on any difference."""
import hashlib
import os
import re
import subprocess
import sys

from codeobj import code_object, llvm
from kernel_resources import notes


def read(path):
    """(.text sha256, [(mangled function, disassembly without addresses)] in code order)."""
    with code_object(path) as co:
        text = co + ".text"
        llvm("llvm-objcopy", f"--dump-section=.text={text}", co)
        with open(text, "rb") as f:
            sha = hashlib.sha256(f.read()).hexdigest()
        asm = llvm("llvm-objdump", "-d", "--no-show-raw-insn", co)
    funcs = []
    for line in asm.splitlines():
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m:
            funcs.append((m.group(1), []))
        elif funcs and line.strip():
            funcs[-1][1].append(re.sub(r"\s*//.*$", "", line))  # (the trailing comment is the address)
    return sha, [(n, "\n".join(body)) for n, body in funcs]


def demangle(names):
    return subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()


def compare(a, b):
    """Print the differences of objects a and b; returns whether there were any."""
    (sha_a, fa), (sha_b, fb) = read(a), read(b)
    da, db = dict(fa), dict(fb)
    changed = [n for n, _ in fa if n in db and da[n] != db[n]]
    only = [(n, "A") for n, _ in fa if n not in db] + [(n, "B") for n, _ in fb if n not in da]
    order = [n for n, _ in fa if n in db] != [n for n, _ in fb if n in da]
    na, nb = ({k["name"]: k for k in notes(p)} for p in (a, b))
    print(f"  .text sha256 {'same' if sha_a == sha_b else 'DIFFERS'} ({len(fa)} / {len(fb)} functions), "
          f"function order {'DIFFERS' if order else 'same'}, kernel metadata {'DIFFERS' if na != nb else 'same'}")
    for n in demangle(changed):
        print(f"    body differs: {n}")
    for n, (_, side) in zip(demangle([n for n, _ in only]), only):
        print(f"    only in {side}: {n}")
    for name in sorted(set(na) | set(nb)):
        if na.get(name) != nb.get(name):
            print(f"    metadata: {na.get(name, 'only in B')} -> {nb.get(name, 'only in A')}")
    return sha_a != sha_b or order or bool(only) or na != nb


def main(dir_a, dir_b):
    names = [sorted(f for f in os.listdir(d) if f.endswith(".o")) for d in (dir_a, dir_b)]
    differs = names[0] != names[1]
    for f in sorted(set(names[0]) ^ set(names[1])):
        print(f"{f}: only in {dir_a if f in names[0] else dir_b}")
    for f in sorted(set(names[0]) & set(names[1])):
        print(f"{f}:")
        differs = compare(os.path.join(dir_a, f), os.path.join(dir_b, f)) or differs
    print("DIFFERENT" if differs else "identical")
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
