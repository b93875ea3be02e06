"""Disassemble one kernel of a built object or library (development tool).
Usage: python tools/isa.py FILE.o|.so 'kernel-name-regex' > out.s"""
import re
import sys

from codeobj import code_object, llvm


def main(path, pat):
    with code_object(path) as co:
        txt = llvm("llvm-objdump", "-d", "--no-show-raw-insn", "-C", co)
    rx = re.compile(pat)
    on = False
    for line in txt.splitlines():
        if line and not line.startswith(" ") and line.endswith(">:"):
            on = bool(rx.search(line))
        if on:
            print(line)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
