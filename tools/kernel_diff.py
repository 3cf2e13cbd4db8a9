"""Compare the device code of two builds of the library, kernel by kernel.

Takes every gfx950 code object of both libraries (tools/kernel_resources.code_objects), disassembles it (llvm-objdump
-d, each line cut before its address and instruction bytes, the zero fill between symbols dropped: two builds of one
source differ in object bytes and kernel placement, not in instruction text) and hashes each kernel symbol's text.
Prints the symbols that were added, dropped or changed; a host-side refactor must leave none. It only compares: no
instruction is looked at for what it is.
Usage: python tools/kernel_diff.py A.so B.so   (exit status 1 when anything differs)"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

from kernel_resources import LLVM, code_objects, demangle

_SYM = re.compile(r"^[0-9a-f]+ <([^>]+)>:$")


def kernel_hashes(lib):
    """{symbol: sha256 of its disassembly} over every function of every gfx950 code object of `lib`."""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for k, co in enumerate(code_objects(lib)):
            f = os.path.join(d, f"co{k}.elf")
            with open(f, "wb") as fh:
                fh.write(co)
            txt = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", f], check=True, capture_output=True,
                                 text=True).stdout
            name, h = None, None
            for line in txt.splitlines():
                m = _SYM.match(line)
                if m:
                    if name:
                        out[name] = h.hexdigest()
                    name, h = m.group(1), hashlib.sha256()
                elif name and line.strip() not in ("", "..."):  # "...": zero fill up to the next symbol's alignment
                    h.update(line.split("//")[0].strip().encode() + b"\n")
            if name:
                out[name] = h.hexdigest()
    return out


def main(argv):
    if len(argv) != 2:
        print(__doc__)
        return 2
    a, b = kernel_hashes(argv[0]), kernel_hashes(argv[1])
    rows = [("dropped", s) for s in sorted(set(a) - set(b))] + [("added", s) for s in sorted(set(b) - set(a))]
    rows += [("changed", s) for s in sorted(set(a) & set(b)) if a[s] != b[s]]
    for (what, _), dn in zip(rows, demangle([s for _, s in rows])):
        print(f"{what:8s}{dn}")
    print(f"{len(a)} kernels, {len(rows)} differ")
    return 1 if rows else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
