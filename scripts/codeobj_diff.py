#!/usr/bin/env python3
"""Compare the gfx950 machine code of two builds of libocn_sw.so, kernel by kernel.

    python scripts/codeobj_diff.py parent/libocn_sw.so new/libocn_sw.so

Takes the union of the function symbols over every gfx950 code object of each library (each object file
contributes one), prints the symbols only one library has and the symbols whose bytes differ, and exits
non-zero if there are any: a host-only change leaves every kernel byte for byte what it was, wherever
its source moved.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ocean_model_arch_amd"))
import _codeobj  # noqa: E402  (the module alone: the package's import needs the built library)


def symbols(lib_path):
    out = {}
    for code in _codeobj.gfx950_code_objects(lib_path):
        for name, body in _codeobj.kernel_symbols(code).items():
            if out.setdefault(name, body) != body:
                raise SystemExit(f"{lib_path}: {name} has different bytes in two code objects")
    return out


def main(argv):
    if len(argv) != 3:
        raise SystemExit(__doc__)
    a, b = symbols(argv[1]), symbols(argv[2])
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"only in {argv[2] if name in b else argv[1]}: {name}")
        elif a[name] != b[name]:
            print(f"bytes differ ({len(a[name])} / {len(b[name])}): {name}")
        else:
            continue
        bad += 1
    print(f"{len(a)} / {len(b)} function symbols, {bad} missing or different")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
