#!/usr/bin/env python3
"""Compare the gfx950 machine code of two builds of libocn_sw.so, kernel by kernel.

    python scripts/codeobj_diff.py parent/libocn_sw.so new/libocn_sw.so

Takes the function symbols over every gfx950 code object of each library (each object file contributes
one) and compares them in the position-independent form of _codeobj (a pc-relative literal that addresses
a device global is replaced by the global's name and offset).  Prints

  * the symbols only one library has,
  * the symbols whose bytes differ,
  * the symbols that are equal only after the replacement (their count; the raw bytes differ by the
    distance to the global alone: the code around them moved),
  * the symbols that more than one code object of a library holds (a kernel template instantiated from
    two sources: two code objects registered under one host stub),

and exits non-zero on anything but the third kind: a host-only change leaves every kernel byte for byte
what it was, wherever its source moved.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ocean_model_arch_amd"))
import _codeobj  # noqa: E402  (the module alone: the package's import needs the built library)


def main(argv):
    if len(argv) != 3:
        raise SystemExit(__doc__)
    a, b = _codeobj.library_kernels(argv[1]), _codeobj.library_kernels(argv[2])
    bad = moved = 0
    for path, lib in {argv[1]: a, argv[2]: b}.items():
        for name in sorted(lib):
            if len(lib[name]) > 1:
                print(f"in {len(lib[name])} code objects of {path}: {name}")
                bad += 1
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"only in {argv[2] if name in b else argv[1]}: {name}")
        elif a[name][0][1] != b[name][0][1]:
            print(f"bytes differ ({len(a[name][0][0])} / {len(b[name][0][0])}): {name}")
        else:
            moved += a[name][0][0] != b[name][0][0]
            continue
        bad += 1
    print(f"{len(a)} / {len(b)} function symbols, {bad} missing or different or duplicated, "
          f"{moved} equal only after the literal replacement")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
