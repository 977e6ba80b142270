#!/bin/bash
# VGPR / SGPR / scratch / LDS of the kernels in a built library (code object metadata), over every gfx950 code
# object of the library (each source file contributes one); by default the one-pass march kernels:
# scripts/kernel_resources.sh [lib.so] [symbol regex]
set -eu
LIB=${1:-ocean_model_arch_amd/libocn_sw.so}
PAT=${2:-MarchStep}
HERE=$(cd "$(dirname "$0")" && pwd)
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
python3 - "$LIB" "$T" "$HERE/../ocean_model_arch_amd" <<'EOF'
import os, sys
sys.path.insert(0, sys.argv[3])
import _codeobj  # (the module alone: the package's import needs the built library)
for i, code in enumerate(_codeobj.gfx950_code_objects(sys.argv[1])):
    with open(os.path.join(sys.argv[2], f"co{i}.o"), "wb") as f:
        f.write(code)
EOF
for CO in "$T"/co*.o; do
/opt/rocm/lib/llvm/bin/llvm-readelf --notes "$CO" | python3 -c '
import sys, re
txt = sys.stdin.read()
pat = re.compile(sys.argv[1])
for blk in txt.split("\n  - .agpr_count")[1:]:
    name = re.search(r"\.name:\s+(\S+)", blk)
    if not name or not pat.search(name.group(1)): continue
    g = lambda k: (re.search(r"\." + k + r":\s+(\S+)", blk) or [None, "?"])[1]
    print(g("vgpr_count"), g("sgpr_count"), g("private_segment_fixed_size"), g("group_segment_fixed_size"), name.group(1))
' "$PAT"
done
