"""The gfx950 machine code of one kernel in a built libocn_sw.so, for profile provenance.

A committed counter summary (profiles/sq_valu.json, profiles/pmc_traffic.json) describes one kernel's
dispatches on one workload.  bench.py uses it when it was taken on the same library build
(ocn_build_id) -- or, with ``code_sha`` recorded per kernel, when the loaded library's code for that
kernel is byte for byte the code that was profiled (sha256 of the function's bytes in the gfx950 code
object), so that host-side or other-kernel changes do not void a measurement of unchanged machine code.

The bytes are hashed in a position-independent form (position_independent): a kernel that addresses a
device global (the pair kernels' g_clk) holds the distance from the instruction to the global as a
literal, and that distance changes whenever code moves in or out of its code object although no
instruction does.  Such a literal is replaced by the global's name and offset; a function without one
hashes as its raw bytes.

Pure Python, no GPU and no ROCm tools: the .hip_fatbin section's clang offload bundles are parsed for
the gfx950 entries (one per object file with device code), and those ELFs' symbol tables for the
kernel's function bytes.
"""
from __future__ import annotations

import hashlib
import struct

_BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _sections(elf: bytes):
    """{name: (offset, size, addr)} of an ELF64 little-endian image."""
    if elf[:4] != b"\x7fELF" or elf[4] != 2 or elf[5] != 1:
        raise ValueError("not an ELF64 little-endian image")
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    hdrs = []
    for i in range(shnum):
        name, _typ, _flags, addr, off, size = struct.unpack_from("<IIQQQQ", elf, shoff + i * shentsize)
        hdrs.append((name, addr, off, size))
    stroff = hdrs[shstrndx][2]
    out = {}
    for i, (name, addr, off, size) in enumerate(hdrs):
        end = elf.index(b"\0", stroff + name)
        out[elf[stroff + name:end].decode()] = (off, size, addr, i)
    return out


def gfx950_code_objects(lib_path: str):
    """Every gfx950 code object (ELF) bundled in the library's .hip_fatbin section, in link order: one
    per object file that holds device code."""
    data = open(lib_path, "rb").read()
    off, size, _addr, _i = _sections(data)[".hip_fatbin"]
    fat = data[off:off + size]
    pos = fat.find(_BUNDLE_MAGIC)
    while pos >= 0:
        n, = struct.unpack_from("<Q", fat, pos + 24)
        p = pos + 32
        for _ in range(n):
            eoff, esize, tlen = struct.unpack_from("<QQQ", fat, p)
            triple = fat[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if triple.endswith("gfx950"):
                yield fat[pos + eoff:pos + eoff + esize]
        pos = fat.find(_BUNDLE_MAGIC, pos + 1)


def _symbols(code: bytes, typ: int):
    """(mangled name, address, size, file offset) of the code object's sized symbols of ELF type typ."""
    secs = _sections(code)
    symoff, symsize, _a, _i = secs[".symtab"]
    stroff = secs[".strtab"][0]
    by_index = {v[3]: v for v in secs.values()}
    for k in range(symsize // 24):
        st_name, st_info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", code, symoff + 24 * k)
        if (st_info & 0xF) != typ or size == 0 or shndx not in by_index:
            continue
        end = code.index(b"\0", stroff + st_name)
        off, _s, addr, _i = by_index[shndx]
        yield code[stroff + st_name:end].decode(), value, size, off + (value - addr)


def kernel_symbols(code: bytes) -> dict:
    """{mangled name: function bytes} of the code object's function symbols."""
    return {name: code[start:start + size] for name, _addr, size, start in _symbols(code, 2)}   # STT_FUNC


def kernel_addresses(code: bytes) -> dict:
    """{mangled name: address} of the code object's function symbols."""
    return {name: addr for name, addr, _size, _start in _symbols(code, 2)}


def data_symbols(code: bytes) -> list:
    """[(address, size, mangled name)] of the code object's data symbols (device globals)."""
    return sorted((addr, size, name) for name, addr, size, _start in _symbols(code, 1))   # STT_OBJECT


def position_independent(body: bytes, addr: int, data) -> tuple:
    """(form, refs) of a function's bytes `body` loaded at `addr`: refs = [(offset in body of the literal,
    data symbol, offset in the symbol)] for every pc-relative literal whose target lies outside the function
    and inside one of the data symbols `data` (data_symbols), and form = the bytes with those literals
    zeroed, followed by one record per ref.  Without refs form is body itself.

    The compiler forms such an address as  s_getpc_b64 s[N:N+1];  s_add_u32 sN, sN, <literal>;
    s_addc_u32 sN+1, sN+1, <0 or literal>:  pc is the address behind s_getpc_b64.  The same sequence
    starts a long branch, whose target lies inside the function: those literals stay as they are, and
    so does one that resolves to no named data symbol."""
    refs, zero = [], []
    words = struct.unpack_from("<%dI" % (len(body) // 4), body) + (0,)
    for i in range(0, len(body) - 11, 4):
        w0 = words[i // 4]
        if (w0 & 0xFF80FFFF) != 0xBE801C00:                        # s_getpc_b64 sN
            continue
        w1, lo, w3 = words[i // 4 + 1:i // 4 + 4]
        n = (w0 >> 16) & 0x7F
        if w1 != (0x8000FF00 | (n << 16) | n):                     # s_add_u32 sN, sN, literal
            continue
        off, hi_at = lo, None
        if w3 == (0x8200FF00 | ((n + 1) << 16) | (n + 1)) and i + 20 <= len(body):   # s_addc_u32 sN+1, sN+1, literal
            hi_at = i + 16
            off |= struct.unpack_from("<I", body, hi_at)[0] << 32
        elif lo & 0x80000000 and w3 == (0x8200C100 | ((n + 1) << 16) | (n + 1)):     # ... sN+1, sN+1, -1
            off |= 0xFFFFFFFF << 32
        target = (addr + i + 4 + off) & 0xFFFFFFFFFFFFFFFF
        if addr <= target < addr + len(body):
            continue
        for a, size, name in data:
            if a <= target < a + size:
                refs.append((i + 8, name, target - a))
                zero.append(i + 8)
                if hi_at is not None:
                    zero.append(hi_at)
                break
    if not refs:
        return body, refs
    form = bytearray(body)
    for z in zero:
        form[z:z + 4] = b"\0\0\0\0"
    for at, name, k in refs:
        form += struct.pack("<II", at, k) + name.encode() + b"\0"
    return bytes(form), refs


def code_sha(form: bytes) -> str:
    return hashlib.sha256(form).hexdigest()[:16]


def library_kernels(lib_path: str) -> dict:
    """{mangled name: [(raw bytes, position-independent form, refs), one per code object that holds the
    symbol]} over every gfx950 code object of the library.  A sound build has one entry per name."""
    out = {}
    for code in gfx950_code_objects(lib_path):
        data = data_symbols(code)
        for name, addr, size, start in _symbols(code, 2):
            body = code[start:start + size]
            out.setdefault(name, []).append((body,) + position_independent(body, addr, data))
    return out


def march_step_symbol(args: str, batched: bool = False) -> str:
    """The mangled name of k_march<MarchStep<args>> (k_march_b with batched), args as in the profile
    summaries: 'true, false, true, false, false, true, false' (with an eighth, NV: k_march<MarchStepT<args>>)."""
    bits = "".join("Lb1E" if a.strip() == "true" else "Lb0E" for a in args.split(","))
    # (eight arguments: MarchStepT, the body template itself -- the inviscid bodies, its last argument)
    body = "10MarchStepT" if len(args.split(",")) == 8 else "9MarchStep"
    if batched:
        return f"_ZN3ocn9k_march_bINS_{body}I{bits}EEEEvNS_10MarchGridBENS_4PackIT_EE"
    return f"_ZN3ocn7k_marchINS_{body}I{bits}EEEEvNS_9MarchGridET_"


def kernel_code_sha(lib_path: str, symbol: str) -> str | None:
    """sha256 (16 hex digits) of the kernel's machine code in the library, in its position-independent
    form, or None if absent.  The symbol is looked up over every gfx950 code object of the library."""
    for code in gfx950_code_objects(lib_path):
        for name, addr, size, start in _symbols(code, 2):
            if name == symbol:
                return code_sha(position_independent(code[start:start + size], addr, data_symbols(code))[0])
    return None


def sha_by_demangled(lib_path: str, names) -> dict:
    """{demangled kernel name (as rocprofv3 reports it): (mangled symbol, code sha)} for the names found
    in the library (c++filt demangles the code objects' symbols; whitespace-insensitive match)."""
    import subprocess
    syms = {m: v[0][1] for m, v in library_kernels(lib_path).items()}
    mangled = sorted(syms)
    dem = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.split("\n")
    key = {"".join(d.split()): m for m, d in zip(mangled, dem)}
    out = {}
    for n in names:
        m = key.get("".join(n.split()))
        if m:
            out[n] = (m, code_sha(syms[m]))
    return out

