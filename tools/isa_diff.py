#!/usr/bin/env python3
"""Did the device code change?    python tools/isa_diff.py A B
A and B are two objects from `hipcc -c` or two libhydra_hip.so.  Out of each come the gfx950 code objects
(kernel_table.code_objects), and out of those, by symbol name, every function's bytes from .text and every kernel
descriptor (`<kernel>.kd`, 64 bytes).  A descriptor's code-entry offset is relative to the descriptor itself and moves
whenever anything in front of the kernel changes size: it is compared as "points at its own kernel", the other 56 bytes
as they are.  `__hip_cuid_<hash of the source>` differs with every edit, a comment included, and is no kernel: ignored.
Prints one line per kernel that differs and a summary; exit status 1 on any difference.  No compiler run, no GPU; bytes
are compared, not disassembled: code that merely moved and addresses something outside itself pc-relatively (a .got
slot) shows as different (profiles/xreg_host_refactor.md met that case)."""
import os, shutil, struct, subprocess, sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_table import LLVM, code_objects

STT_OBJECT, STT_FUNC = 1, 2
KD_SIZE, KD_ENTRY = 64, 16          # kernel descriptor: int64 kernel_code_entry_byte_offset at byte 16


def symbols(elf):
    """{name: (type, address, size, bytes)} of the defined FUNC / OBJECT symbols of one ELF64 image."""
    assert elf[:6] == b"\x7fELF\x02\x01", "not a little-endian ELF64 image"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for _, sh_type, _, _, off, size, link, _, _, entsize in secs:
        if sh_type != 2:            # SHT_SYMTAB
            continue
        str_off = secs[link][4]
        for pos in range(off, off + size, entsize):
            st_name, st_info, _, shndx, value, st_size = struct.unpack_from("<IBBHQQ", elf, pos)
            if st_info & 15 not in (STT_OBJECT, STT_FUNC) or shndx == 0 or shndx >= shnum:
                continue
            name = elf[str_off + st_name:elf.index(b"\0", str_off + st_name)].decode()
            _, s_type, _, s_addr, s_off, _, _, _, _, _ = secs[shndx]
            data = b"" if s_type == 8 else elf[s_off + value - s_addr:s_off + value - s_addr + st_size]   # 8: NOBITS
            out[name] = (st_info & 15, value, st_size, data)
    return out


def kernels(path):
    """{symbol: (code bytes, descriptor bytes without the entry offset or None, entry points at the symbol or None)}"""
    out = {}
    for img in code_objects(path):
        syms = symbols(img)
        for name, (kind, addr, _, data) in syms.items():
            if kind != STT_FUNC or name.startswith("__hip_cuid_"):
                continue
            kd, own = None, None
            d = syms.get(name + ".kd")
            if d and d[0] == STT_OBJECT and d[2] == KD_SIZE:
                entry, = struct.unpack_from("<q", d[3], KD_ENTRY)
                kd, own = d[3][:KD_ENTRY] + d[3][KD_ENTRY + 8:], d[1] + entry == addr
            key, n = name, 1
            while key in out:       # the same internal name in two translation units of a library
                n += 1
                key = "%s #%d" % (name, n)
            out[key] = (data, kd, own)
    return out


def demangled(names):
    tool = os.path.join(LLVM, "llvm-cxxfilt")
    if not names or not os.path.exists(tool) and not shutil.which("c++filt"):
        return {n: n for n in names}
    r = subprocess.run([tool if os.path.exists(tool) else "c++filt"], input="\n".join(names), capture_output=True, text=True)
    lines = r.stdout.splitlines()
    return dict(zip(names, lines)) if len(lines) == len(names) else {n: n for n in names}


def compare(path_a, path_b, out=sys.stdout):
    a, b = kernels(path_a), kernels(path_b)
    lines = []
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            lines.append((name, "only in " + (path_a if name in a else path_b)))
            continue
        (ca, ka, oa), (cb, kb, ob) = a[name], b[name]
        what = []
        if ca != cb:
            first = next((i for i, (x, y) in enumerate(zip(ca, cb)) if x != y), min(len(ca), len(cb)))
            what.append("code (%d / %d bytes, first difference at +0x%x)" % (len(ca), len(cb), first))
        if ka != kb:
            what.append("descriptor")
        if oa != ob or oa is False:
            what.append("descriptor entry (points at its kernel: %s / %s)" % (oa, ob))
        if what:
            lines.append((name, ", ".join(what)))
    nice = demangled([n.split(" #")[0] for n, _ in lines])
    for name, what in lines:
        print("DIFF %s: %s" % (nice[name.split(" #")[0]], what), file=out)
    both = len(set(a) & set(b))
    n_kd = sum(1 for n in set(a) & set(b) if a[n][1] is not None)
    print("%d / %d symbols, %d in both (%d with a kernel descriptor): %s" %
          (len(a), len(b), both, n_kd, "%d differ" % len(lines) if lines else "code bytes and descriptors identical"), file=out)
    return 1 if lines else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(compare(sys.argv[1], sys.argv[2]))
