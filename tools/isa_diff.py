#!/usr/bin/env python3
"""Did the device code change?    python tools/isa_diff.py A B
A and B are two objects from `hipcc -c` or two libhydra_hip.so.  Out of each come the gfx950 code objects
(kernel_table.code_objects), and out of those, by symbol name, every function's bytes from .text and every kernel
descriptor (`<kernel>.kd`, 64 bytes).  A descriptor's code-entry offset is relative to the descriptor itself and moves
whenever anything in front of the kernel changes size: it is compared as "points at its own kernel", the other 56 bytes
as they are.  `__hip_cuid_<hash of the source>` differs with every edit, a comment included, and is no kernel: ignored.
Prints one line per kernel that differs and a summary; exit status 1 on any DIFF.  No compiler run, no GPU; bytes are
compared, not disassembled.  A function that merely moved (another function changed size or place, and with it this one's
distance to the .got) and forms the address of a .got slot pc-relatively carries another 32-bit displacement: two
versions of EQUAL length that differ only in aligned 32-bit words are MOVED, not DIFF, when every such word names the
same place relative to the image's .got in both (literal + function address - .got address; the offset of the s_getpc
cancels) and the .got slots carry the same relocation symbols in the same order.  MOVED is counted on its own and does
not fail the comparison."""
import os, shutil, struct, subprocess, sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_table import LLVM, code_objects

STT_OBJECT, STT_FUNC = 1, 2
KD_SIZE, KD_ENTRY = 64, 16          # kernel descriptor: int64 kernel_code_entry_byte_offset at byte 16


def sections(elf):
    """The section headers of one ELF64 image: (name offset, type, flags, address, offset, size, link, info, align, entsize)."""
    assert elf[:6] == b"\x7fELF\x02\x01", "not a little-endian ELF64 image"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    return [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]


def cstr(elf, pos):
    return elf[pos:elf.index(b"\0", pos)].decode()


def symbols(elf):
    """{name: (type, address, size, bytes)} of the defined FUNC / OBJECT symbols of one ELF64 image."""
    secs = sections(elf)
    shnum = len(secs)
    out = {}
    for _, sh_type, _, _, off, size, link, _, _, entsize in secs:
        if sh_type != 2:            # SHT_SYMTAB
            continue
        str_off = secs[link][4]
        for pos in range(off, off + size, entsize):
            st_name, st_info, _, shndx, value, st_size = struct.unpack_from("<IBBHQQ", elf, pos)
            if st_info & 15 not in (STT_OBJECT, STT_FUNC) or shndx == 0 or shndx >= shnum:
                continue
            name = cstr(elf, str_off + st_name)
            _, s_type, _, s_addr, s_off, _, _, _, _, _ = secs[shndx]
            data = b"" if s_type == 8 else elf[s_off + value - s_addr:s_off + value - s_addr + st_size]   # 8: NOBITS
            out[name] = (st_info & 15, value, st_size, data)
    return out


def got(elf):
    """(address of .got, [(slot offset, relocation type, symbol, addend)] in slot order) of one image, or None without a .got."""
    secs = sections(elf)
    shstr = secs[struct.unpack_from("<H", elf, 0x3E)[0]][4]
    at = next(((s[3], s[5]) for s in secs if cstr(elf, shstr + s[0]) == ".got"), None)
    if at is None:
        return None
    slots = []
    for _, sh_type, _, _, off, size, link, _, _, entsize in secs:
        if sh_type != 4:            # SHT_RELA
            continue
        sym_off, sym_ent, str_off = secs[link][4], secs[link][9], secs[secs[link][6]][4]
        for pos in range(off, off + size, entsize):
            r_offset, r_info, r_addend = struct.unpack_from("<QQq", elf, pos)
            if at[0] <= r_offset < at[0] + at[1]:
                st_name, = struct.unpack_from("<I", elf, sym_off + (r_info >> 32) * sym_ent)
                slots.append((r_offset - at[0], r_info & 0xffffffff, cstr(elf, str_off + st_name), r_addend))
    return at[0], sorted(slots)


def moved(code_a, where_a, code_b, where_b):
    """Equal length, only aligned 32-bit words differ, and each of those is a displacement to the same place of the same .got."""
    (addr_a, got_a), (addr_b, got_b) = where_a, where_b
    if len(code_a) != len(code_b) or len(code_a) % 4 or got_a is None or got_b is None or got_a[1] != got_b[1]:
        return False
    for o in range(0, len(code_a), 4):
        if code_a[o:o + 4] != code_b[o:o + 4]:
            (la,), (lb,) = struct.unpack_from("<I", code_a, o), struct.unpack_from("<I", code_b, o)
            if (la + addr_a - got_a[0] - (lb + addr_b - got_b[0])) & 0xffffffff:
                return False
    return True


def kernels(path):
    """{symbol: (code bytes, descriptor bytes without the entry offset or None, entry points at the symbol or None,
    (address, .got of its image))}"""
    out = {}
    for img in code_objects(path):
        syms = symbols(img)
        img_got = got(img)
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
            out[key] = (data, kd, own, (addr, img_got))
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
    lines = []                      # (symbol, "DIFF" | "MOVED", what): one line per symbol that is not identical
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            lines.append((name, "DIFF", "only in " + (path_a if name in a else path_b)))
            continue
        (ca, ka, oa, wa), (cb, kb, ob, wb) = a[name], b[name]
        what = []
        code_moved = ca != cb and moved(ca, wa, cb, wb)
        if ca != cb and not code_moved:
            first = next((i for i, (x, y) in enumerate(zip(ca, cb)) if x != y), min(len(ca), len(cb)))
            what.append("code (%d / %d bytes, first difference at +0x%x)" % (len(ca), len(cb), first))
        if ka != kb:
            what.append("descriptor")
        if oa != ob or oa is False:
            what.append("descriptor entry (points at its kernel: %s / %s)" % (oa, ob))
        if what:
            lines.append((name, "DIFF", ", ".join(what)))
        elif code_moved:
            lines.append((name, "MOVED", "same .got target (%d bytes, at 0x%x / 0x%x)" % (len(ca), wa[0], wb[0])))
    nice = demangled([n.split(" #")[0] for n, _, _ in lines])
    for name, tag, what in lines:
        print("%s %s: %s" % (tag, nice[name.split(" #")[0]], what), file=out)
    both = len(set(a) & set(b))
    n_kd = sum(1 for n in set(a) & set(b) if a[n][1] is not None)
    n_moved = sum(1 for _, tag, _ in lines if tag == "MOVED")
    n_diff = len(lines) - n_moved
    if n_moved:
        verdict = "%d identical, %d moved (same .got target), %d differ" % (len(set(a) | set(b)) - len(lines), n_moved, n_diff)
    else:
        verdict = "%d differ" % n_diff if n_diff else "code bytes and descriptors identical"
    print("%d / %d symbols, %d in both (%d with a kernel descriptor): %s" % (len(a), len(b), both, n_kd, verdict), file=out)
    return 1 if n_diff else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(compare(sys.argv[1], sys.argv[2]))
