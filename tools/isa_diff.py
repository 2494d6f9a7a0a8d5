"""Per-kernel ISA diff of two --save-temps builds: the check that a change leaves the kernels' code alone.

    python tools/isa_diff.py BEFORE AFTER [--shift OFF]

BEFORE / AFTER: the device assembly of one build each -- a .s file, or several separated by commas (the units' *-hip-amdgcn-amd-amdhsa-gfx950.s:
a kernel may change translation unit).  Normalised: the kernel's own name, label numbers, comments.  Reports every kernel that differs, every
kernel of BEFORE missing from AFTER and every kernel new in AFTER, and exits non-zero if there is any.

--shift OFF compares against the parent of the per-block parameter change: kernels of BEFORE map to the AFTER kernel whose template argument list
gained a trailing `false` (Lb0E, the defaulted BP flag), and in kernels that take ModelArgs the kernarg offsets (loads, address arithmetic on the
kernarg pointer) at or behind OFF move back by 8 (ModelArgs grew by one pointer) and the kernarg size by 8."""
import difflib
import re
import sys


def funcs(paths):
    out = {}
    for path in paths.split(","):
        cur, name = None, None
        for line in open(path):
            m = re.match(r"^(_Z\S+):\s*(;.*)?$", line)
            if m and cur is None:
                name, cur = m.group(1), []; continue
            if cur is not None:
                if line.startswith(".Lfunc_end"): out.setdefault(name, cur); cur = None; continue
                cur.append(line)
    return out


def norm(lines, name, off):
    t = []
    for l in lines:
        l = l.replace(name, "FN")
        l = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", l); l = re.sub(r"\.Ltmp\d+", ".Ltmp", l); l = re.sub(r"\.Lfunc_begin\d+", ".Lfunc_begin", l)
        l = re.sub(r";.*$", "", l).rstrip()
        if off is not None:
            l = re.sub(r"(s_load_dword\S*\s+s\[?[\d:]+\]?, s\[\d+:\d+\], )0x([0-9a-f]+)", lambda m: m.group(1) + hex(int(m.group(2), 16) - (8 if off <= int(m.group(2), 16) < 0x400 else 0)), l)
            l = re.sub(r"(s_add_u32 s\d+, s0, )0x([0-9a-f]+)$", lambda m: m.group(1) + hex(int(m.group(2), 16) - (8 if off <= int(m.group(2), 16) < 0x400 else 0)), l)
            l = re.sub(r"(\.amdhsa_kernarg_size )(\d+)", lambda m: m.group(1) + str(int(m.group(2)) - 8), l)
        if l: t.append(l)
    return t


def main(argv):
    if len(argv) not in (2, 4) or (len(argv) == 4 and argv[2] != "--shift"):
        sys.exit(__doc__)
    off = int(argv[3], 16) if len(argv) == 4 else None
    b, a = funcs(argv[0]), funcs(argv[1])
    same = diff = 0
    missing, matched = [], set()
    for n, body in sorted(b.items()):
        m = n
        if m not in a and off is not None:
            m = re.sub(r"(k_(?:init|step|move)I(?:L[ib]\d+E)+)(EEv)", r"\1Lb0E\2", n)
        if m not in a:
            missing.append(n); continue
        matched.add(m)
        x, y = norm(body, n, None), norm(a[m], m, off if off is not None and "ModelArgs" in n else None)
        if x == y: same += 1
        else:
            diff += 1
            d = [l for l in difflib.unified_diff(x, y, lineterm="", n=0) if not l.startswith(("---", "+++", "@@"))]
            print("DIFF", n, len(d)); print("\n".join(d[:10]))
    new = sorted(set(a) - matched)
    for n in missing: print("MISSING", n)
    for n in new: print("NEW", n)
    print(f"kernels before: {len(b)}; after: {len(a)}; identical: {same}; differing: {diff}; missing: {len(missing)}; new kernels: {len(new)}")
    return 1 if diff or missing or new else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
