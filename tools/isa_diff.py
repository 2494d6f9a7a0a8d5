"""Per-kernel ISA diff of a --save-temps build before / after the per-block parameter change.  Kernels of `before` map to the `after`
kernel whose template argument list gained a trailing `false` (Lb0E, the defaulted BP flag).  Normalised: the kernel's own name, label
numbers, comments; with --shift OFF: kernarg offsets (loads, address arithmetic on the kernarg pointer) at or behind OFF move back by 8 (ModelArgs grew by one pointer) and the kernarg size by 8."""
import re, sys, difflib
def funcs(path):
    out, cur, name = {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\S+):\s*(;.*)?$", line)
        if m and cur is None:
            name, cur = m.group(1), []; continue
        if cur is not None:
            if line.startswith(".Lfunc_end"): out[name] = cur; cur = None; continue
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
before, after = sys.argv[1], sys.argv[2]
off = int(sys.argv[4], 16) if len(sys.argv) > 4 and sys.argv[3] == "--shift" else None
b, a = funcs(before), funcs(after)
same = diff = 0
for n, body in sorted(b.items()):
    m = n if n in a else re.sub(r"(k_(?:init|step|move)I(?:L[ib]\d+E)+)(EEv)", r"\1Lb0E\2", n)
    has = "ModelArgs" in n
    x, y = norm(body, n, None), norm(a[m], m, off if has else None)
    if x == y: same += 1
    else:
        diff += 1
        d = [l for l in difflib.unified_diff(x, y, lineterm="", n=0) if not l.startswith(("---", "+++", "@@"))]
        print("DIFF", n, len(d)); print("\n".join(d[:10]))
print(f"pre-existing kernels: {len(b)}; identical: {same}; differing: {diff}; new kernels: {len(a) - len(b)}")
