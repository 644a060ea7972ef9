#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds, kernel by kernel.

    python tools/compare_device_code.py <parent csrc/_obj dir> <branch csrc/_obj dir>

For every *.o of either directory: the .hip_fatbin section is copied out (objcopy), the gfx950 code object unbundled
(clang-offload-bundler) and disassembled (llvm-objdump -d), as tests/test_isa_guards_cpu.py does.  Per kernel symbol the instruction
listing (addresses, encodings, comments and pc-relative distances stripped) and the metadata of its note record (VGPR / AGPR / SGPR counts, scratch and LDS bytes,
kernarg size, workgroup size limit) are compared.  Functions are keyed by (object, symbol); a symbol that exactly one object holds on each side is
matched across objects, compared like any other and counted under "moved" with both object names (LIST_MOVED=1 names each one).  Prints the
kernels only the parent has, only the branch has, and those whose listing or metadata differ; exit status 1 when a kernel was added or
changed (a refactor may remove or move kernels, nothing else).
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
META_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".kernarg_segment_size",
             ".max_flat_workgroup_size", ".vgpr_spill_count", ".sgpr_spill_count", ".wavefront_size", ".uses_dynamic_stack")


def code_object(obj, tmp):
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "gfx950.co")
    subprocess.check_call([shutil.which("objcopy") or "objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
    if not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return None
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat,
                           "--output=" + co, "--unbundle"])
    return co


def listings(co):
    """{function symbol: [instruction text, ...]} of a code object (kernels and device functions alike)."""
    txt = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], capture_output=True, text=True, check=True).stdout
    out, cur, pc = {}, None, None
    for ln in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
        if m:
            cur, pc = out.setdefault(m.group(1), []), None
            continue
        if cur is None or not ln.startswith((" ", "\t")):
            continue
        ins = ln.split("//")[0].strip()               # llvm-objdump puts address and encoding behind `//`
        ins = re.sub(r"<[^>]+>", "<label>", ins)      # branch targets print as symbol+offset
        if not ins:
            continue
        ins = " ".join(ins.split())
        # pc-relative address of a constant or function: s_getpc_b64 s[a:b]; s_add_u32 sa, sa, <distance>; s_addc_u32 sb, sb, <carry part>.
        # The distance moves with the position of the function in the code object, i.e. whenever another kernel is removed.
        m = re.match(r"s_getpc_b64 (?:s\[(\d+):(\d+)\]|(vcc))$", ins)
        if m:
            pc = ("vcc_lo", "vcc_hi") if m.group(3) else ("s" + m.group(1), "s" + m.group(2))
        elif pc and re.match(r"s_add_u32 %s, %s, (0x[0-9a-f]+|-?\d+)$" % (pc[0], pc[0]), ins):
            ins = "s_add_u32 %s, %s, <pcrel>" % (pc[0], pc[0])
        elif pc and re.match(r"s_addc_u32 %s, %s, (0x[0-9a-f]+|-?\d+)$" % (pc[1], pc[1]), ins):
            ins, pc = "s_addc_u32 %s, %s, <pcrel>" % (pc[1], pc[1]), None
        cur.append(ins)
    # a function ends at s_endpgm / its last branch; the alignment padding behind it depends on what FOLLOWS it in the object, not on the function
    # (KEEP_PADDING=1 compares it too: shows which functions differ in nothing else)
    for body in out.values() if not os.environ.get("KEEP_PADDING") else ():
        while body and body[-1] in ("s_nop 0", "...", "s_code_end"):
            body.pop()
    return out


def metadata(co):
    """{kernel symbol: {key: value}} from the AMDGPU metadata note."""
    txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for ln in txt.splitlines():
        m = re.match(r"^  (- | {2})(\.[a-z_]+):\s*(.*)$", ln)      # the keys of a kernel record, not those of its argument list
        if not m:
            continue
        first, k, v = m.groups()
        if first == "- ":
            cur = {}                                   # a record starts at its first key
        if cur is None:
            continue
        if k == ".symbol":
            out[v[:-3] if v.endswith(".kd") else v] = cur
        elif k in META_KEYS:
            cur[k] = v
    return out


def survey(objdir):
    lst, meta = {}, {}
    for f in sorted(os.listdir(objdir)):
        if not f.endswith(".o"):
            continue
        with tempfile.TemporaryDirectory() as tmp:
            co = code_object(os.path.join(objdir, f), tmp)
            if co is None:
                continue
            for k, v in listings(co).items():
                lst[(f, k)] = v
            for k, v in metadata(co).items():
                meta[(f, k)] = v
    return lst, meta


def demangle(names):
    if not names:
        return {}
    filt = next((c for c in (os.path.join(LLVM, "llvm-cxxfilt"), shutil.which("c++filt")) if c and os.path.exists(c)), None)
    if filt is None:
        return {n: n for n in names}
    r = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, r.stdout.splitlines())) if r.returncode == 0 else {n: n for n in names}


def pairs(parent, branch):
    """{parent key: branch key} for two {(object, symbol): ...} surveys.  The same (object, symbol) on both sides is a pair; a symbol that
    exactly one object holds on each side is a pair across objects (a move); a symbol several objects hold on a side stays keyed per object."""
    holders = [{}, {}]
    for side, keys in enumerate((parent, branch)):
        for f, k in keys:
            holders[side].setdefault(k, []).append(f)
    out = {}
    for f, k in parent:
        if (f, k) in branch:
            out[(f, k)] = (f, k)
        elif len(holders[0][k]) == 1 and len(holders[1].get(k, ())) == 1:
            out[(f, k)] = (holders[1][k][0], k)
    return out


def main(parent_dir, branch_dir):
    pl, pm = survey(parent_dir)
    bl, bm = survey(branch_dir)
    lp, mp = pairs(pl, bl), pairs(pm, bm)
    removed = sorted(set(pl) - set(lp))
    added = sorted(set(bl) - set(lp.values()))
    moved = sorted(k for k in lp if lp[k] != k)
    changed = sorted(k for k in lp if pl[k] != bl[lp[k]])
    meta_changed = sorted(k for k in mp if pm[k] != bm[mp[k]])
    meta_added = sorted(set(bm) - set(mp.values()))
    names = demangle(sorted({k[1] for k in removed + added + changed + meta_changed + moved}))
    print("functions: parent %d, branch %d, identical %d (moved to another object: %d)" % (len(pl), len(bl), len(lp) - len(changed), len(moved)))
    print("kernel metadata records: parent %d, branch %d, identical %d" % (len(pm), len(bm), len(mp) - len(meta_changed)))
    for title, keys in (("removed", removed), ("ADDED", added), ("CHANGED listing", changed), ("CHANGED metadata", meta_changed)):
        print("%s: %d" % (title, len(keys)))
        for f, k in keys:
            to = (lp if title != "CHANGED metadata" else mp).get((f, k), (f, k))[0]
            print("   %-12s %s" % (f if to == f or title == "ADDED" else f + " -> " + to, names.get(k, k)))
    for k in meta_changed:
        print("   metadata of", names.get(k[1], k[1]), {x: (pm[k].get(x), bm[mp[k]].get(x)) for x in META_KEYS if pm[k].get(x) != bm[mp[k]].get(x)})
    print("moved: %d" % len(moved))      # compared like every other pair: a moved function that differs is under CHANGED too
    routes = {}
    for k in moved:
        routes.setdefault((k[0], lp[k][0]), []).append(k)
    for (src, dst), keys in sorted(routes.items()):
        print("   %s -> %s: %d" % (src, dst, len(keys)))
        for k in keys if os.environ.get("LIST_MOVED") else ():
            print("      " + names.get(k[1], k[1]))
    return 1 if (added or changed or meta_changed or meta_added) else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
