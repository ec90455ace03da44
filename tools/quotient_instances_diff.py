"""Compare the quotient_kernel instances of two builds of csrc/quotient.hip from their device assembly:

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S quotient.hip -o {before,after}.s
    python tools/quotient_instances_diff.py before.s after.s

Per instance: registers, scratch and spills from the code object's metadata, and the number of assembly lines that differ once what
only names things is taken out (the kernel's mangled name, the per-file ordinals in local labels, comments).  An instance whose
template argument list grew by a defaulted `false` is matched with its predecessor."""
import difflib
import re
import sys


def kernels(path):
    s = open(path).read()
    body = {m.group(1): m.group(2) for m in re.finditer(r"^(_ZN5gl355\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", s, re.S | re.M)}
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count", s[s.index("amdhsa.kernels:"):])[1:]:
        def g(k):
            return int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
        meta[re.search(r"\.name:\s+(\S+)", blk).group(1)] = dict(
            vgpr=g("vgpr_count"), sgpr=g("sgpr_count"), scratch=g("private_segment_fixed_size"), lds=g("group_segment_fixed_size"),
            sgpr_spill=g("sgpr_spill_count"), vgpr_spill=g("vgpr_spill_count"))
    return body, meta


def norm(text):
    text = re.sub(r"_ZN5gl35515quotient_kernelILi(\d)E(?:Lb[01]E)+EEvNS_8QuotArgsE", r"quotient_kernel_\1", text)
    text = re.sub(r"\.LBB\d+_", ".LBB_", text)
    text = re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", text)
    text = re.sub(r"\s*;.*", "", text)
    return [l for l in text.splitlines() if l.strip()]


def short(name):
    m = re.match(r"_ZN5gl35515quotient_kernelILi(\d)E((?:Lb[01]E)+)EEvNS_8QuotArgsE", name)
    if not m:
        return name
    return "quotient_kernel<%s%s>" % (m.group(1), "".join(", %s" % ("true" if f == "1" else "false") for f in re.findall(r"Lb([01])E", m.group(2))))


def waves(vgpr):
    return min(8, 512 // ((vgpr + 7) // 8 * 8))


def main(before, after):
    bk, bm = kernels(before)
    ak, am = kernels(after)
    for name in sorted(ak):
        old = name if name in bk else name.replace("Lb0ELb0EEEv", "Lb0EEEv")
        m = am[name]
        line = "%-36s vgpr %3d sgpr %3d scratch %3d B spills v %d s %d  waves/SIMD %d" % (short(name), m["vgpr"], m["sgpr"], m["scratch"], m["vgpr_spill"],
                                                                                      m["sgpr_spill"], waves(m["vgpr"]))
        if old in bk:
            a, b = norm(bk[old]), norm(ak[name])
            d = [l for l in difflib.unified_diff(a, b, lineterm="", n=0) if not l.startswith(("---", "+++", "@@"))]
            line += " | before (%s): metadata %s, %d instructions/labels, %d differ" % (short(old), "equal" if bm[old] == m else "DIFFERENT %r" % bm[old], len(b), len(d))
        else:
            line += " | new instance, %d instructions/labels" % len(norm(ak[name]))
        print(line)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
