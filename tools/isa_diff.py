#!/usr/bin/env python3
"""Compare the device assembly of two -save-temps builds instruction for instruction (comments, .file / .ident / .loc lines stripped:
label comments carry the mangled names of inlined functions, which change with any template signature; the __hip_cuid_<hash> symbol
is a hash of the unit's path, which differs between two checkouts).
   python tools/isa_diff.py <dir_before> [<dir_after> = quantumattention_amd/_build_temps] [--mix]
Used in round 6 to show that taking the QATTN_DEV scaffolding out of the product sources left every kernel's ISA unchanged.
--mix: for every unit that DIFFERS, compare kernel by kernel (same mangled name) the count of every opcode -- except the moves, compares
and branches a refactor shuffles: v_mov* s_mov* v_accvgpr_* s_cmp* s_cbranch* s_branch -- the scratch size and the occupancy tier
(waves per SIMD that vgpr + agpr allow).  A kernel line ends SAME-MIX or names what moved; exit status 1 if any kernel's did."""
import collections, glob, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = [a for a in sys.argv[1:] if not a.startswith("--")]
mix = "--mix" in sys.argv
before = args[0]
after = args[1] if len(args) > 1 else os.path.join(ROOT, "quantumattention_amd", "_build_temps")
FREE = re.compile(r"v_mov|s_mov|v_accvgpr_|s_cmp|s_cbranch|s_branch$")


def norm(path):
    out = []
    for line in open(path, errors="replace"):
        line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", re.sub(r";.*$", "", line)).rstrip()
        if line.strip() and not re.search(r"\.file|\.ident|\.loc\b", line):
            out.append(line)
    return out


def kernels(lines):
    """{mangled name: (opcode histogram, scratch bytes, vgpr + agpr)} of the unit's kernels"""
    hist, meta, cur = {}, {}, None
    for line in lines:
        w = line.split()
        if re.match(r"^_Z\w+:$", line):
            cur = hist.setdefault(line[:-1], collections.Counter())
        elif w[0] == ".amdhsa_kernel":
            cur = meta.setdefault(w[1], {})
        elif w[0] == ".end_amdhsa_kernel" or w[0].startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and (line[0] == "\t" and w[0][0] != "." or w[0].startswith(".amdhsa_")):
            if w[0].startswith(".amdhsa_"):
                cur[w[0]] = w[1]
            else:
                cur[w[0]] += 1
    return {k: (hist[k], int(m[".amdhsa_private_segment_fixed_size"]), int(m[".amdhsa_next_free_vgpr"])) for k, m in meta.items()}


def tier(regs):
    return min(8, 512 // ((regs + 7) // 8 * 8))


bad = 0
for f in sorted(glob.glob(os.path.join(after, "*gfx950.s"))):
    g = os.path.join(before, os.path.basename(f))
    if not os.path.exists(g):
        print(f"{os.path.basename(f):60s} (no counterpart)")
        continue
    a, b = norm(f), norm(g)
    same = a == b
    n_mfma = sum("v_mfma" in x for x in a)
    print(f"{os.path.basename(f):60s} {'IDENTICAL' if same else 'DIFFERS  '}  {len(a)} lines, {n_mfma} v_mfma")
    if same or not mix:
        bad += not same
        continue
    ka, kb = kernels(a), kernels(b)
    for k in sorted(set(ka) | set(kb)):
        if k not in ka or k not in kb:
            print(f"    {k}: only {'after' if k in ka else 'before'}")
            bad += 1
            continue
        (ha, sa, ra), (hb, sb, rb) = ka[k], kb[k]
        moved = [f"{op} {hb[op]}->{ha[op]}" for op in sorted(set(ha) | set(hb)) if ha[op] != hb[op] and not FREE.match(op)]
        if sa or sb:
            moved.append(f"scratch {sb}->{sa}")
        if tier(ra) < tier(rb):
            moved.append(f"occupancy tier {tier(rb)}->{tier(ra)}")
        bad += bool(moved)
        print(f"    {k}: regs {rb}->{ra} (tier {tier(ra)}), {sum(ha.values())} instructions  {'SAME-MIX' if not moved else 'MOVED: ' + ', '.join(moved)}")
sys.exit(1 if bad else 0)
