#!/bin/bash
# Code generation of two builds of the library, side by side (kernel_regs.sh shows one): for EVERY kernel the registers, scratch,
# LDS and spill counts of both; for the kernels whose names contain one of the patterns, the disassembly -- "identical", or
# whether the ordered sequence of vector-memory instructions (LDS-DMA included), LDS reads and writes, MFMAs, s_waitcnt (with
# its counts) and s_barrier is the same and how many other lines differ. Markdown tables on stdout; exit status 1 if a
# resource differs or such a sequence does.
#   bash tools/debug/kernel_diff.sh PARENT/libpet_hip.so metatrain_amd/lib/libpet_hip.so k_emlp_s k_rowgemm_s ...
A=$1; B=$2; shift 2
LLVM=/opt/rocm/lib/llvm/bin
TMP=$(mktemp -d)
for side in a b; do
    lib=$A; [ $side = b ] && lib=$B
    mkdir -p $TMP/$side
    objcopy -O binary --only-section=.hip_fatbin $lib $TMP/$side/fat.bin
    python3 - $TMP/$side/fat.bin $TMP/$side <<'PY'
import sys
data = open(sys.argv[1], 'rb').read(); out = sys.argv[2]
magic = b"__CLANG_OFFLOAD_BUNDLE__"  # split concatenated clang offload bundles
idx = []; i = data.find(magic)
while i >= 0: idx.append(i); i = data.find(magic, i + 1)
idx.append(len(data))
for n, (a, b) in enumerate(zip(idx[:-1], idx[1:])): open(f"{out}/b{n:03d}.bin", "wb").write(data[a:b])
PY
    for f in $TMP/$side/b*.bin; do
        $LLVM/clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$f --output=$f.co --unbundle 2>/dev/null || continue
        $LLVM/llvm-readelf --notes $f.co >> $TMP/$side/notes.txt
        [ $# -gt 0 ] && $LLVM/llvm-objdump -d --no-show-raw-insn --no-leading-addr $f.co >> $TMP/$side/asm.txt
    done
done
python3 - $TMP "$@" <<'PY'
import difflib, os, re, sys
tmp, pats = sys.argv[1], sys.argv[2:]
INTERN = re.compile(r"\.intern\.[0-9a-f]+")
KEYS = ["vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"]

def resources(side):
    out = {}
    for blk in open(f"{tmp}/{side}/notes.txt").read().split("- .agpr_count:")[1:]:
        blk = ".agpr_count:" + blk
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name:  # (kernels of anonymous namespaces carry a per-build hash; one name may come from several code objects)
            out.setdefault(INTERN.sub("", name.group(1)), []).append(tuple((re.search(rf"\.{k}:\s+(\d+)", blk) or [None, "?"])[1] for k in KEYS))
    return {k: sorted(v) for k, v in out.items()}

def listing(side):
    out, cur = {}, None
    if not os.path.exists(f"{tmp}/{side}/asm.txt"): return out
    for line in open(f"{tmp}/{side}/asm.txt"):
        m = re.match(r"^<(\S+)>:", line) or re.match(r"^\S* ?<(\S+)>:", line)
        if m: cur = out.setdefault(INTERN.sub("", m.group(1)), []); continue
        ins = line.split("//")[0].strip()
        if cur is not None and ins: cur.append(re.sub(r"\s+", " ", ins))
    return out

ORDERED = re.compile(r"^(global_|buffer_|flat_|scratch_|ds_|v_mfma|v_smfmac|s_waitcnt|s_barrier)")
def ordered(ins):  # the mnemonic; a wait with its counts
    return [i if i.startswith("s_waitcnt") else i.split(" ")[0] for i in ins if ORDERED.match(i)]

ra, rb = resources("a"), resources("b")
bad = 0
print(f"kernels: {len(ra)} / {len(rb)}; only in one build: {sorted(set(ra) ^ set(rb))}")
bad += len(set(ra) ^ set(rb))
changed = [k for k in sorted(set(ra) & set(rb)) if ra[k] != rb[k]]
print(f"kernels whose resources differ: {len(changed)}")
for k in changed: print("  ", k, ra[k], "->", rb[k])
bad += len(changed)
if pats:
    la, lb = listing("a"), listing("b")
    print("\n| kernel | VGPR | AGPR | SGPR | scratch | LDS | spills | code |\n|---|---|---|---|---|---|---|---|")
    for k in sorted(set(ra) & set(rb)):
        if not any(p in k for p in pats): continue
        a, b = la.get(k, []), lb.get(k, [])
        if a == b: code = f"identical ({len(a)} lines)"
        elif ordered(a) == ordered(b):
            n = sum(1 for d in difflib.ndiff(a, b) if d[:1] == "+")
            code = f"same memory/MFMA/wait sequence ({len(ordered(a))}), {n} of {len(b)} lines differ"
        else:
            code = "SEQUENCE DIFFERS"; bad += 1
            for d in list(difflib.unified_diff(ordered(a), ordered(b), lineterm="", n=2))[:40]: print("    ", d, file=sys.stderr)
        cell = lambda i: ra[k][0][i] if ra[k][0][i] == rb[k][0][i] else f"{ra[k][0][i]} -> {rb[k][0][i]}"
        sp = cell(5) + " / " + cell(6)
        print(f"| `{k}` | {cell(0)} | {cell(1)} | {cell(2)} | {cell(3)} | {cell(4)} | {sp} | {code} |")
sys.exit(1 if bad else 0)
PY
rc=$?
rm -rf $TMP
exit $rc
