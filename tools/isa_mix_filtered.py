#!/usr/bin/env python3
"""Static VALU count and weighted issue cycles of the per-k-mer fast path of the FILTERED headline sketch kernel,
k_sketch_min<DNA, LDS table, optdens, 64-bit values, u32 keys, filtered emitter, canonical compiled in> (the one bench.py's request step runs).

Cross-compiles gsearch_amd/csrc/gs_sketch.hip (of this tree, or of --src TREE) for gfx950 and takes, in the interior full-wave loop, the path of one
k-mer that is dropped by the filter test: from the loop header of the innermost loop holding the survivor-queue push (v_mbcnt_hi) down to that
push's ballot test (`s_cbranch_vccz`; `s_cbranch_scc1` on the OR of two masks where a pair of k-mers shares a push) in fall-through order (the direct
form is laid out elsewhere). When the loop body holds two k-mers, the span is halved. The push itself is reported as an item of its own (`push`): the
VALU of each push site on the path that does not flush, and their sum per pair of k-mers. Issue cycles per wave64 instruction come from
tools/ubench_valu output (profiles/r02_ubench_valu.txt by default); opcodes it did not measure count as a simple op (v_xor_b32).
usage: isa_mix_filtered.py [--src TREE] [--ubench FILE]"""
import argparse, collections, json, os, re, subprocess, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "_ZN2gs12k_sketch_minILb0ELb1ELi4ELi64EjLb1ELi0EEE"

ap = argparse.ArgumentParser()
ap.add_argument("--src", default=ROOT, help="source tree whose gsearch_amd/csrc/gs_sketch.hip is compiled")
ap.add_argument("--ubench", default=os.path.join(ROOT, "profiles", "r02_ubench_valu.txt"))
ap.add_argument("--asm", default=None, help="device assembly of gs_sketch.hip that is already there (tools/kregs.sh with KEEP_ASM): nothing is compiled")
args = ap.parse_args()

src = os.path.join(args.src, "gsearch_amd", "csrc", "gs_sketch.hip")
asm = args.asm or os.path.join(tempfile.mkdtemp(), "gs_sketch.s")
if not args.asm:
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S", "-o", asm, src])
text = open(asm).read()
a = text.index(KERNEL + "vPKhPKmS4_S4_S4_S4_jjmPT3_f:")
lines = text[a:text.index("s_endpgm", a)].splitlines()

UB = {}
for line in open(args.ubench):
    m = re.match(r"(v_\w+)\s+[0-9.]+ ms\s+->\s+([0-9.]+) ns per wave-instr per SIMD\s+\(= ([0-9.]+) cycles", line)
    if m:
        UB[m.group(1)] = float(m.group(3))


def cycles(op):
    o = re.sub(r"_e(32|64)$", "", op)
    for k in (o, "v_mul_lo_u32" if o.startswith("v_mul_") else None, "v_cmp_lt_u64" if o.startswith("v_cmp_") and "_u64" in o else None):
        if k and k in UB:
            return UB[k]
    return UB["v_xor_b32"]


def op_of(l):
    s = l.strip()
    return None if (not l.startswith("\t") or not s or s.startswith((";", "."))) else s.split()[0]


# the innermost loop header in front of a survivor-queue push, for the interior loop at k > 16 (the bench's k = 21)
push = [i for i, l in enumerate(lines) if op_of(l) == "v_mbcnt_hi_u32_b32"]
best = None
for p in push:
    hs = [i for i in range(p) if lines[i].startswith(".LBB") and "This Loop Header" in "".join(lines[i:i + 6])]
    if not hs:
        continue
    h = hs[-1]
    body = [op_of(l) for l in lines[h:p]]
    if any(o == "ds_min_u32" for o in body[:40]) or not any(o and o.startswith("v_cmp_lt_u64") for o in body):
        continue                                                   # not the interior loop, or the k <= 16 form (32-bit canonical minimum)
    if best is None or p - h < best[1] - best[0]:
        best = (h, p)
h, p = best
ops = [o for o in map(op_of, lines[h:p]) if o]                    # fall-through order: the direct form is laid out after the loop
# the ballot test of the push and everything before it; the push block itself (taken when any lane passes) is counted apart, below.
# One k-mer per push: the test is `s_cbranch_vccz` on the compare's mask; a pair per push: `s_cbranch_scc1` on the OR of the two masks.
cut = max(j for j, o in enumerate(ops) if o in ("s_cbranch_vccz", "s_cbranch_scc1"))
ops = ops[:cut + 1]
per = max(1, sum(1 for o in ops if o.startswith("v_cmp_lt_u64")))  # one canonical-minimum compare per k-mer of the body
valu = [o for o in ops if o.startswith("v_")]
cls = collections.Counter(o for o in valu)
weighted = sum(cycles(o) for o in valu)

# The push, as its own item: for every v_mbcnt_hi of the loop (one per push site), the VALU from the branch in front of it to its first queue
# write (the path that does not flush, laid out first) and on to the next branch (the fill-count bookkeeping, where it is VALU work).
label = lines[h].split(":")[0]
last = max(i for i in range(h, len(lines)) if re.search(r"(Header=|Parent Loop )%s\b" % label[2:], lines[i]))          # the loop's last block starts here
back = next((i for i in range(last + 1, len(lines)) if lines[i].startswith(".LBB")), len(lines) - 1)
sites = []
for q in [i for i in range(h, back) if op_of(lines[i]) == "v_mbcnt_hi_u32_b32"]:
    a = max(i for i in range(h, q) if (op_of(lines[i]) or "").startswith("s_cbranch"))
    w = next(i for i in range(q, back) if (op_of(lines[i]) or "").startswith("ds_write_b"))
    e = next(i for i in range(w, back + 1) if (op_of(lines[i]) or "").startswith(("s_cbranch", "s_branch")))
    sites.append([o for o in map(op_of, lines[a + 1:e]) if o and o.startswith("v_")])
first = sites[0]
pair = ops[-1] == "s_cbranch_scc1"
push = {"kmers_per_first_push": 2 if pair else 1, "push_sites_in_loop_body": len(sites),
        "valu_first_push": len(first), "issue_cycles_first_push": sum(cycles(o) for o in first), "opcodes_first_push": dict(collections.Counter(first))}
if pair:
    # the second site is the push of the lanes where BOTH k-mers survive, behind a wave-uniform branch: ~a quarter of the pairs at 7 % survivors
    push.update({"valu_second_push": len(sites[1]), "opcodes_second_push": dict(collections.Counter(sites[1])),
                 "valu_per_pair": len(first) + 0.25 * len(sites[1])})
else:
    push["valu_per_pair"] = 2 * len(first)
print(json.dumps({"kernel": "k_sketch_min<DNA, LDS table, optdens, u32 keys, filtered, canonical>: interior full-wave loop, one k-mer dropped by the filter test",
                  "source": os.path.relpath(src, args.src) if args.src == ROOT else src,
                  "valu_per_kmer": len(valu) / per, "issue_cycles_per_kmer": weighted / per, "salu_and_other_per_kmer": (len(ops) - len(valu)) / per,
                  "opcodes": {k: v / per for k, v in sorted(cls.items())},
                  "push": push,
                  "model": "issue cycles of one wave64 instruction as measured by tools/ubench_valu (8 waves/SIMD); the queue push (taken by ~98 % of "
                           "the k-mers, ~100 % of the pairs, for 64 lanes at ~7 % survivors) is the item `push`, on the path that does not flush; "
                           "the flush of 64 survivors and the bound refresh are not in this count"}, indent=1))
