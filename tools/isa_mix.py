#!/usr/bin/env python3
"""Static instruction mix of the sketch kernel's per-k-mer hot path: disassembles gs_sketch.hip for gfx950, takes the
interior-word fast loop of k_sketch_min<DNA, LDS table, optdens, 64-bit values, u32 keys> (the span between two consecutive ds_min_u32 of
the unrolled-by-2 loop that carries the fewest 64-bit compares, i.e. no bounds test) and counts instructions per class. Issue cycles per
wave64 instruction: simple VALU 2 (MI355X_MICROARCH.md:52-54); 32-bit integer multiplies / v_mad_u64_u32 weighted by the ratio measured by
tools/ubench_valu (profiles/r02_ubench_valu.txt) when that file is given, else the quarter-rate assumption (x4).
usage: isa_mix.py [ubench_valu.txt] > profiles/r05_sketch_isa_mix.json

--trav [--src TREE]: static census of one phase-1 pop of the dense traversal instead. Compiles gs_index.hip with line tables, takes the headline
instantiation k_hnsw_search_dense<VLDS, !PROF, 6, !ONEG, !WLOG, !SPLIT> and books every instruction of the kernel to the source line of the KERNEL it
was inlined into (the outermost frame of its .loc), lines grouped into the stretches of the pop loop by anchors looked up in the source text. Opcodes
are classified by prefix only. Static: an instruction counts once however often its block runs (the insertion loop of wavefront 0 runs once per key
that enters the front) and both sides of a branch count; the measured figure is the PMC one (tools/pmc_trav.sh)."""
import collections, json, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def trav_census(tree):
    rel = os.path.join("gsearch_amd", "csrc", "gs_index.hip")
    src = os.path.join(tree, rel)
    asm = os.path.join(tempfile.mkdtemp(), "gs_index_g.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-gline-tables-only",
                           "-S", "-o", asm, src], stderr=subprocess.DEVNULL)
    text = open(asm).read()
    a = text.index("\n_ZN2gs19k_hnsw_search_denseILb1ELb0ELi6ELb0ELb0ELb0EEE")
    body = text[a:text.index("s_endpgm", a)].splitlines()
    source = open(src).read().splitlines()
    k0 = next(i for i, l in enumerate(source) if "void k_hnsw_search_dense(" in l)
    # (name, on the headline's path, who runs it, anchor text, line offset): a group runs from its anchor to the next group's
    groups = [("kernel prologue, per-query set-up, descent", False, "-", "void k_hnsw_search_dense(", 0),
              ("loop head: phase test, head keys of the front", True, "all", "if (PHASE2 && dmax == tau && !(cap_log & 1u))", 0),
              ("refill / compaction (pq_rebuild)", False, "-", "if (empty || crowded) {", 0),
              ("pop: front down one lane, publish", True, "all", "if (KCNT(c) > dmax) break;", 0),
              ("!PQ form", False, "-", "if (headG < nG && headG - wbase >= wn) {", 0),
              ("expanding half: row, test-and-set, look-up", True, "expand", "const long long p0 = PROF", 0),
              ("hint half: row, visited hint, look-up", True, "hint", "} else if (!ONEG && c1 != ~(uint64_t)0) {", 0),
              ("ballots, wave sums out, row after next, POP BARRIER", True, "all", "} else if (!ONEG) pk = ~(uint64_t)0;", 0),
              ("sums of the wave words, accept rule (fast)", True, "all", "const long long p2 = PROF", 0),
              ("slow accept (ranks)", False, "-", "// the expansion E in adjacency order", 0),
              ("accepted keys: histogram, compaction into As, BARRIER", True, "all", "const long long p4 = PROF", 0),
              ("wavefront 0: keys into the front / U", True, "wave0", "// wavefront 0 takes the accepted keys 64 at a time", -1),
              ("BARRIER, state back, rows of the new heads", True, "all", "nU = (uint32_t)S.scal[4]; minA = S.scal[5];", -1),
              ("trim of R, fast form", True, "all", "const long long q1 = PROF", 0),
              ("trim of R, histogram walk", False, "-", "// full: wave 0 reads bins other waves have just incremented", 0),
              ("trim tail, T test", True, "all", "dmax = (uint32_t)S.scal[2]; tieT = (uint32_t)S.scal[3];", 2),
              ("T merge", False, "-", "const uint64_t k = S.As[threadIdx.x];", 0),
              ("!PQ rest of the pop", False, "-", "// T <- knbn smallest of T u A (only when A reaches into it)", -1),
              ("after the loop: phase 2, outputs, WLOG sort", False, "-", "const long long tm2 = tm ? clock64() : 0;", 0)]
    starts, at = [], k0
    for g in groups:
        at = next(i for i in range(at, len(source)) if g[3] in source[i]) + g[4]
        starts.append(at + 1)                                  # 1-based like .loc
    def group_of(line):
        j = -1
        for i, s in enumerate(starts):
            if line >= s:
                j = i
        return j
    def klass(op):
        if op.startswith("v_"): return "valu"
        if op.startswith("ds_"): return "lds"
        if op.startswith(("global_", "buffer_", "flat_", "scratch_")): return "vmem"
        if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_call")): return "branch"
        if op.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_sleep")): return "wait"
        if op.startswith(("s_load", "s_buffer_load")): return "smem"
        return "salu" if op.startswith("s_") else "other"
    counts = [collections.Counter() for _ in groups]
    cur = 0
    for l in body:
        s = l.strip()
        if s.startswith(".loc"):
            hits = re.findall(r"gs_index\.hip:(\d+)", s)
            if hits and group_of(int(hits[-1])) >= 0:
                cur = group_of(int(hits[-1]))
            continue
        if not l.startswith("\t") or not s or s.startswith((";", ".")):
            continue
        counts[cur][klass(s.split()[0])] += 1
    cols = ["valu", "salu", "lds", "vmem", "smem", "branch", "wait", "other"]
    print("static census of one phase-1 pop, k_hnsw_search_dense<VLDS, !PROF, 6, !ONEG, !WLOG, !SPLIT>, %s" % rel)
    print("%-58s %-7s %5s  " % ("stretch (source lines)", "runs", "all") + " ".join("%6s" % c for c in cols))
    per_role = collections.Counter()
    for g, s, e, c in zip(groups, starts, starts[1:] + [starts[-1] + 400], counts):
        tot = sum(c.values())
        print("%-58s %-7s %5d  " % ("%s%s (%d-%d)" % ("" if g[1] else "[off path] ", g[0], s, e - 1), g[2], tot) + " ".join("%6d" % c[k] for k in cols))
        if g[1]:
            per_role[g[2]] += tot
    n_all, n_e, n_h, n_0 = per_role["all"], per_role["expand"], per_role["hint"], per_role["wave0"]
    print("on the path, per wave: every wave %d + expanding half %d | hint half %d; wavefront 0 a further %d" % (n_all, n_e, n_h, n_0))
    print("static wave-instructions of one accepting pop over the eight waves: 8 x %d + 4 x %d + 4 x %d + %d = %d" % (n_all, n_e, n_h, n_0, 8 * n_all + 4 * n_e + 4 * n_h + n_0))


if "--trav" in sys.argv:
    trav_census(sys.argv[sys.argv.index("--src") + 1] if "--src" in sys.argv else ROOT)
    sys.exit(0)
src = os.path.join(ROOT, "gsearch_amd", "csrc", "gs_sketch.hip")
asm = os.path.join(tempfile.gettempdir(), "gs_sketch_isa.s")
subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S", "-o", asm, src],
                      stderr=subprocess.DEVNULL)
text = open(asm).read()
a = text.index("_ZN2gs12k_sketch_minILb0ELb1ELi4ELi64EjLb0ELi0EEE")      # <DNA, LDS table, optdens, 64-bit values, u32 keys, unfiltered emitter, canonical compiled in>
body = text[a:text.index("s_endpgm", a)].splitlines()
ins = [l.split()[0] for l in body if l.startswith("\t") and l.strip() and not l.strip().startswith((";", "."))]
mins = [i for i, op in enumerate(ins) if op == "ds_min_u32"]
best = None
for x, y in zip(mins, mins[1:]):
    ops = ins[x + 1:y + 1]
    if len(ops) > 400:
        continue
    n_cmp64 = sum(1 for op in ops if op.startswith("v_cmp_") and "_u64" in op)
    if best is None or (n_cmp64, len(ops)) < (best[0], len(best[1])):
        best = (n_cmp64, ops)
ops = best[1]
# per-opcode issue cycles: measured by tools/ubench_valu when its output is given (cycles at the clock it ran at), else 2 / 8
UB = {}
if len(sys.argv) > 1 and os.path.exists(sys.argv[1]):
    for line in open(sys.argv[1]):
        m = re.match(r"(v_\w+)\s+[0-9.]+ ms\s+->\s+([0-9.]+) ns per wave-instr per SIMD", line)
        if m:
            UB[m.group(1)] = float(m.group(2))
base_ns = UB.get("v_xor_b32")


def cost(op):
    """issue cost of one wave64 instruction in units of a simple VALU op (v_xor_b32 = 1)"""
    o = re.sub(r"_e(32|64)$", "", op)
    if UB and base_ns:
        for k in (o, "v_mul_lo_u32" if o.startswith("v_mul_") else None, "v_cmp_lt_u64" if o.startswith("v_cmp_") and "_u64" in o else None,
                  "v_lshlrev_b64" if o in ("v_lshlrev_b64", "v_ashrrev_i64") else None):
            if k and k in UB:
                return UB[k] / base_ns
        return 1.0
    return 4.0 if o.startswith(("v_mul_lo_u32", "v_mul_hi_u32", "v_mad_u64_u32")) else 1.0


cls, weighted = collections.Counter(), 0.0
for op in ops:
    if op.startswith("v_"):
        key = "valu_mul32" if op.startswith(("v_mul_lo_u32", "v_mul_hi_u32", "v_mad_u64_u32")) else ("valu_64bit" if re.search(r"_[bui]64", op) else "valu_simple")
        cls[key] += 1
        weighted += cost(op)
    elif op.startswith("ds_"):
        cls["lds"] += 1
    elif op.startswith("s_"):
        cls["salu_or_branch"] += 1
    else:
        cls["other"] += 1
valu = cls["valu_mul32"] + cls["valu_simple"] + cls["valu_64bit"]
simple_cycles = 2.0 if not (UB and base_ns) else base_ns * 2.4       # cycles of a simple op: guide value, or measured ns at 2.4 GHz
print(json.dumps({"kernel": "k_sketch_min<DNA, LDS table, optdens, u32 keys>: interior-word loop, one k-mer (one half of the unroll-by-2 body)",
                  "instructions_per_kmer": len(ops), "classes": dict(cls), "valu_per_kmer": valu, "valu_weighted_in_simple_ops": weighted,
                  "cycles_per_simple_valu_op": simple_cycles, "issue_cycles_per_kmer": weighted * simple_cycles,
                  "per_opcode_ns_per_wave_instr_per_simd": UB or None,
                  "model": "issue cycles per wave64 group of 64 k-mers = sum over VALU instructions of their measured issue time (tools/ubench_valu, one op stream per SIMD "
                           "at 8 waves/SIMD) when given, else 2 cycles per simple op and 8 per 32-bit multiply (MI355X_MICROARCH.md:52-54); SALU / branch / LDS issue on other ports"}, indent=1))
