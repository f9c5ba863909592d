"""Code-generation comparison of two builds of gcr_preprocess.hip (no GPU needed), as profiles/k1_refactor_codegen.txt has it.
Each build: the Makefile's flags for gcr_preprocess.o plus `--cuda-device-only -S -Rpass-analysis=kernel-resource-usage`,
assembly to NAME.s and the remarks (stderr) to NAME.remarks.
    python tools/k1_codegen.py DIR/parent DIR/branch > profiles/k1_refactor_codegen.txt
Per kernel: VGPRs, AGPRs, SGPRs, LDS, scratch, waves/SIMD, instructions; whether the instruction stream is the parent's (labels,
symbol names and directives stripped); for the kernels that differ, the mnemonic histogram of the difference per part of the
kernel (from the natural loops of its control flow), and the loads, stores, vmcnt waits and barriers of its streaming loop.

Any other translation unit (profiles/gcs_unify_codegen.txt: gcs_sparse.hip with the Makefile's flags for gcs_sparse.o):
    python tools/k1_codegen.py --loops DIR/parent DIR/branch ["parent kernel=branch kernel" ...]
`--loops` cuts a kernel into prologue / loops (every natural loop) / epilogue instead of K1's stream and pass, and prints for a
kernel that differs whether its loops keep the parent's MFMA, LDS, global-memory, barrier and `s_waitcnt vmcnt` instructions.
The trailing arguments pair a renamed kernel of the parent with the branch's.  c++filt does not know `_Float16` (DF16_), so it
is demangled as the equally builtin `half` (Dh), which leaves the substitutions of the mangled name as they are."""
import collections, re, subprocess, sys


def demangle(fn):
    d = subprocess.run(["c++filt", fn.replace("DF16_", "Dh")], capture_output=True, text=True).stdout.strip()
    return re.sub(r"\(anonymous namespace\)::|\(.*", "", d).replace("void ", "")


def load(stem):
    rem, asm = open(stem + ".remarks").read(), open(stem + ".s").read()
    out = collections.OrderedDict()
    for blk in rem.split("Function Name: ")[1:]:
        fn = blk.split()[0]
        g = lambda k: int(re.search(re.escape(k) + r": (\d+)", blk).group(1))
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(fn), asm, re.S | re.M).group(1)
        lines = [l.split(";")[0].strip() for l in body.split("\n")]
        lines = [re.sub(r"\.LBB\d+_", "L", l.replace(fn, "SYM")) for l in lines if l and not l.startswith(".") or l.startswith(".LBB")]
        out[demangle(fn)] = dict(vgpr=g("VGPRs"), agpr=g("AGPRs"), sgpr=g("TotalSGPRs"), lds=g("LDS Size [bytes/block]"),
                                 scratch=g("ScratchSize [bytes/lane]"), waves=g("Occupancy [waves/SIMD]"),
                                 sspill=g("SGPRs Spill"), lines=lines)
    return out


def insns(lines):
    return [l for l in lines if not l.endswith(":")]


def mnem(l):
    m = l.split()[0]
    return m + " " + l.split()[1] if m == "s_waitcnt" and "vmcnt" in l else m  # vmcnt waits with their count


def blocks(lines):
    """Basic blocks [label, instructions] and their successors."""
    bl, cur = [], [None, []]
    for l in lines:
        if l.endswith(":"):
            if cur[0] or cur[1]:
                bl.append(cur)
            cur = [l[:-1], []]
        else:
            cur[1].append(l)
            if l.split()[0].startswith(("s_cbranch", "s_branch", "s_endpgm")):
                bl.append(cur)
                cur = [None, []]
    if cur[0] or cur[1]:
        bl.append(cur)
    at = {b[0]: i for i, b in enumerate(bl) if b[0]}
    succ = []
    for i, b in enumerate(bl):
        t = b[1][-1].split() if b[1] else [""]
        nxt = [i + 1] if i + 1 < len(bl) else []
        succ.append([at[t[-1]]] + nxt if t[0].startswith("s_cbranch") else [at[t[-1]]] if t[0] == "s_branch" else
                    [] if t[0] == "s_endpgm" else nxt)
    return bl, succ


def natural_loops(succ):
    """header -> blocks of the loop, from the back edges (an edge to a block that dominates its source)."""
    n = len(succ)
    pred = [[p for p in range(n) if i in succ[p]] for i in range(n)]
    dom = [{0}] + [set(range(n)) for _ in range(n - 1)]
    changed = True
    while changed:
        changed = False
        for i in range(1, n):
            d = (set.intersection(*[dom[p] for p in pred[i]]) if pred[i] else set()) | {i}
            changed, dom[i] = changed or d != dom[i], d
    lp = {}
    for t in range(n):
        for h in succ[t]:
            if h in dom[t]:
                body, todo = {h, t}, [t]
                while todo:
                    x = todo.pop()
                    todo += [p for p in pred[x] if x != h and p not in body and not body.add(p)]
                lp.setdefault(h, set()).update(body)
    return lp


def parts(lines):
    """stream = the loop over the chunk without the processing pass inside it; pass = the loop(s) that store records."""
    bl, succ = blocks(lines)
    has = lambda body, pat: any(pat in l for i in body for l in bl[i][1])
    lp = [b for b in natural_loops(succ).values() if has(b, "global_load")]
    outer = max(lp, key=len)
    inner = [b for b in lp if b < outer and has(b, "global_store_dwordx4")]
    pas = max(inner, key=len) if inner else outer if has(outer, "global_store_dwordx4") else set()
    ins = lambda idx: [l for i in sorted(idx) for l in bl[i][1]]
    rest = set(range(len(bl))) - outer
    return collections.OrderedDict((("prologue", ins(i for i in rest if i < min(outer))), ("stream", ins(outer - pas)),
                                    ("pass", ins(pas)), ("epilogue", ins(i for i in rest if i > min(outer)))))


def loop_parts(lines):
    """prologue / loops (the union of the natural loops) / epilogue; a kernel without a loop is all prologue."""
    bl, succ = blocks(lines)
    loops = set().union(*natural_loops(succ).values()) if natural_loops(succ) else set()
    ins = lambda idx: [l for i in sorted(idx) for l in bl[i][1]]
    rest = set(range(len(bl))) - loops
    first = min(loops) if loops else len(bl)
    return collections.OrderedDict((("prologue", ins(i for i in rest if i < first)), ("loops", ins(loops)),
                                    ("epilogue", ins(i for i in rest if i > first))))


def hot(ins):
    """What a loop must keep: MFMA, LDS, global-memory instructions, barriers and vmcnt waits, by mnemonic."""
    keep = ("v_mfma", "ds_", "global_", "flat_", "buffer_", "s_barrier")
    return collections.Counter(m for m in map(mnem, ins) if m.startswith(keep) or m.startswith("s_waitcnt vmcnt"))


def mem_profile(ins):
    r = []
    for l in ins:
        m = l.split()[0]
        if m.startswith(("global_load", "flat_load", "global_store")):
            r.append(m)
        elif m == "s_waitcnt" and "vmcnt" in l:
            r.append("vmcnt(%s)" % l.split("vmcnt(")[1].split(")")[0])
        elif m == "s_barrier":
            r.append("barrier")
    return " ".join(r)


def main(pa, br, renamed=(), loops=False):
    A, B = load(pa), load(br)
    for pair in renamed:  # a renamed kernel is listed under "parent name -> branch name"
        old, new = pair.split("=")
        A = collections.OrderedDict((old + " -> " + new if k == old else k, v) for k, v in A.items())
        B = collections.OrderedDict((old + " -> " + new if k == new else k, v) for k, v in B.items())
    assert list(A) == list(B) or set(A) == set(B), (set(A) ^ set(B))
    cols = ("vgpr", "agpr", "sgpr", "sspill", "lds", "scratch", "waves")  # sspill: SGPRs kept in VGPR lanes (never memory: scratch 0)
    print("%-34s %-42s %-42s %s" % ("kernel", "parent " + "/".join(cols) + "/insns", "branch", "instruction stream"))
    differ = []
    for k in A:
        x, y = A[k], B[k]
        row = lambda z: "/".join(str(z[c]) for c in cols) + "/%d" % len(insns(z["lines"]))
        same = [re.sub(r"L\d+", "L", l) for l in insns(x["lines"])] == [re.sub(r"L\d+", "L", l) for l in insns(y["lines"])]
        if not same:
            differ.append(k)
        print("%-34s %-42s %-42s %s" % (k, row(x), row(y), "identical" if same else "differs"))
    for k in differ:
        print("\n== %s" % k)
        cut = loop_parts if loops else parts
        px, py = cut(A[k]["lines"]), cut(B[k]["lines"])
        for part in px:
            cx, cy = collections.Counter(map(mnem, px[part])), collections.Counter(map(mnem, py[part]))
            d = {m: cy[m] - cx[m] for m in sorted(set(cx) | set(cy)) if cy[m] != cx[m]}
            print("  %-8s %5d -> %5d instructions; branch - parent: %s" % (part, len(px[part]), len(py[part]),
                  " ".join("%s %+d" % kv for kv in d.items()) or "same histogram"))
        if loops:
            hx, hy = hot(px["loops"]), hot(py["loops"])
            print("  loops: MFMA, LDS, global memory, barriers, vmcnt waits: %s" % (
                "the parent's (%s)" % " ".join("%s x%d" % kv for kv in sorted(hx.items())) if hx == hy else
                "DIFFER: " + " ".join("%s %+d" % (m, hy[m] - hx[m]) for m in sorted(set(hx) | set(hy)) if hx[m] != hy[m])))
            continue
        for name, pz in (("parent", px), ("branch", py)):
            print("  %s stream, in layout order: %s" % (name, mem_profile(pz["stream"])))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--loops"]
    main(args[0], args[1], args[2:], "--loops" in sys.argv[1:])
