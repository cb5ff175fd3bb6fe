"""VALU instructions of an integrate kernel's attempt loops, per basic block.

usage: python tools/hot_loop_mix.py [geometry=1] [kernel .s] [--ops]
Builds geodesic.hip for gfx950 (unless a .s from `hipcc -S --cuda-device-only` is given),
takes integrate_kernel<geometry, false>, builds its control-flow graph from the labels and
branches, and finds every innermost loop that holds at least six RHS blocks (a basic block
with two or more v_rcp_f64: one RKF45 attempt evaluates the RHS six times).  For each such
loop it prints, per basic block in layout order, the VALU instructions split into
  f64   FP64 arithmetic (v_*_f64 but the reciprocal)
  rcp   v_rcp_f64
  rest  every other VALU instruction (compares, selects, moves, lane access, integer)
and the scalar-memory loads, LDS and vector-memory instructions beside them.  With --ops the
`rest` column is listed by opcode.  A counter: it knows these categories and nothing else.
The loop totals are sums over all blocks of the loop, not over one path through it; the
blocks an RKF stage runs one of (the sincos cases) are told apart by their rcp counts."""
import collections
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def kernel_lines(asm: Path, geometry: int):
    S = asm.read_text().split("\n")
    name = f"_ZN3grt16integrate_kernelILi{geometry}ELb0EEE"
    start = next(i for i, l in enumerate(S) if re.match(re.escape(name) + r"\S*:", l))
    end = next(i for i in range(start, len(S)) if S[i].startswith(".Lfunc_end"))
    return S[start + 1:end]


def basic_blocks(lines):
    """[(label, [opcode and operands])] in layout order, and the successor lists."""
    blocks = [["entry", []]]
    for l in lines:
        m = re.match(r"^(\.LBB\S+):", l)
        if m:
            blocks.append([m.group(1), []])
            continue
        t = l.split(";")[0].strip()
        if t and not t.startswith("."):
            blocks[-1][1].append(t)
    index = {b[0]: k for k, b in enumerate(blocks)}
    succ = []
    for k, (_, ins) in enumerate(blocks):
        out, falls = [], True
        for t in ins:
            op, _, rest = t.partition(" ")
            if op.startswith("s_cbranch") or op == "s_branch":
                tgt = rest.strip().split(",")[-1].strip()
                if tgt in index:
                    out.append(index[tgt])
                if op == "s_branch":
                    falls = False
            elif op in ("s_endpgm", "s_setpc_b64"):
                falls = False
        if falls and k + 1 < len(blocks):
            out.append(k + 1)
        succ.append(out)
    return blocks, succ


def sccs(nodes, succ):
    """Strongly connected components of the subgraph on `nodes` (iterative Tarjan)."""
    nodes = set(nodes)
    idx, low, on, stack, out, n = {}, {}, set(), [], [], 0
    for root in sorted(nodes):
        if root in idx:
            continue
        work = [(root, iter([s for s in succ[root] if s in nodes]))]
        idx[root] = low[root] = n
        n += 1
        stack.append(root)
        on.add(root)
        while work:
            v, it = work[-1]
            for w in it:
                if w not in idx:
                    idx[w] = low[w] = n
                    n += 1
                    stack.append(w)
                    on.add(w)
                    work.append((w, iter([s for s in succ[w] if s in nodes])))
                    break
                if w in on:
                    low[v] = min(low[v], idx[w])
            else:
                work.pop()
                if work:
                    low[work[-1][0]] = min(low[work[-1][0]], low[v])
                if low[v] == idx[v]:
                    comp = set()
                    while True:
                        w = stack.pop()
                        on.discard(w)
                        comp.add(w)
                        if w == v:
                            break
                    if len(comp) > 1 or v in succ[v]:
                        out.append(comp)
    return out


def innermost_loops(nodes, succ, pred, is_rhs, outer_entries=()):
    """Innermost loops among `nodes` that hold at least six RHS blocks."""
    found = []
    for comp in sccs(nodes, succ):
        if sum(is_rhs[b] for b in comp) < 6:
            continue
        heads = {b for b in comp if any(p not in comp for p in pred[b])} or {min(comp)}
        inner = innermost_loops(comp - heads, succ, pred, is_rhs)
        found += inner if inner else [comp]
    return found


def category(op):
    if not op.startswith("v_"):
        if op.startswith(("s_load", "s_buffer_load")):
            return "smem"
        if op.startswith("ds_"):
            return "lds"
        if op.startswith("s_"):
            return "salu"
        return "vmem"
    base = re.sub(r"_(e32|e64|dpp|sdwa)$", "", op)
    if base == "v_rcp_f64":
        return "rcp"
    if base.endswith("_f64") and not base.startswith(("v_cmp", "v_cmpx", "v_cndmask", "v_mov")):
        return "f64"
    return "rest"


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    by_op = "--ops" in sys.argv
    g = int(args[0]) if args else 1
    if len(args) > 1:
        asm = Path(args[1])
    else:
        asm = Path(tempfile.mkdtemp(prefix="hot_loop_mix.")) / "geodesic.s"
        subprocess.run(["/opt/rocm/bin/hipcc", f"-I{ROOT}/include", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-ffp-contract=off", "-fno-fast-math", "-munsafe-fp-atomics", "--cuda-device-only", "-S",
                        str(ROOT / "gr_raytracer_amd/csrc/device/geodesic.hip"), "-o", str(asm)],
                       check=True, capture_output=True)
    blocks, succ = basic_blocks(kernel_lines(asm, g))
    pred = [[] for _ in blocks]
    for k, out in enumerate(succ):
        for s in out:
            pred[s].append(k)
    counts = []
    for _, ins in blocks:
        counts.append(collections.Counter((category(t.split()[0]), re.sub(r"_(e32|e64)$", "", t.split()[0])) for t in ins))
    cat_of = [collections.Counter() for _ in blocks]
    for k, c in enumerate(counts):
        for (cat, _), v in c.items():
            cat_of[k][cat] += v
    is_rhs = [c["rcp"] >= 2 for c in cat_of]
    loops = innermost_loops(range(len(blocks)), succ, pred, is_rhs)
    print(f"integrate_kernel<{g}, false>: {len(blocks)} basic blocks, {len(loops)} innermost loop(s) with six RHS blocks or more")
    cols = ("f64", "rcp", "rest", "salu", "smem", "lds", "vmem")
    for n, comp in enumerate(sorted(loops, key=min)):
        print(f"loop {n}: {len(comp)} blocks, {sum(is_rhs[b] for b in comp)} of them RHS blocks")
        print(f"  {'block':14s}" + "".join(f"{c:>6s}" for c in cols))
        total = collections.Counter()
        for b in sorted(comp):
            total.update(cat_of[b])
            print(f"  {blocks[b][0]:14s}" + "".join(f"{cat_of[b][c]:6d}" for c in cols) + ("  RHS" if is_rhs[b] else ""))
            if by_op:
                rest = {op: v for (cat, op), v in sorted(counts[b].items()) if cat == "rest"}
                if rest:
                    print("      " + ", ".join(f"{op} {v}" for op, v in rest.items()))
        print(f"  {'all blocks':14s}" + "".join(f"{total[c]:6d}" for c in cols))
        rest = collections.Counter()
        for b in comp:
            for (cat, op), v in counts[b].items():
                if cat == "rest":
                    rest[op] += v
        print("  rest by opcode, all blocks: " + ", ".join(f"{op} {v}" for op, v in sorted(rest.items())))


if __name__ == "__main__":
    main()
