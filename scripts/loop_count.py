"""Instructions on the path of ONE plain ADMM iteration (no factorisation, no check, no exit) of the MPC kernel, by class,
counted in a listing compiled with the SHIPPED flags (no phase markers: scripts/phase_mix.py needs them and they move the
register allocation).  Kernels: the N = 16 FULL instantiation <1,true,false,false> and the runtime-horizon one
<1,false,false,false>.

    python scripts/loop_count.py                  compiles csrc/mpc_kernel.hip and counts
    python scripts/loop_count.py --listing x.s    counts in an existing listing (e.g. one of an earlier commit)

The path is found twice, and the two must agree wherever both exist:
  path   the control-flow graph of the kernel is followed from the basic block of the Delta^-1 product (it reads the parked
         Delta^-1 rows, 24 accumulation registers per asm statement) round to itself along the cheapest cycle, an s_cbranch_execz never taken
         -- EXEC is never empty on this path -- unless it skips a factorisation, and an s_cbranch_execnz always.  Works in every form of the loop: where checks and
         factorisations hang off the iteration as side blocks, the path crosses several blocks and skips them.
  loop   the innermost loop around that block taken whole: the one that holds the sweeps' v_fmac_f64_dpp.  It is the plain iteration only
         where the loop holds nothing else, i.e. since the loop runs in check-free blocks (docs/HISTORY.md 6b); in older
         listings it also holds the check and the factorisation and the figure is printed for information."""
import argparse
import collections
import heapq
import os
import re
import subprocess
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(R, "quadruped-reactive-walking_amd", "csrc")
KERNELS = collections.OrderedDict([
    ("<1,true,false,false>", "_ZN3qrw16mpc_solve_kernelILi1ELb1ELb0ELb0EEEvNS_7MpcArgsE"),
    ("<1,false,false,false>", "_ZN3qrw16mpc_solve_kernelILi1ELb0ELb0ELb0EEEvNS_7MpcArgsE"),
])
CLASSES = ("fp64", "accvgpr", "lds", "v_mov_b32_dpp", "v_mov_b32", "valu32", "s_nop", "s_waitcnt", "branch/EXEC", "salu",
           "vmem", "scratch", "other")


def shipped_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    return re.search(r"^MPCFLAGS\s*:=\s*(.*)$", mk, re.M).group(1).split()


def compile_listing(out, defs=()):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-pass-failed",
                           "-Wno-unused-value", "-Wno-unused-result", "-Wno-unused-function"] + shipped_flags() + list(defs) +
                          ["-I" + os.path.join(R, "include"), "-I" + CSRC, os.path.join(CSRC, "mpc_kernel.hip"), "-o", out])
    return out


def touches_exec(ins):
    """EXEC-mask bookkeeping: s_*_saveexec_*, or a scalar instruction whose destination is exec."""
    op = ins.split()[0]
    if not op.startswith("s_"):
        return False
    if "saveexec" in op:
        return True
    ops = ins[len(op):].split(",")
    return bool(ops) and ops[0].strip() in ("exec", "exec_lo", "exec_hi")


def classify(ins):
    op = ins.split()[0]
    if op.startswith("v_accvgpr"): return "accvgpr"
    if op.startswith("scratch_"): return "scratch"
    if op.startswith("ds_"): return "lds"
    if op.startswith(("global_", "flat_", "buffer_")): return "vmem"
    if op.startswith("v_mov_b32"): return "v_mov_b32_dpp" if "dpp" in op or "row_" in ins or "quad_perm" in ins else "v_mov_b32"
    if op.startswith("v_") and "f64" in op: return "fp64"
    if op.startswith("v_"): return "valu32"
    if op == "s_nop": return "s_nop"
    if op == "s_waitcnt": return "s_waitcnt"
    if op.startswith(("s_cbranch", "s_branch")) or touches_exec(ins): return "branch/EXEC"
    if op.startswith("s_"): return "salu"
    return "other"


class Block:
    def __init__(self, idx, label):
        self.idx, self.label, self.ins, self.succ = idx, label, [], []  # succ: (block index, kind)
        self.rows = 0  # asm statements that read 24 accumulation registers at once (AccD::get12: one Delta^-1 row)


def kernel_blocks(txt, symbol):
    """Basic blocks of one kernel in listing order; a block ends at a label or behind a branch."""
    body = txt[txt.index(symbol + ":"):]
    body = body[:body.index(".Lfunc_end")]
    blocks, cur = [], Block(0, None)
    in_asm = None
    for line in body.splitlines()[1:]:
        if "#ASMSTART" in line:
            in_asm = 0
        elif "#ASMEND" in line:
            cur.rows += in_asm == 24
            in_asm = None
        t = line.split(";")[0].strip()
        if in_asm is not None and t.startswith("v_accvgpr_read"):
            in_asm += 1
        if not t or t.startswith((".", "#")) and not t.endswith(":"):
            continue
        if t.endswith(":"):
            if cur.ins or cur.label is not None:  # (an empty labelled block still is a branch target)
                blocks.append(cur)
            cur = Block(len(blocks), t[:-1])
            continue
        cur.ins.append(t)
        if t.startswith(("s_cbranch", "s_branch")):
            blocks.append(cur)
            cur = Block(len(blocks), None)
    blocks.append(cur)
    for i, b in enumerate(blocks):
        b.idx = i
    by_label = {b.label: b.idx for b in blocks if b.label}
    anchor = anchor_block(blocks)
    for b in blocks:
        last = b.ins[-1] if b.ins else ""
        op = last.split()[0] if last else ""
        nxt = b.idx + 1 if b.idx + 1 < len(blocks) else None
        if op == "s_branch":
            b.succ = [(by_label[last.split()[1]], "taken")]
        elif op.startswith("s_cbranch"):
            tgt = by_label[last.split()[1]]
            if op == "s_cbranch_execz":
                # EXEC is never empty on the plain path, with one exception: where the decision to factorise is carried in
                # a lane mask, the branch around the factorisation (the only code of the loop that writes AGPRs) is taken
                # (a branch that skips the iteration itself is the loop's exit)
                skipped = blocks[b.idx + 1:tgt] if tgt > b.idx and not b.idx < anchor < tgt else []
                factor = any(t.startswith("v_accvgpr_write") for x in skipped for t in x.ins)
                b.succ = [(tgt, "taken")] if factor else [(nxt, "fall")]
            elif op == "s_cbranch_execnz":
                b.succ = [(tgt, "taken")]
            else:
                b.succ = [(tgt, "taken")] + ([(nxt, "fall")] if nxt is not None else [])
        elif nxt is not None:
            b.succ = [(nxt, "fall")]
    return blocks


def anchor_block(blocks):
    """The block of the Delta^-1 product between the two sweeps: the last one, in listing order, with an asm statement that
    reads a whole parked Delta^-1 row (AccD::get12, 24 accumulation registers; nothing else reads them that way)."""
    hits = [b.idx for b in blocks if b.rows]
    if not hits:
        raise RuntimeError("no block reads a parked Delta^-1 row")
    return hits[-1]


def cheapest_cycle(blocks, start):
    """Blocks of the cheapest cycle start -> ... -> start, the cost of entering a block being its instruction count."""
    dist, prev = {}, {}
    heap = [(len(blocks[s].ins), s, start) for s, _ in blocks[start].succ]
    while heap:
        d, u, p = heapq.heappop(heap)
        if u in dist:
            continue
        dist[u], prev[u] = d, p
        if u == start:
            break
        for s, _ in blocks[u].succ:
            if s not in dist:
                heapq.heappush(heap, (d + len(blocks[s].ins), s, u))
    if start not in dist:
        raise RuntimeError("the sweep block is in no loop")
    path, u = [start], prev[start]
    while u != start:
        path.append(u)
        u = prev[u]
    return list(reversed(path))


def innermost_loop(blocks, start):
    """Blocks [h .. u] in listing order: h the nearest loop header at or before `start` that has a backward branch from at or
    behind `start`, u the last block that branches back to h."""
    back = collections.defaultdict(list)  # header -> sources of its backward branches
    by_label = {b.label: b.idx for b in blocks if b.label}
    for b in blocks:
        last = b.ins[-1] if b.ins else ""
        if last.startswith(("s_cbranch", "s_branch")):
            h = by_label.get(last.split()[1])
            if h is not None and h <= b.idx:
                back[h].append(b.idx)
    heads = [h for h, us in back.items() if h <= start <= max(us)]
    if not heads:
        raise RuntimeError("no backward branch around the anchor block")
    h = max(heads)
    return list(range(h, max(back[h]) + 1))


def count(blocks, idxs):
    c = collections.Counter()
    for i in idxs:
        for t in blocks[i].ins:
            c[classify(t)] += 1
    return c


def analyse(txt, symbol):
    blocks = kernel_blocks(txt, symbol)
    s = anchor_block(blocks)
    path, loop = cheapest_cycle(blocks, s), innermost_loop(blocks, s)
    pc, lc = count(blocks, path), count(blocks, loop)
    exec_ins = [t for i in path for t in blocks[i].ins if touches_exec(t) or t.startswith(("s_cbranch_execz", "s_cbranch_execnz"))]
    branches = [t for i in path for t in blocks[i].ins if t.startswith(("s_cbranch", "s_branch"))]
    return dict(path_total=sum(pc.values()), path=pc, path_blocks=len(path), loop_total=sum(lc.values()), loop=lc,
                loop_blocks=len(loop), exec_mask=exec_ins, branches=branches)


def report(txt, out=sys.stdout):
    res = collections.OrderedDict()
    for name, sym in KERNELS.items():
        r = res[name] = analyse(txt, sym)
        out.write("mpc_solve_kernel%s: one plain iteration = %d instructions over %d basic block(s) [path]; innermost loop = %d "
                  "instructions over %d block(s) [loop]: %s\n" % (name, r["path_total"], r["path_blocks"], r["loop_total"], r["loop_blocks"],
                                                                   "the two agree" if r["path_total"] == r["loop_total"] else
                                                                   "the loop holds more than the plain iteration"))
        for c in CLASSES:
            if r["path"][c] or r["loop"][c]:
                out.write("    %-14s %4d   (loop %4d)\n" % (c, r["path"][c], r["loop"][c]))
        out.write("    EXEC-mask instructions on the path: %d %s\n" % (len(r["exec_mask"]), r["exec_mask"][:6]))
        out.write("    branches on the path: %s\n" % r["branches"])
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--listing", help="count in this listing instead of compiling the source")
    a = ap.parse_args()
    path = a.listing or compile_listing(os.path.join(R, "build", "mpc_ship.s"))
    report(open(path).read())
