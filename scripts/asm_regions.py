"""Static instruction counts per region of one kernel, from the compiler's assembly listing.

  hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -std=c++17 -I../include -gline-tables-only \
        --cuda-device-only -S csrc/sg_stack_hist.hip -o hist.s
  python3 scripts/asm_regions.py hist.s 'k_stack_histILi2ELi0EE'                 # every basic block
  python3 scripts/asm_regions.py hist.s 'k_stack_histILi2ELi0EE' \
        --region pass=.LBB0_61-.LBB0_61+2 --region removal=.LBB0_70                  # sums over block runs

The listing of the kernel whose symbol matches the pattern is cut into basic blocks at its labels
and after every branch (the fall-through block after the k-th branch below LABEL is LABEL+k).
Every instruction is put into a class by its mnemonic's prefix alone (v_ = VALU, s_ = SALU with
the no-ops, waits and branches apart, ds_ = LDS, buffer_/global_/flat_/scratch_ = VMEM); nothing is
searched for by name.  With line tables in the listing (-gline-tables-only, which does not change
the code) each block also shows the span of source lines its instructions come from, innermost
inlined function first, which is how a block is matched to a source region; a region is a label
or an inclusive run FIRST-LAST of labels in listing order.  Label numbers change with every edit
of the source: read them off the block table of the build in hand."""
import argparse
import collections
import re
import sys

CLASSES = ("valu", "salu", "lds", "vmem", "nop", "wait", "branch", "other")


def classify(m):
    if m.startswith("v_"):
        return "valu"
    if m.startswith("ds_"):
        return "lds"
    if m.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if m.startswith(("s_nop", "s_sleep")):
        return "nop"
    if m.startswith(("s_waitcnt", "s_barrier")):
        return "wait"
    if m.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc", "s_swappc")):
        return "branch"
    if m.startswith("s_"):
        return "salu"
    return "other"


def blocks_of(path, pattern):
    """[(label, Counter, {file: (min line, max line)})] of the first function matching pattern."""
    sym = re.compile(pattern)
    label = re.compile(r"^([.\w$]+):")
    loc = re.compile(r"^\s+\.loc\s+(\d+)\s+(\d+)")
    ins = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")
    out, cur, inside = [], None, False
    fileno, base, parts, split = None, None, 0, False
    for line in open(path):
        m = label.match(line)
        if m:
            name = m.group(1)
            if not inside:
                if sym.search(name) and not name.startswith("."):
                    inside = True
                    cur = [name, collections.Counter(), {}]
                    out.append(cur)
                    base = name
                continue
            if name.startswith(".Lfunc_end"):
                break
            if name.startswith(".LBB"):
                cur = [name, collections.Counter(), {}]
                out.append(cur)
                base, parts, split = name, 0, False
            continue
        if not inside:
            continue
        m = loc.match(line)
        if m:
            fileno = (int(m.group(1)), int(m.group(2)))
            continue
        if line.lstrip().startswith((".", ";")):
            continue
        m = ins.match(line)
        if m:
            if split:                   # the fall-through block after a branch carries no label
                parts += 1
                cur = ["%s+%d" % (base, parts), collections.Counter(), {}]
                out.append(cur)
                split = False
            kind = classify(m.group(1))
            cur[1][kind] += 1
            split = kind == "branch"
            if fileno and fileno[1]:    # line 0: no source position
                f, ln = fileno
                lo, hi = cur[2].get(f, (ln, ln))
                cur[2][f] = (min(lo, ln), max(hi, ln))
    return out


def fmt(c):
    return " ".join("%s %d" % (k, c[k]) for k in CLASSES if c[k])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("listing")
    ap.add_argument("symbol", help="regular expression matched against the kernel's (mangled) symbol")
    ap.add_argument("--region", action="append", default=[], metavar="NAME=FIRST[-LAST]")
    a = ap.parse_args()
    blocks = blocks_of(a.listing, a.symbol)
    if not blocks:
        sys.exit("no function matches " + a.symbol)
    index = {b[0]: i for i, b in enumerate(blocks)}
    if not a.region:
        for name, c, src in blocks:
            span = ", ".join("f%d:%d-%d" % (f, lo, hi) for f, (lo, hi) in sorted(src.items()))
            print("%-12s %-60s %s" % (name, fmt(c), span))
    total = collections.Counter()
    for b in blocks:
        total.update(b[1])
    for r in a.region:
        name, _, span = r.partition("=")
        first, _, last = span.partition("-")
        i, j = index[first], index[last or first]
        c = collections.Counter()
        for b in blocks[i:j + 1]:
            c.update(b[1])
        print("%-24s %s" % (name, fmt(c)))
    print("%-24s %s" % ("whole kernel", fmt(total)))


if __name__ == "__main__":
    main()
