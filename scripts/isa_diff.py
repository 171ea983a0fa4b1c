"""Kernel-by-kernel comparison of two gfx950 assembly files (hipcc --cuda-device-only -S).
Usage: isa_diff.py OLD.s NEW.s [--kernel SUBSTR]

Splits both files by kernel symbol, renumbers the block labels of each kernel in order of first
appearance (so a kernel that merely moved in the file compares equal) and prints, per kernel,
`identical`, `only in OLD` / `only in NEW`, or `differs` with both sides' instruction counts by
class (as isa_stats.py) and register, scratch and LDS sizes.  A text comparison: it looks for no
particular instruction.  Exit status 1 if any kernel differs or is missing."""
import argparse
import re
import sys

CLASSES = (("valu", "v_"), ("salu", "s_"), ("vmem", ("global_", "buffer_", "flat_", "scratch_")), ("lds", "ds_"))
SIZES = (("vgpr", ".amdhsa_next_free_vgpr"), ("sgpr", ".amdhsa_next_free_sgpr"),
         ("scratch", ".amdhsa_private_segment_fixed_size"), ("lds_bytes", ".amdhsa_group_segment_fixed_size"))
LABEL = re.compile(r"\.L(?:BB|func_end|func_begin|tmp)\d+(?:_\d+)?")


def split_kernels(text):
    """{symbol: (code lines, kernel-descriptor lines)} of every `.amdhsa_kernel` in the file."""
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\s*$(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S):
        sym = m.group(1)
        i = text.index("\n" + sym + ":") + 1
        j = text.index(".Lfunc_end", i)
        code = [ln.split(";")[0].strip() for ln in text[i:j].splitlines()]
        desc = [ln.strip() for ln in m.group(2).splitlines() if ln.strip()]
        out[sym] = ([ln for ln in code if ln], desc)
    return out


def relabel(lines):
    names = {}
    return [LABEL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), ln) for ln in lines]


def counts(code, desc):
    ins = [ln for ln in code if not ln.startswith(".") and not ln.endswith(":")]
    c = {"total": len(ins)}
    for k, pre in CLASSES:
        c[k] = sum(1 for x in ins if x.startswith(pre))
    for k, key in SIZES:
        v = [ln.split()[1] for ln in desc if ln.split()[0] == key]
        c[k] = int(v[0]) if v else None
    return c


def diff(old_text, new_text, substr=""):
    """[(symbol, verdict, old counts or None, new counts or None)], sorted by symbol."""
    old, new = split_kernels(old_text), split_kernels(new_text)
    rows = []
    for sym in sorted(set(old) | set(new)):
        if substr not in sym:
            continue
        if sym not in new or sym not in old:
            rows.append((sym, "only in OLD" if sym in old else "only in NEW", None, None))
            continue
        (oc, od), (nc, nd) = old[sym], new[sym]
        if relabel(oc) == relabel(nc) and od == nd:
            rows.append((sym, "identical", None, None))
        else:
            rows.append((sym, "differs", counts(oc, od), counts(nc, nd)))
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--kernel", default="", help="only kernels whose symbol contains this")
    a = ap.parse_args()
    rows = diff(open(a.old).read(), open(a.new).read(), a.kernel)
    for sym, verdict, oc, nc in rows:
        print(f"{verdict:12s} {sym}")
        if oc:
            print("    old " + " ".join(f"{k}={v}" for k, v in oc.items()))
            print("    new " + " ".join(f"{k}={v}" for k, v in nc.items()))
    n = {v: sum(1 for r in rows if r[1] == v) for v in ("identical", "differs", "only in OLD", "only in NEW")}
    print(f"{len(rows)} kernels: " + ", ".join(f"{c} {v}" for v, c in n.items()))
    sys.exit(0 if n["identical"] == len(rows) else 1)
