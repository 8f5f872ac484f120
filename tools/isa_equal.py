#!/usr/bin/env python3
"""Are two builds of the engine's device code the same, kernel by kernel?  (CPU only.)

    tools/isa_equal.py A B [--units pass_pair,pass_flat] [--jobs 4] [--keep DIR]

A and B are each a source tree (holding fluidframework_amd/csrc) or a directory
of listings <unit>.s with the compiler's remarks in <unit>.remarks.  A source
tree is cross-compiled first: every unit of libmte.so and the two `prof`
objects, with `hipcc --cuda-device-only -S -Rpass-analysis=kernel-resource-usage`
(--keep DIR leaves the listings in DIR/a and DIR/b for a later run).  For each
function (mangled name -> its lines, comments and .LBB label numbers stripped)
it prints EQ or DIFF with both line counts, then compares the resource-usage
remark values; the exit status is non-zero on any difference or missing kernel.
Listings, not .hip_fatbin hashes: the compile-unit id follows the build path.
"""
import argparse, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950"]  # csrc/Makefile HIPFLAGS
# unit -> (source, extra flags); cheapest first, the tree units take minutes
UNITS = {"query": ("mte_query.hip", []), "pass_pair": ("mte_pass_pair.hip", None),
         "engine": ("mte_engine.hip", []), "pass_chunk": ("mte_pass_chunk.hip", []),
         "pass_flat": ("mte_pass_flat.hip", []),
         "pass_tree": ("mte_pass_tree.hip", []), "pass_htree": ("mte_pass_htree.hip", []),
         "pass_tree_prof": ("mte_pass_tree.hip", ["-DMTE_TREE_PROF"]),
         "pass_htree_prof": ("mte_pass_htree.hip", ["-DMTE_HTREE_PROF"])}


def listings(tree, out, units, jobs):
    """Compile `units` of the source tree into out/<unit>.s and out/<unit>.remarks."""
    csrc = os.path.join(tree, "fluidframework_amd", "csrc")
    if not os.path.isdir(csrc):
        return tree  # already a directory of listings
    os.makedirs(out, exist_ok=True)
    pair = subprocess.check_output(["make", "-s", "pair-flags"], cwd=csrc, text=True).split()

    def one(u):
        src, extra = UNITS[u]
        cmd = [HIPCC, *FLAGS, *(pair if extra is None else extra), "--cuda-device-only", "-S",
               "-Rpass-analysis=kernel-resource-usage", "-o", os.path.abspath(f"{out}/{u}.s"), src]
        r = subprocess.run(cmd, cwd=csrc, stderr=subprocess.PIPE, text=True)
        if r.returncode:
            sys.exit(f"{tree}: {u} does not compile\n{r.stderr[-2000:]}")
        with open(f"{out}/{u}.remarks", "w") as f:
            f.write(r.stderr)

    with ThreadPoolExecutor(jobs) as ex:
        list(ex.map(one, units))
    return out


def functions(path):
    """mangled name -> the function's lines up to .Lfunc_end, comments and label numbers stripped."""
    fns, cur = {}, None
    for line in open(path):
        line = re.sub(r"\.LBB\d+_\d+", ".LBB", line.split(";")[0]).strip()
        m = re.match(r"\.type\s+(\S+),@function", line)
        if m:
            cur = fns.setdefault(m.group(1), [])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and line:
            cur.append(line)
    return fns


def remarks(path):
    """mangled name -> {resource: value}, source positions dropped (code may move between files)."""
    res, cur = {}, None
    for m in re.finditer(r"remark:\s+(.+?):\s+(\S+) \[-Rpass-analysis", open(path).read()):
        if m.group(1) == "Function Name":
            cur = res.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a"), ap.add_argument("b")
    ap.add_argument("--units", default=",".join(UNITS))
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--keep", help="write listings compiled here to DIR/a and DIR/b")
    o = ap.parse_args()
    units = o.units.split(",")
    keep = o.keep or tempfile.mkdtemp(prefix="isa_equal_")
    a = listings(o.a, f"{keep}/a", units, o.jobs)
    b = listings(o.b, f"{keep}/b", units, o.jobs)
    bad = 0
    for u in units:
        fa, fb = functions(f"{a}/{u}.s"), functions(f"{b}/{u}.s")
        ra, rb = remarks(f"{a}/{u}.remarks"), remarks(f"{b}/{u}.remarks")
        if not fa:
            print(f"{u}: no function in {a}/{u}.s"); bad += 1
        for k in sorted(set(fa) | set(fb)):
            if k not in fa or k not in fb:
                print(f"{u} MISSING in {'a' if k not in fa else 'b'}  {k}"); bad += 1
                continue
            eq = fa[k] == fb[k]
            print(f"{u} {'EQ  ' if eq else 'DIFF'} {len(fa[k]):6d} {len(fb[k]):6d}  {k}")
            bad += not eq
        for k in sorted(set(ra) | set(rb)):
            if ra.get(k) != rb.get(k):
                print(f"{u} REMARKS differ  {k}\n    a: {ra.get(k)}\n    b: {rb.get(k)}"); bad += 1
        print(f"{u}: {len(fa)} functions, remarks for {len(ra)} kernels")
    print("ALL EQ" if not bad else f"{bad} difference(s)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
