#!/usr/bin/env python3
"""Do two trees compile to the same gfx950 kernels?   tools/isa_diff.py <tree A> <tree B> [-j N] [--only-a NAME.hip ...] [--only-b NAME.hip ...] [--resources]

The proof a kernel refactor wants, on any machine with hipcc (no GPU): every .hip of each tree's lsdradixsort_amd/csrc is
compiled, device code only, with the Makefile's flags; the assembly is cut into one piece per kernel symbol (its function
body and its .amdhsa_kernel descriptor) and normalised for what depends on the FILE a kernel is compiled in and not on the
kernel: comments, .ident, the __hip_cuid_* symbol, the function index inside .LBB<i>_<j> / .Lfunc_end<i> labels.  Printed per
mangled kernel name: same, differs, only in A, only in B -- and a count of each.  A kernel of A and a kernel of B that exist
on one side only and whose pieces are equal once each one's own name is masked are reported as `renamed` (a template
parameter gone from a signature changes the symbol and nothing else).  --resources adds, for kernels that differ, VGPRs,
scratch, occupancy and LDS of both sides from -Rpass-analysis=kernel-resource-usage.  Exit status 0 unless a compile fails."""
import argparse
import concurrent.futures
import glob
import os
import re
import shutil
import subprocess
import tempfile

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S"]
RESOURCES = {"vgprs": "VGPRs", "scratch": "ScratchSize [bytes/lane]", "occupancy": "Occupancy [waves/SIMD]", "lds": "LDS Size [bytes/block]"}


def compile_unit(hipcc, source, want_resources):
    """(assembly text, {kernel: resources}) of one translation unit."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "x.s")
        extra = ["-Rpass-analysis=kernel-resource-usage"] if want_resources else []
        p = subprocess.run([hipcc] + FLAGS + extra + [source, "-o", out], capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"{source}: hipcc failed\n{p.stderr[-3000:]}")
        res = {}
        for block in p.stderr.split("Function Name: ")[1:]:
            res[block.split()[0]] = {k: int(re.search(re.escape(label) + r": (\d+)", block).group(1)) for k, label in RESOURCES.items()}
        return open(out).read(), res


def normalise(line):
    line = re.sub(r"\s*;.*$", "", line).rstrip()          # comments (file-dependent ones among them)
    line = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", line)     # the function's index in its file
    line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)
    line = re.sub(r"__hip_cuid_\w+", "__hip_cuid", line)
    return line


def kernels_of(asm):
    """{mangled name: normalised text of the function body + its .amdhsa_kernel descriptor}."""
    lines = asm.split("\n")
    names = [m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))]
    pieces = {n: [] for n in names}
    current = None
    for l in lines:
        if l.lstrip().startswith(".ident"):
            continue
        m = re.match(r"(\S+):\s*(;.*)?$", l)
        if m and m.group(1) in pieces:
            current = m.group(1)                           # the function's entry label
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            current = m.group(1)
        if current is not None:
            n = normalise(l)
            if n.strip():
                pieces[current].append(n)
        if current is not None and (re.match(r"\s*\.end_amdhsa_kernel", l) or re.match(r"\.Lfunc_end\d+:", l)):
            current = None
    return {n: "\n".join(p) for n, p in pieces.items()}


def tree_kernels(tree, only, jobs, want_resources):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    sources = sorted(glob.glob(os.path.join(tree, "lsdradixsort_amd", "csrc", "*.hip")))
    if only:
        sources = [s for s in sources if os.path.basename(s) in only]
    text, where, res = {}, {}, {}
    with concurrent.futures.ThreadPoolExecutor(max_workers=jobs) as pool:
        for src, (asm, r) in zip(sources, pool.map(lambda s: compile_unit(hipcc, s, want_resources), sources)):
            for name, piece in kernels_of(asm).items():
                text[name], where[name] = piece, os.path.basename(src)
            res.update(r)
    return text, where, res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("-j", type=int, default=min(16, os.cpu_count() or 1), help="translation units compiled at a time (16 at most)")
    ap.add_argument("--only-a", nargs="*", default=None, help="translation units of tree A to compile (default: all)")
    ap.add_argument("--only-b", nargs="*", default=None, help="... of tree B")
    ap.add_argument("--resources", action="store_true", help="list the resources of kernels that differ")
    a = ap.parse_args()
    jobs = max(1, min(16, a.j))
    ta, wa, ra = tree_kernels(a.tree_a, a.only_a, jobs, a.resources)
    tb, wb, rb = tree_kernels(a.tree_b, a.only_b, jobs, a.resources)
    only_a = sorted(set(ta) - set(tb))
    only_b = sorted(set(tb) - set(ta))
    renamed = []
    for na in list(only_a):
        for nb in only_b:
            if ta[na].replace(na, "@") == tb[nb].replace(nb, "@"):
                renamed.append((na, nb))
                only_a.remove(na)
                only_b.remove(nb)
                break
    count = {"same": 0, "differs": 0, "renamed": len(renamed), "only in A": len(only_a), "only in B": len(only_b)}
    differing = []
    for n in sorted(set(ta) & set(tb)):
        verdict = "same" if ta[n] == tb[n] else "differs"
        count[verdict] += 1
        if verdict == "differs":
            differing.append(n)
        moved = "" if wa[n] == wb[n] else f"   [{wa[n]} -> {wb[n]}]"
        print(f"{verdict:9} {n}{moved}")
    for na, nb in renamed:
        print(f"renamed   {na} [{wa[na]}] -> {nb} [{wb[nb]}]   (same but for its own name)")
    for n in only_a:
        print(f"only in A {n}   [{wa[n]}]")
    for n in only_b:
        print(f"only in B {n}   [{wb[n]}]")
    if a.resources and differing:
        print("\nresources of the kernels that differ (A -> B): VGPRs, scratch B/lane, waves/SIMD, static LDS B")
        for n in differing:
            x, y = ra.get(n), rb.get(n)
            if x is None or y is None:
                print(f"{n}: no resource remark from hipcc on side {'A' if x is None else 'B'}")
                continue
            worse = "   WORSE" if y["scratch"] > x["scratch"] or y["occupancy"] < x["occupancy"] else ""
            print(f"{n}: vgprs {x['vgprs']} -> {y['vgprs']}, scratch {x['scratch']} -> {y['scratch']}, "
                  f"occupancy {x['occupancy']} -> {y['occupancy']}, lds {x['lds']} -> {y['lds']}{worse}")
    print("\n" + ", ".join(f"{k}: {v}" for k, v in count.items()))


if __name__ == "__main__":
    main()
