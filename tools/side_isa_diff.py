"""The device code of the side libraries in two trees, kernel by kernel: is it the same, and if not, where does it part and what does it cost.
   usage: python tools/side_isa_diff.py OLD_TREE NEW_TREE [--libs elevation lidar ...] [--out profiles/NAME.txt]
Both trees are compiled by THIS checkout's csrc/pgtt_side.mk (`make asm resources`, so an OLD_TREE from before the `asm` target serves), each into
a temporary BUILD; nothing is written into either tree.  From the listing <lib>.s go the comments, the .loc / .file / .ident lines and the
__hip_cuid_* symbol (it differs between any two compilations); what is left is split per kernel symbol - the body up to its .Lfunc_end and its
.amdhsa_kernel block - its block labels are named in order of appearance, and the two are compared line by line.  Per kernel: `identical`, or both instruction counts and a unified diff of the first differing
region; then both trees' VGPRs / SGPRs / AGPRs / scratch / static LDS / occupancy side by side, from -Rpass-analysis=kernel-resource-usage.
It compares two listings and says where they differ; it needs no GPU.  Exit status: non-zero on a build failure only."""
import argparse
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "phase_guided_terrain_traversal_amd"
ALL_LIBS = ("render", "depth", "perceive", "elevation", "learn", "lidar")
FIELDS = (("VGPRs", r"\bVGPRs: (\d+)"), ("SGPRs", r"TotalSGPRs: (\d+)"), ("AGPRs", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
          ("LDS", r"LDS Size \[bytes/block\]: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"))


def build(tree, libs, tmp):
    """-> {lib: listing text}, {kernel symbol: {field: int}}"""
    csrc = os.path.join(os.path.abspath(tree), PKG, "csrc")
    cmd = ["make", "-C", csrc, "-f", os.path.join(ROOT, PKG, "csrc", "pgtt_side.mk"), "LIBS=" + " ".join(libs), "BUILD=" + tmp, "asm", "resources"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.stdout.write(r.stdout)
        sys.exit(f"side_isa_diff: the build of {tree} failed")
    res, cur = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        for name, pat in FIELDS:
            m = re.search(pat, line)
            if m and cur is not None:
                cur[name] = int(m.group(1))
    listings = {}
    for lib in libs:
        with open(os.path.join(tmp, lib + ".s")) as fh:
            listings[lib] = fh.read()
    return listings, res


def kernels(listing):
    """-> {symbol: [cleaned lines]} in the listing's order: each function's body and, behind it, its .amdhsa_kernel block"""
    out, cur = {}, None
    for raw in listing.splitlines():
        line = raw.split(";", 1)[0].rstrip()
        s = line.strip()
        if not s or s.startswith((".loc", ".file", ".ident", ".cfi_")) or "__hip_cuid_" in s:
            continue
        m = re.match(r"\.type\s+(\S+),@function", s)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", s)
        if m:
            cur = out.setdefault(m.group(1), [])
        if cur is not None:
            cur.append(" ".join(s.split()))
        if s.startswith(".Lfunc_end") or s == ".end_amdhsa_kernel":
            cur = None
    # block labels are numbered by the compiler's block order, which an edit elsewhere in the function shifts: name them in order of appearance
    for sym, lines in out.items():
        seen = {}
        out[sym] = [re.sub(r"\.LBB\d+_\d+", lambda m: seen.setdefault(m.group(0), f".L{len(seen)}"), s) for s in lines]
    return out


def n_instr(lines):
    return sum(1 for s in lines if not s.startswith(".") and not s.endswith(":"))


def demangle(names):
    rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-cxxfilt")
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or (rocm if os.path.exists(rocm) else None)
    if not tool or not names:
        return {n: n for n in names}
    r = subprocess.run([tool] + list(names), stdout=subprocess.PIPE, text=True)
    got = r.stdout.splitlines()
    short = [re.sub(r"\(anonymous namespace\)::|\(.*\)$|^void ", "", g) for g in got]
    return dict(zip(names, short)) if len(got) == len(names) else {n: n for n in names}


def first_region(a, b, context=3, limit=60):
    """a unified diff of the first region where the two line lists differ"""
    for group in difflib.SequenceMatcher(None, a, b, autojunk=False).get_grouped_opcodes(context):
        out = []
        for tag, i1, i2, j1, j2 in group:
            if tag == "equal":
                out += ["   " + s for s in a[i1:i2]]
            else:
                out += ["-  " + s for s in a[i1:i2]] + ["+  " + s for s in b[j1:j2]]
        return [f"   @@ old line {group[0][1] + 1}, new line {group[0][3] + 1} @@"] + out[:limit] + (["   ..."] if len(out) > limit else [])
    return []


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--libs", nargs="+", default=list(ALL_LIBS), choices=ALL_LIBS)
    ap.add_argument("--out")
    args = ap.parse_args()
    built = []
    for tree in (args.old_tree, args.new_tree):
        tmp = tempfile.mkdtemp(prefix="side_isa_")
        try:
            built.append(build(tree, args.libs, tmp))
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    (lst_a, res_a), (lst_b, res_b) = built
    lines = [f"# tools/side_isa_diff.py --libs {' '.join(args.libs)}: the device code (gfx950) of two trees, per kernel; old = first tree, new = second",
             "# compared: the listing without comments, .loc / .file / .ident and the __hip_cuid_* symbol"]
    n_same = n_diff = 0
    for lib in args.libs:
        ka, kb = kernels(lst_a[lib]), kernels(lst_b[lib])
        names = list(ka) + [k for k in kb if k not in ka]
        nice = demangle(names)
        lines.append(f"\n== libpgtt_{lib}: {len(names)} kernels")
        for k in names:
            if k not in ka or k not in kb:
                lines.append(f"{nice[k]}: only in the {'old' if k in ka else 'new'} tree")
                n_diff += 1
            elif ka[k] == kb[k]:
                lines.append(f"{nice[k]}: identical ({n_instr(ka[k])} instructions)")
                n_same += 1
            else:
                lines.append(f"{nice[k]}: DIFFERENT, {n_instr(ka[k])} -> {n_instr(kb[k])} instructions")
                lines += first_region(ka[k], kb[k])
                n_diff += 1
        lines.append(f"\n{'kernel':58s} " + " ".join(f"{name:>11s}" for name, _ in FIELDS) + "   (old -> new)")
        for k in names:
            ra, rb = res_a.get(k, {}), res_b.get(k, {})
            cells = []
            for name, _ in FIELDS:
                x, y = ra.get(name, "-"), rb.get(name, "-")
                cells.append(f"{str(x) if x == y else f'{x}->{y}':>11s}")
            lines.append(f"{nice[k]:58s} " + " ".join(cells))
    lines.append(f"\n{n_same} kernels identical, {n_diff} different")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
