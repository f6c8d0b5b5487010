#!/usr/bin/env python
"""Compare the gfx950 instruction streams of kernels between a commit and the work tree (CPU only: needs hipcc, no GPU).

usage: python tools/kernel_isa_diff.py COMMIT FILE.hip OLD_KERNEL=NEW_KERNEL [OLD=NEW ...] [--max-diff-lines N]

FILE.hip is compiled twice, device-only to assembly, with the flags codd_amd.build.compile_cmd gives the product build
of that file: once as COMMIT has it (`git show COMMIT:FILE.hip` into a temporary directory, next to COMMIT's headers)
and once from the work tree.  A kernel is named as c++filt prints it without return type and parameter list
(``se3_gn_solve_kernel``, ``se3_gn_build_kernel<true>``).  Per pair the tool prints the resource-usage remarks of both
sides and either IDENTICAL or the mnemonics whose count changed and a unified diff of the two instruction streams
(comments and directives stripped, .LBB<n>_ labels normalised).  Exit status 1 on any difference.  It looks for no
particular instruction: it only compares.
"""
import argparse
import collections
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from codd_amd import build  # noqa: E402

RESOURCES = ("VGPRs", "TotalSGPRs", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]",
             "LDS Size [bytes/block]")


def git(*args):
    return subprocess.check_output(("git", "-C", ROOT) + args)


def checkout(commit, rel, dst):
    """COMMIT's copy of `rel` and of every header the product build can see, under dst/ at their repository paths."""
    dirs = sorted({"include", os.path.dirname(rel), os.path.relpath(build.CSRC, ROOT)})
    names = git("ls-tree", "-r", "--name-only", commit, "--", *dirs).decode().split("\n")
    for name in names:
        if name == rel or name.endswith((".h", ".hpp", ".inc")):
            path = os.path.join(dst, name)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "wb") as f:
                f.write(git("show", f"{commit}:{name}"))


def compile_asm(root, rel, asm):
    """-> (assembly text, remarks text) of root/rel: build.compile_cmd's command, device-only, to assembly."""
    cmd = build.compile_cmd(os.path.join(ROOT, rel), asm)
    cmd[cmd.index("-c")] = "-S"
    cmd = [root + a[len(ROOT):] if a.startswith(ROOT + os.sep) else a for a in cmd]  # sources and -I of that side
    cmd += ["--offload-device-only", "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode:
        sys.exit(f"{' '.join(cmd)}\n{p.stderr}\nkernel_isa_diff: compile failed")
    with open(asm) as f:
        return f.read(), p.stderr


def demangle(symbols):
    filt = os.path.join(os.path.dirname(os.path.realpath(build.HIPCC)), "..", "llvm", "bin", "llvm-cxxfilt")
    filt = filt if os.path.exists(filt) else "c++filt"
    out = subprocess.run([filt], input="\n".join(symbols), stdout=subprocess.PIPE, text=True, check=True).stdout
    return dict(zip(symbols, out.split("\n")))


def short_name(demangled):
    """'void k<true>(float const*, int)' -> 'k<true>'"""
    s = demangled[:demangled.index("(")] if "(" in demangled else demangled
    return s.split(" ", 1)[1] if s.startswith("void ") else s


def functions(asm):
    """-> {short demangled name: [instruction lines]}"""
    symbols = re.findall(r"^\s*\.type\s+(\S+),@function", asm, re.M)
    names = demangle(symbols)
    lines = asm.split("\n")
    out = {}
    for sym in symbols:
        start = next(i for i, l in enumerate(lines) if l.split(";")[0].strip() == sym + ":")
        body = []
        for line in lines[start + 1:]:
            code = line.split(";")[0].strip()
            if code.startswith(".Lfunc_end"):
                break
            if not code or (code.startswith(".") and not code.endswith(":")):  # comment, blank or directive
                continue
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", code))
        out[short_name(names[sym])] = body
    return out


def resources(remarks):
    """-> {short demangled name: 'VGPRs 125, SGPRs 106, ...'} from -Rpass-analysis=kernel-resource-usage"""
    blocks = re.split(r"remark: [^\n]*Function Name: ", remarks)[1:]
    names = demangle([b.split()[0] for b in blocks])
    out = {}
    for b in blocks:
        found = dict(re.findall(r"remark:\s+([A-Za-z][^:\n]*): (\d+)", b))
        out[short_name(names[b.split()[0]])] = ", ".join(f"{k.split(' [')[0]} {found[k]}" for k in RESOURCES if k in found)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("commit")
    ap.add_argument("file", help="a .hip file, path relative to the repository root")
    ap.add_argument("pairs", nargs="+", metavar="OLD=NEW")
    ap.add_argument("--max-diff-lines", type=int, default=80)
    args = ap.parse_args()
    rel = os.path.relpath(os.path.abspath(args.file), ROOT)
    commit = git("rev-parse", "--short", args.commit).decode().strip()
    with tempfile.TemporaryDirectory() as tmp:
        old_root = os.path.join(tmp, "old")
        checkout(args.commit, rel, old_root)
        old_asm, old_rem = compile_asm(old_root, rel, os.path.join(tmp, "old.s"))
        new_asm, new_rem = compile_asm(ROOT, rel, os.path.join(tmp, "new.s"))
    old_fn, new_fn = functions(old_asm), functions(new_asm)
    old_res, new_res = resources(old_rem), resources(new_rem)
    print(f"{rel}: {commit} against the work tree")
    flags = [a for a in build.compile_cmd(os.path.join(ROOT, rel), "OUT")[1:] if ROOT not in a and a not in ("-c", "-o", "OUT", "-I")]
    print("flags: " + " ".join(flags) + " (-S --offload-device-only in place of -c)")
    differ = 0
    for pair in args.pairs:
        old, _, new = pair.partition("=")
        new = new or old
        for name, fns, side in ((old, old_fn, commit), (new, new_fn, "work tree")):
            if name not in fns:
                sys.exit(f"kernel_isa_diff: no kernel {name!r} in {side}; it has: {', '.join(sorted(fns))}")
        a, b = old_fn[old], new_fn[new]
        print(f"\n{old} ({commit}) -> {new} (work tree)")
        for side, body, res in (("old", a, old_res.get(old)), ("new", b, new_res.get(new))):
            print(f"  {side}: {sum(not l.endswith(':') for l in body)} instructions; {res or 'no resource remarks'}")
        if a == b:
            print("  IDENTICAL")
            continue
        differ += 1
        diff = list(difflib.unified_diff(a, b, old, new, n=2, lineterm=""))
        ca, cb = (collections.Counter(l.split()[0] for l in body if not l.endswith(":")) for body in (a, b))
        print("  DIFFERENT; mnemonics whose count changed: " +
              (", ".join(f"{m} {ca[m]} -> {cb[m]}" for m in sorted(set(ca) | set(cb)) if ca[m] != cb[m]) or "none"))
        print("\n".join("  " + l for l in diff[:args.max_diff_lines]))
        if len(diff) > args.max_diff_lines:
            print(f"  ... ({len(diff) - args.max_diff_lines} more diff lines)")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
