#!/usr/bin/env python3
"""Did a source change alter what the compiler emits?  Builds csrc files from two trees and compares every kernel's instruction stream.
usage: tools/isa_diff.py OLD_TREE NEW_TREE FILE.hip [NEW_FILE.hip ...] [-v] [-- extra hipcc flags]          (needs hipcc, no GPU)
FILE.hip is built from the old tree; from the new tree the NEW_FILEs (FILE.hip itself where none is given).  Kernels are matched by name
(for an anonymous-namespace kernel the name does not depend on the file), so kernels that moved to another source file compare as
usual: `isa_diff.py old new gemm_tn.hip gemm_tn.hip gemm_tn_wide.hip`.

Both builds: hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only.  Comment lines, directives and the per-build __hip_cuid_*
symbol are dropped; what is left of a kernel (labels + instructions) is its stream.  One line per kernel:
  A  streams identical
  B  same opcode multiset and the same VGPR / AGPR / SGPR / scratch / LDS in the kernel metadata: instructions moved or registers renamed
  C  same metadata; opcode counts differ by at most 0.5 % of the kernel's instructions; the counts of v_mfma*, s_barrier, ds_*, global / flat /
     buffer loads and stores and scratch_* are unchanged (needs a timing)
  D  anything else, a kernel that exists in one build only included
followed by VGPR / AGPR / SGPR / scratch / LDS of the old build, and of the new one where they differ.  -v adds the opcode count differences.
Exit status 1 if any kernel is D."""
import collections
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
META = (("vgpr_count", "VGPR"), ("agpr_count", "AGPR"), ("sgpr_count", "SGPR"), ("private_segment_fixed_size", "scratch"),
        ("group_segment_fixed_size", "LDS"))
PINNED = ("v_mfma", "s_barrier", "ds_", "global_load", "global_store", "global_atomic", "flat_", "buffer_", "scratch_")     # class C: counts unchanged


def build(tree, name, flags, out):
    src = os.path.join(tree, "swin_v2_weather_amd", "csrc", name)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out, src] + flags,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        sys.exit("hipcc failed on %s:\n%s" % (src, r.stdout.decode()))
    return open(out).read().splitlines()


def kernels(lines):
    """{symbol: (stream, metadata)}: stream = the labels and instructions between `symbol:` and its .amdhsa_kernel block"""
    meta, cur = {}, None
    for l in lines[next((i for i, l in enumerate(lines) if l.startswith("amdhsa.kernels:")), len(lines)):]:
        if l.startswith("  - ."):              # a new kernel's entry (the entries of its .args list are indented further)
            cur = {}
        m = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)\s*$", l)
        if m and cur is not None:
            if m.group(1) == "name" and m.group(2).startswith("_Z"):
                meta[m.group(2)] = cur
            elif m.group(1) in dict(META):
                cur[m.group(1)] = int(m.group(2))
    out, name, body = {}, None, []
    for l in lines:
        if name is None:
            m = re.match(r"(_Z\w+):", l)
            if m and m.group(1) in meta:
                name, body = m.group(1), []
            continue
        s = l.split(";")[0].rstrip()
        if s.lstrip().startswith(".amdhsa_kernel") or s.lstrip().startswith(".Lfunc_end"):
            out[name] = (body, meta[name])
            name = None
        elif not s.strip() or "__hip_cuid_" in s:
            continue
        elif re.match(r"\.?\w+:$", s) or (s.startswith("\t") and not s.lstrip().startswith(".")):
            body.append(s)
    return out


def opcodes(stream):
    return collections.Counter(s.split()[0] for s in stream if s.startswith("\t"))


def classify(old, new):
    (so, mo), (sn, mn) = old, new
    if so == sn and mo == mn:
        return "A", {}
    co, cn = opcodes(so), opcodes(sn)
    delta = {k: cn[k] - co[k] for k in set(co) | set(cn) if cn[k] != co[k]}
    if mo != mn:
        return "D", delta
    if not delta:
        return "B", delta
    moved = sum(abs(v) for v in delta.values())
    if moved <= 0.005 * sum(co.values()) and not any(k.startswith(PINNED) for k in delta):
        return "C", delta
    return "D", delta


def main():
    args = sys.argv[1:]
    flags = []
    if "--" in args:
        i = args.index("--")
        args, flags = args[:i], args[i + 1:]
    verbose = "-v" in args
    args = [a for a in args if a != "-v"]
    if len(args) < 3:
        sys.exit(__doc__)
    new_files = args[3:] or [args[2]]
    with tempfile.TemporaryDirectory() as tmp:
        old = kernels(build(args[0], args[2], flags, os.path.join(tmp, "old.s")))
        new = {}
        for i, f in enumerate(new_files):
            ks = kernels(build(args[1], f, flags, os.path.join(tmp, "new%d.s" % i)))
            twice = sorted(set(ks) & set(new))
            if twice:
                sys.exit("kernel(s) in more than one new file: %s" % " ".join(twice))
            new.update(ks)
    names = list(old) + [n for n in new if n not in old]
    try:
        pretty = subprocess.run(["c++filt"] + names, stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    except (OSError, subprocess.CalledProcessError):
        pretty = names
    worst = "A"
    fmt = lambda m: " / ".join(str(m.get(k, "?")) for k, _ in META)
    print("%s %s: class  kernel  %s (old -> new where different)" % (args[2] if new_files == [args[2]] else "%s -> %s" % (args[2], " + ".join(new_files)), " ".join(flags), " / ".join(t for _, t in META)))
    for n, p in zip(names, pretty):
        p = re.sub(r"\((anonymous namespace)::\w+\)$|\(.*\)$", "", p.replace("(anonymous namespace)::", "")).replace("void ", "")
        if n not in old or n not in new:
            cls, delta, regs = "D", {}, "only in the %s build" % ("old" if n in old else "new")
        else:
            cls, delta = classify(old[n], new[n])
            regs = fmt(old[n][1]) + ("" if old[n][1] == new[n][1] else " -> " + fmt(new[n][1]))
            if cls != "A":
                regs += "   %d instructions, %d opcode counts moved" % (sum(opcodes(old[n][0]).values()), sum(abs(v) for v in delta.values()))
        worst = max(worst, cls)
        print("  %s  %-60s %s" % (cls, p, regs))
        if verbose and delta:
            print("       " + "  ".join("%s %+d" % kv for kv in sorted(delta.items())))
    print("%d kernels, worst class %s" % (len(names), worst))
    return 1 if worst == "D" else 0


if __name__ == "__main__":
    sys.exit(main())
