#!/usr/bin/env python3
"""Hashes of the gfx950 code object of smp_kernels.hip, to show that a change moved no machine code.

    tools/codeobj_sections.py <tree> [-DSWITCH ...] [--keep DIR]

<tree> is a checkout of this repository.  For the parent commit use a scratch worktree:
    git worktree add --detach /tmp/smp_parent HEAD~1 && tools/codeobj_sections.py /tmp/smp_parent
The device side is compiled alone with the Makefile's compiler and FLAGS (--offload-device-only -c), the
bundle is opened with clang-offload-bundler, and the sha256 and size of .text, .rodata and .note are
printed.  .note carries every kernel's register, scratch and LDS figures.  The __hip_cuid_<hash> symbol
differs between any two builds, and with it .dynsym, .dynstr and the hash tables; they are not compared.
No GPU is needed.
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

SECTIONS = (".text", ".rodata", ".note")
SRC = os.path.join("squirrel_motion_planner_amd", "csrc", "smp_kernels.hip")


def makefile_vars(tree):
    """HIPCC, ARCH and FLAGS as the Makefile sets them (EXTRA empty)."""
    text = open(os.path.join(tree, "squirrel_motion_planner_amd", "Makefile")).read()
    def var(name):
        m = re.search(r"^%s\s*\??=\s*(.*)$" % name, text, re.M)
        return m.group(1).strip() if m else ""
    flags = var("FLAGS").replace("$(EXTRA)", "").split()
    return os.environ.get("HIPCC", var("HIPCC")), os.environ.get("ARCH", var("ARCH")), flags


def sections(tree, defines, workdir):
    hipcc, arch, flags = makefile_vars(tree)
    bindir = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin")
    bundle = os.path.join(workdir, "smp_kernels.dev.o")
    elf = os.path.join(workdir, "smp_kernels.%s.elf" % arch)
    subprocess.check_call([hipcc, "--offload-arch=" + arch] + flags + list(defines) +
                          ["--offload-device-only", "-c", os.path.join(tree, SRC), "-o", bundle])
    subprocess.check_call([os.path.join(bindir, "clang-offload-bundler"), "--unbundle", "--type=o",
                           "--targets=hipv4-amdgcn-amd-amdhsa--" + arch, "--input=" + bundle, "--output=" + elf])
    out = {}
    for sec in SECTIONS:
        raw = os.path.join(workdir, "sec" + sec.replace(".", "_"))
        subprocess.check_call([os.path.join(bindir, "llvm-objcopy"), "--dump-section", "%s=%s" % (sec, raw), elf,
                               os.path.join(workdir, "discard.elf")])
        data = open(raw, "rb").read()
        out[sec] = (hashlib.sha256(data).hexdigest(), len(data))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree")
    ap.add_argument("--keep", metavar="DIR", help="leave the code object and the raw sections in DIR")
    args, defines = ap.parse_known_args()
    bad = [d for d in defines if not d.startswith("-D")]
    if bad:
        ap.error("only -D options are passed on: %s" % " ".join(bad))
    if args.keep:
        os.makedirs(args.keep, exist_ok=True)
        res = sections(args.tree, defines, args.keep)
    else:
        with tempfile.TemporaryDirectory() as tmp:
            res = sections(args.tree, defines, tmp)
    for sec in SECTIONS:
        print("%-8s %s %9d  %s" % (sec, res[sec][0], res[sec][1], " ".join(defines) or "default"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
