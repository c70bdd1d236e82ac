#!/usr/bin/env python3
"""Which device functions differ between two builds of the library's objects (CPU only).

    python tools/isa_digest.py PARENT_BUILD_DIR CHANGE_BUILD_DIR [--rename REGEX=REPL] [OBJ ...]

For each object (default: the four HIP objects of build.py) the gfx950 code
object is taken out of both files, disassembled, and every `<symbol>:` block
is hashed without its address comments, keyed by the demangled name up to the
parameter list. The report lists the functions removed, added and changed,
counts the byte-identical ones, and gives VGPRs, LDS bytes and scratch bytes
of every kernel that is not identical; a changed function that differs in at
most 3 lines has them printed. --rename rewrites parent keys first, for
kernels whose template parameters changed.
"""
import difflib
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--" + os.environ.get("VS_OFFLOAD_ARCH", "gfx950")
OBJECTS = ["vs_kernels.o", "vs_select.o", "vs_q8.o", "vs_delete.o"]


def run(*cmd, **kw):
    return subprocess.run(cmd, check=True, capture_output=True, text=True, **kw).stdout


def key_of(demangled):
    """`void f<1, (X)2>(int*)` -> `f<1, (X)2>`: cut at the '(' outside every <>."""
    depth = 0
    for i, ch in enumerate(demangled):
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0 and i and demangled[i - 1] != "<":
            return demangled[:i].split(" ", 1)[-1] if demangled.startswith("void ") else demangled[:i]
    return demangled


def digest(obj, tmp):
    """{key: (sha of the block, vgprs, lds, scratch, its lines)} of one object's device code."""
    fat, co = os.path.join(tmp, "fat"), os.path.join(tmp, "co")
    run(f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat)
    run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", "--targets=" + TARGET,
        "--input=" + fat, "--output=" + co)
    dis = [f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co]
    head = re.compile(r"^(?:[0-9a-f]+ )?<(.+)>:$")
    blocks, name = {}, None
    for line in run(*dis).splitlines():
        m = head.match(line)
        if m:
            name = m.group(1)
            blocks[name] = []
        elif name and line.strip():
            blocks[name].append(line.split("//")[0].strip())
    # the same listing demangled: its symbol lines come in the same order
    plain = [m.group(1) for m in map(head.match, run(*dis, "--demangle").splitlines()) if m]
    res = {}
    notes = run(f"{LLVM}/llvm-readelf", "--notes", co)
    for k in notes.split("- .agpr_count:")[1:]:
        f = {m.group(1): m.group(2) for m in re.finditer(r"\.(\w+):\s+'?([^'\n]+)'?", k)}
        res[f["name"]] = (f["vgpr_count"], f["group_segment_fixed_size"],
                          f["private_segment_fixed_size"])
    assert len(plain) == len(blocks), obj
    return {key_of(d): (hashlib.sha256("\n".join(blocks[n]).encode()).hexdigest(),
                        *res.get(n, ("-", "-", "-")), blocks[n])
            for n, d in zip(blocks, plain)}


def main():
    args, renames = [], []
    it = iter(sys.argv[1:])
    for a in it:
        if a == "--rename":
            renames.append(next(it).split("=", 1))
        else:
            args.append(a)
    if len(args) < 2:
        sys.exit(__doc__)
    for obj in args[2:] or OBJECTS:
        with tempfile.TemporaryDirectory() as tmp:
            old = digest(os.path.join(args[0], obj), tmp)
            new = digest(os.path.join(args[1], obj), tmp)
        for pat, repl in renames:
            old = {re.sub(pat, repl, k): v for k, v in old.items()}
        removed = sorted(set(old) - set(new))
        added = sorted(set(new) - set(old))
        changed = sorted(k for k in set(old) & set(new) if old[k][0] != new[k][0])
        same = len(set(old) & set(new)) - len(changed)
        print(f"== {obj}: {len(old)} -> {len(new)} device functions; {same} byte-identical, "
              f"{len(changed)} changed, {len(removed)} removed, {len(added)} added")
        for title, ks in (("removed", removed), ("added", added)):
            for k in ks:
                v = (old if title == "removed" else new)[k]
                print(f"  {title}: {k}  vgpr {v[1]} lds {v[2]} scratch {v[3]}")
        for k in changed:
            o, n = old[k], new[k]
            print(f"  changed: {k}  vgpr {o[1]} -> {n[1]}  lds {o[2]} -> {n[2]}  "
                  f"scratch {o[3]} -> {n[3]}")
            d = [x for x in difflib.unified_diff(o[4], n[4], lineterm="", n=0)
                 if x[0] in "+-" and x[:3] not in ("+++", "---")]
            print(f"    {len(o[4])} -> {len(n[4])} lines" +
                  ("".join(f"\n    {x}" for x in d) if len(d) <= 6 else ""))


if __name__ == "__main__":
    main()
