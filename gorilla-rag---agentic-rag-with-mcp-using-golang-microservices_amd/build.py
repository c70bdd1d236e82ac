"""Builds lib/libvsearch.so in-tree with hipcc for gfx950.

The .so is git-ignored but travels to the GPU box with the repo snapshot.

Provenance is by content, not mtime: every object is rebuilt when the hash of
its inputs (sources, headers, flags) differs from the hash recorded beside it,
and the library exports `vs_build_id()` = `tree_hash()` of the sources it was
linked from (csrc/**, include/*.h, this file). smoke() and bench.py print the
id of the library they loaded, and smoke() fails when it differs from the
hash of the tree it runs from.
"""
from __future__ import annotations

import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
BUILD = os.path.join(HERE, "build")
LIB = os.path.join(HERE, "lib", "libvsearch.so")
SVC_LIB = os.path.join(HERE, "lib", "libvsearch_service.so")
SVC_SOURCES = ["service/json.cpp", "service/vector_service.cpp", "service/batcher.cpp",
               "service/loadgen.cpp", "service/http.cpp"]
SVC_HEADERS = ["service/json.h", "service/batcher.h", "service/http.h"]
# the vector-service process (PORT, VS_DEVICES, ...; csrc/service/server_main.cpp)
SERVER = os.path.join(HERE, "lib", "vsearch_server")
ROOT = os.path.dirname(HERE)
# test-only C entry points over the vsk:: launchers (tests/kprobe/__init__.py loads
# it); beside the product libraries because lib/ is what travels with the tree,
# but no part of them: not in tree_files(), so not in the build id
KPROBE_SRC = os.path.join(ROOT, "tests", "kprobe", "vs_kprobe.cpp")
KPROBE_LIB = os.path.join(HERE, "lib", "libvs_kprobe.so")
# the int8 pass with its run_if word (tests/test_q8_split_wg_gpu.py), a shim of its own
KPROBE_RUNIF_SRC = os.path.join(ROOT, "tests", "kprobe", "vs_kprobe_runif.cpp")
KPROBE_RUNIF_LIB = os.path.join(HERE, "lib", "libvs_kprobe_runif.so")
# the grouped-search stages (tests/test_groups_stages_gpu.py), a shim of its own
KPROBE_GROUPS_SRC = os.path.join(ROOT, "tests", "kprobe", "vs_kprobe_groups.cpp")
KPROBE_GROUPS_LIB = os.path.join(HERE, "lib", "libvs_kprobe_groups.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("VS_OFFLOAD_ARCH", "gfx950")

SOURCES = {
    "vs_kernels.o": (["vs_kernels.hip"], ["--offload-arch=" + ARCH, "-O3"]),
    "vs_select.o": (["vs_select.hip"], ["--offload-arch=" + ARCH, "-O3"]),
    "vs_q8.o": (["vs_q8.hip"], ["--offload-arch=" + ARCH, "-O3"]),
    "vs_delete.o": (["vs_delete.hip"], ["--offload-arch=" + ARCH, "-O3"]),
    "vs_mmr.o": (["vs_mmr.hip"], ["--offload-arch=" + ARCH, "-O3"]),
    "vs_group.o": (["vs_group.hip"], ["--offload-arch=" + ARCH, "-O3"]),
    "vs_fuse.o": (["vs_fuse.hip"], ["--offload-arch=" + ARCH, "-O3"]),
    "vs_engine.o": (["vs_engine.cpp"], ["-O2", "-Wall"]),
    "vs_api.o": (["vs_api.cpp"], ["-O2", "-Wall"]),
}
# every object depends on every header beside the sources (r06: a listed
# subset left vs_bound_dev.h out, so an edit to it rebuilt vs_kernels.o but
# not vs_q8.o)
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".h"))
SRC_EXT = (".hip", ".cpp", ".h")


def tree_files():
    """The files whose content defines a build: csrc/** sources, include/*.h, build.py."""
    out = []
    for dp, dns, fns in os.walk(CSRC):
        dns.sort()
        for f in sorted(fns):
            if f.endswith(SRC_EXT):
                out.append(os.path.join(dp, f))
    inc = os.path.join(ROOT, "include")
    out += [os.path.join(inc, f) for f in sorted(os.listdir(inc)) if f.endswith(".h")]
    out.append(os.path.abspath(__file__))
    return out


def tree_hash() -> str:
    """sha256 over (path relative to the repo root, content) of tree_files(); 16 hex digits."""
    h = hashlib.sha256()
    for p in tree_files():
        h.update(os.path.relpath(p, ROOT).replace(os.sep, "/").encode() + b"\0")
        with open(p, "rb") as f:
            h.update(f.read())
        h.update(b"\0")
    return h.hexdigest()[:16]


def _inputs_hash(paths, cmd) -> str:
    h = hashlib.sha256("\0".join(cmd).encode())
    for p in paths:
        h.update(p.encode() + b"\0")
        if os.path.exists(p):
            with open(p, "rb") as f:
                h.update(f.read())
    return h.hexdigest()


def _run_if_changed(out, inputs, cmd, verbose, force) -> bool:
    """Runs `cmd` unless `out` exists and `out`.hash records the hash of (inputs, cmd)."""
    stamp = os.path.join(BUILD, os.path.basename(out) + ".hash")
    want = _inputs_hash(inputs, cmd)
    if not force and os.path.exists(out) and os.path.exists(stamp):
        with open(stamp) as f:
            if f.read().strip() == want:
                return False
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    with open(stamp, "w") as f:
        f.write(want + "\n")
    return True


def build(verbose: bool = False, force: bool = False) -> str:
    os.makedirs(BUILD, exist_ok=True)
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    hdrs = [os.path.join(CSRC, h) for h in HEADERS] + [os.path.join(ROOT, "include", "vsearch.h")]
    objs = []
    for obj, (srcs, flags) in SOURCES.items():
        out = os.path.join(BUILD, obj)
        src = os.path.join(CSRC, srcs[0])
        objs.append(out)
        cmd = [HIPCC, "-std=c++17", "-fPIC", *flags, "-c", src, "-o", out]
        _run_if_changed(out, [src] + hdrs, cmd, verbose, force)
    # the build id: one generated translation unit holding tree_hash()
    bid = tree_hash()
    bid_src = os.path.join(BUILD, "vs_build_id.cpp")
    text = ('// generated by build.py: tree_hash() of the sources this library is linked from\n'
            f'extern "C" const char* vs_build_id(void) {{ return "{bid}"; }}\n')
    if not os.path.exists(bid_src) or open(bid_src).read() != text:
        with open(bid_src, "w") as f:
            f.write(text)
    bid_obj = os.path.join(BUILD, "vs_build_id.o")
    _run_if_changed(bid_obj, [bid_src], [HIPCC, "-std=c++17", "-fPIC", "-O2", "-c", bid_src,
                                         "-o", bid_obj], verbose, force)
    objs.append(bid_obj)
    cmd = [HIPCC, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", LIB, *objs,
           "-L/opt/rocm/lib", "-lrccl", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-soname,libvsearch.so"]
    _run_if_changed(LIB, objs, cmd, verbose, force)
    # host-only service layer (the rag/vector-service handler mirror) over the C-ABI
    svc_srcs = [os.path.join(CSRC, x) for x in SVC_SOURCES]
    svc_hdrs = [os.path.join(CSRC, x) for x in SVC_HEADERS] + [
        os.path.join(ROOT, "include", "vsearch_service.h"), os.path.join(ROOT, "include", "vsearch.h")]
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-fPIC", "-Wall", "-shared",
           "-o", SVC_LIB, *svc_srcs, "-L" + os.path.dirname(LIB), "-lvsearch",
           "-pthread", "-Wl,-rpath,$ORIGIN", "-Wl,-soname,libvsearch_service.so"]
    _run_if_changed(SVC_LIB, svc_srcs + svc_hdrs + [LIB], cmd, verbose, force)
    main_src = os.path.join(CSRC, "service", "server_main.cpp")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-Wall", "-o", SERVER, main_src,
           "-L" + os.path.dirname(LIB), "-lvsearch_service", "-lvsearch", "-pthread",
           "-Wl,-rpath,$ORIGIN"]
    _run_if_changed(SERVER, [main_src, SVC_LIB] + svc_hdrs, cmd, verbose, force)
    if os.path.exists(KPROBE_SRC):
        cmd = [HIPCC, "-std=c++17", "-fPIC", "-O2", "-Wall", "-shared", "-I" + CSRC, KPROBE_SRC,
               "-o", KPROBE_LIB, "-L" + os.path.dirname(LIB), "-lvsearch", "-Wl,-rpath,$ORIGIN",
               "-Wl,-soname,libvs_kprobe.so"]
        _run_if_changed(KPROBE_LIB, [KPROBE_SRC, LIB] + hdrs, cmd, verbose, force)
    if os.path.exists(KPROBE_RUNIF_SRC):
        cmd = [HIPCC, "-std=c++17", "-fPIC", "-O2", "-Wall", "-shared", "-I" + CSRC, KPROBE_RUNIF_SRC,
               "-o", KPROBE_RUNIF_LIB, "-L" + os.path.dirname(LIB), "-lvsearch", "-Wl,-rpath,$ORIGIN",
               "-Wl,-soname,libvs_kprobe_runif.so"]
        _run_if_changed(KPROBE_RUNIF_LIB, [KPROBE_RUNIF_SRC, LIB] + hdrs, cmd, verbose, force)
    if os.path.exists(KPROBE_GROUPS_SRC):
        cmd = [HIPCC, "-std=c++17", "-fPIC", "-O2", "-Wall", "-shared", "-I" + CSRC, KPROBE_GROUPS_SRC,
               "-o", KPROBE_GROUPS_LIB, "-L" + os.path.dirname(LIB), "-lvsearch", "-Wl,-rpath,$ORIGIN",
               "-Wl,-soname,libvs_kprobe_groups.so"]
        _run_if_changed(KPROBE_GROUPS_LIB, [KPROBE_GROUPS_SRC, LIB] + hdrs, cmd, verbose, force)
    return LIB


if __name__ == "__main__":
    print(build(verbose=True, force="--force" in sys.argv))
