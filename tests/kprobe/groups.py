"""ctypes loader of lib/libvs_kprobe_groups.so (tests/kprobe/vs_kprobe_groups.cpp:
the grouped-search launchers of csrc/vs_group.hip and launch_merge), for
tests/test_groups_stages_gpu.py. build.py builds the library; nothing is
compiled here. Pointers are device addresses, launches go to stream 0.
"""
import ctypes
import os

u32, u64, i32 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int

_CONSTS = ["group_none", "max_limit", "max_size", "max_lists", "rsel_bins"]
_SIGS = {
    "group_lists": (u32, [u32]),
    "group_best": (i32, [u64, u64, u32, u32, u32, u64, u64]),
    "group_heads": (i32, [u64, u64, u64, u32, u32, u32, u32, u64]),
    "group_members": (i32, [u64, u64, u64, u32, u32, u32, u64, u32, u32, u64, u64]),
    "group_clear": (i32, [u64, u32]),
    "merge": (i32, [u64, u32, u64, u64, u32, u32, u32, u64]),
}

_lib = None


class GroupsProbe:
    """The shim's functions without their kpg_ prefix, and its constants as ints."""

    def __init__(self, lib):
        self._lib = lib
        for name in _CONSTS:
            fn = getattr(lib, "kpg_" + name)
            fn.restype, fn.argtypes = u32, []
            setattr(self, name, int(fn()))
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, "kpg_" + name)
            fn.restype, fn.argtypes = res, args
            setattr(self, name, fn)

    @staticmethod
    def check(err):
        assert err == 0, f"launcher returned hipError_t {err}"


def load():
    """The product library through the package first (so the HIP runtime bound
    is torch's), then the shim beside it."""
    global _lib
    if _lib is None:
        import __graft_entry__ as ge
        ge.load_package().load_library()
        path = os.path.join(ge.PKG_DIR, "lib", "libvs_kprobe_groups.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} not found: run __graft_entry__.build() first")
        _lib = GroupsProbe(ctypes.CDLL(path))
    return _lib
