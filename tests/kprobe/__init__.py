"""ctypes loader of lib/libvs_kprobe.so (tests/kprobe/vs_kprobe.cpp: C entry
points over the vsk:: launchers of csrc/vs_kernels.h), for the stage-level
GPU tests. build.py builds the library; nothing is compiled here.

    kp = kprobe.load()
    kp.check(kp.q8_absmax(X.data_ptr(), 0, X.numel(), glob.data_ptr()))

Every pointer argument is a device address (a torch tensor's data_ptr(), 0 =
null); launches go to stream 0 and the caller runs torch.cuda.synchronize().
"""
import ctypes
import os

_lib = None

u32, u64, i32, f64 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_double
pu32 = ctypes.POINTER(ctypes.c_uint32)

_CONSTS64 = ["q8_glob_bytes", "q8_spec_stat_off", "q8_spec_k_off", "q8_spec_k_size",
             "q8_spec_k_count", "q8_spec_stat_size", "spec_k_ratio_off", "spec_k_backoff_off",
             "spec_k_loose_off", "spec_k_since_off", "spec_stat_tries_off", "spec_stat_fails_off",
             "spec_stat_skipped_off", "q8_par_bytes", "rsel_state_size", "rsel_state_thr_off",
             "rsel_state_krem_off", "rsel_state_done_off", "rsel_state_count_off"]
_CONSTS32 = ["gate_verdict", "gate_forced", "gate_go", "q8_spec_probe", "q8_spec_max_backoff",
             "mfma_query_slots", "mfma_max_k", "mfma_max_cand_cap", "rsel_bins", "max_k",
             "gemv_small_arg_dim", "gemv_small_max_rows", "gemv_small_max_k", "gemv_small_max_parts"]
_SIGS = {
    "device_cu_count": (u32, []),
    "gemv_scores": (i32, [u64, i32, u32, u32, u64, u64, u64, u64]),
    "gemv": (i32, [u64, i32, u32, u32, u32, u64, u32, u64, u32, pu32, u64]),
    "gemv_gather": (i32, [u64, i32, u32, u32, u32, u64, u32, u64, u32, pu32, u64]),
    "compact_scratch_words": (u32, [u32]),
    "compact_rows": (i32, [u64, u32, u64, u64]),
    "gemv_small_ok": (i32, [u32, u32, u32]),
    "gemv_small_parts": (u32, [u32, i32, u32]),
    "gemv_one_ok": (i32, [u32, u32]),
    "gemv_small": (i32, [u64, i32, u32, u32, u32, u64, i32, u32, u64, u64, u64, u64]),
    "gemv_one_host": (i32, [u64, i32, u32, u32, u32, u64, i32, u64, u32, u64, u32, pu32]),
    "rsel": (i32, [u64, u32, u32, u32, u64, u64, u64]),
    "rsel_fused": (i32, [u64, u32, u32, u32, u64, u64, u64, u64, u64]),
    "sort_keys_temp_bytes": (u64, [u64]),
    "sort_keys_desc": (i32, [u64, u64, u64, u64, u64]),
    "merge_large_scratch": (u64, [u32, u32, u32]),
    "merge_large": (i32, [u64, u32, u64, u64, u32, u32, u32, u64, u64, u64]),
    "remap_keys": (i32, [u64, u64, u32, u32, u32]),
    "mfma_grid": (None, [u32, pu32, pu32]),
    "mfma_max_lists": (u32, [u32]),
    "mfma_tiles_per_wg": (u32, [u32]),
    "mfma_sample_tiles": (u32, [u32, u32, i32]),
    "mfma_cand_cap": (u32, [u32, u32, u32, f64]),
    "mfma_queries": (u32, [u32, i32]),
    "mfma_supported": (i32, [u32, i32]),
    "q8_supported": (i32, [u32, i32]),
    "sample_bound_passes": (i32, []),
    "q8_absmax": (i32, [u64, i32, u64, u64]),
    "q8_set_scale": (i32, [u64]),
    "q8_quantize": (i32, [u64, i32, u32, u32, u64, u32, u32, u64, u64, u64]),
    "query_prep": (i32, [u64, u32, u32, i32, i32, u64, u64]),
    "q8_query": (i32, [u64, i32, u32, u32, u64, u64, u64, u64]),
    "q8_query_spec": (i32, [u64, i32, u32, u32, u64, u64, u64, u64, u64, u64, u64, u64, i32]),
    "q8_prep_query": (i32, [u64, i32, i32, u64, u64, i32, u32, u32, u64, u64, u64, u64, u64, u64,
                            u64, u64, i32]),
    "sample_bound_q8": (i32, [u64, u32, u32, u32, u64, u64, i32, u32, u32, u64, u64, u64, u64]),
    "mfma_sample": (i32, [u64, i32, u32, u32, u32, u64, u32, u32, u32, u64, u32, pu32, u64]),
    "sample_bound": (i32, [u64, u32, u32, u32, u64]),
    "mfma_cand": (i32, [u64, i32, u32, u32, u32, u64, u32, u32, u64, u64, u64, u32, u64, u32, pu32,
                        u64, u64]),
    "select_slabs": (i32, [u64, u64, u64, u32, u32, u32, u32, u64, u32, u64, u64]),
    "mfma_cand_q8": (i32, [u64, u32, u32, u32, u64, u32, u32, u64, u64, u64, u64, u64, u32, u64,
                           u64, u32, pu32, u64, u64]),
    "select_q8": (i32, [u64, u64, u64, u64, u32, u32, u32, u32, u64, u32, u64, u64, i32, u32, u64,
                        u64, u64, u64, u64, u64, u64, u32, i32, u64, u64, u64, u64, u64, u64]),
    "q8_verify_record": (i32, [u64, u32, u32, u32, u64, u64, u64, i32, u64, u64, u64, u64]),
    "gemv_max_lists": (u32, [u32, i32, u32, u32]),
    "gemv_one": (i32, [u64, i32, u32, u32, u32, u64, i32, u64, u32, u64, u32, pu32]),
    "merge": (i32, [u64, u32, u64, u64, u32, u32, u32, u64]),
    "gemv_q8_lists": (u32, [u32]),
    "gemv_q8_scratch_bytes": (u64, [u32, u32]),
    "gemv_q8_ulist_off": (u64, [u32, u32]),
    "gemv_q8_lbest_off": (u64, [u32, u32]),
    "gemv_q8_cand_off": (u64, [u32, u32]),
    "gemv_q8_kp": (u32, [u32, u32]),
    "gemv_q8": (i32, [i32, u64, i32, u64, u64, u64, u32, u32, u32, u64, i32, u64, u32, u64, u64, u64,
                      u64, u64]),
}


class KProbe:
    """The shim's functions without their kp_ prefix, and its constants as ints."""

    def __init__(self, lib):
        self._lib = lib
        for name in _CONSTS64 + _CONSTS32:
            fn = getattr(lib, "kp_" + name)
            fn.restype, fn.argtypes = (u64 if name in _CONSTS64 else u32), []
            setattr(self, name, int(fn()))
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, "kp_" + name)
            fn.restype, fn.argtypes = res, args
            setattr(self, name, fn)

    @staticmethod
    def check(err):
        assert err == 0, f"launcher returned hipError_t {err}"

    def grid(self, n_rows):
        """(workgroups, rows per workgroup) of the MFMA passes at n_rows."""
        a, b = u32(0), u32(0)
        self._lib.kp_mfma_grid(n_rows, ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value


def load():
    """Loads the product library through the package first (so the HIP runtime
    bound is torch's), then the shim beside it."""
    global _lib
    if _lib is None:
        import __graft_entry__ as ge
        ge.load_package().load_library()
        path = os.path.join(ge.PKG_DIR, "lib", "libvs_kprobe.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} not found: run __graft_entry__.build() first")
        _lib = KProbe(ctypes.CDLL(path))
    return _lib
