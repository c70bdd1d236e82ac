"""Device buffers and launch sequences of the single-query int8 stage tests
(tests/test_q8_gemv_stages_gpu.py): launch_gemv_q8's scan and finish through
tests/kprobe on a q8_stage.Collection, every buffer the launcher writes with
poisoned guard words behind it, and the plain GEMV's keys (launch_gemv_one +
launch_merge) on the same device buffers. The scratch layout and the grid
come from the shim (gemv_q8_layout, gemv_q8_lists), never from here.
"""
import ctypes

import numpy as np

import q8_stage as St

GUARD = 64  # guard words behind every buffer
POISON64 = 0x5A5A5A5A5A5A5A5A
POISON32 = 0x5A5A5A5A


def query_dev(torch, q):
    """A raw fp32 query on the device (the launchers preprocess it)."""
    return torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(St.DEV)


def allow_dev(torch, mask, n):
    """bool mask of local rows -> (device bitmap, its pointer); None -> (None, 0)."""
    if mask is None:
        return None, 0
    t = St._i64(torch, St.pack_allow(np.asarray(mask[:n], bool), (n + 63) // 64))
    return t, t.data_ptr()


class Q8Gemv:
    """scratch / dst / ctr / stats of launch_gemv_q8 for one (collection, k)."""

    def __init__(self, kp, torch, coll, k):
        self.kp, self.torch, self.coll, self.k = kp, torch, coll, k
        n = coll.n
        self.nscan = kp.gemv_q8_lists(n)
        self.KP = kp.gemv_q8_kp(n, k)
        self.bytes = kp.gemv_q8_scratch_bytes(n, k)
        self.ul = kp.gemv_q8_ulist_off(n, k)
        self.lb = kp.gemv_q8_lbest_off(n, k)
        self.cd = kp.gemv_q8_cand_off(n, k)
        assert self.bytes % 8 == 0 and self.ul % 8 == 0 and self.lb % 4 == 0 and self.cd % 8 == 0
        assert self.ul + 8 * self.nscan * self.KP <= self.lb and self.lb + 4 * self.nscan <= self.cd < self.bytes
        self.scratch = torch.full((self.bytes // 8 + GUARD,), POISON64, dtype=torch.int64, device=St.DEV)
        self.dst = torch.full((k + GUARD,), POISON64, dtype=torch.int64, device=St.DEV)
        self.ctr = torch.full((2 + GUARD,), POISON32, dtype=torch.int32, device=St.DEV)
        self.stats = torch.full((2 + GUARD,), POISON32, dtype=torch.int32, device=St.DEV)
        self.ctr[:2] = 0
        self.stats[:2] = 0

    def launch(self, part, q, cosine, allow_ptr=0):
        kp, c = self.kp, self.coll
        kp.check(kp.gemv_q8(part, c.Xd.data_ptr(), int(not c.f32), c.X8d.data_ptr(), c.meta.data_ptr(),
                            c.glob.data_ptr(), c.dim, c.n, c.row_base, q.data_ptr(), int(cosine), allow_ptr,
                            self.k, self.scratch.data_ptr(), self.bytes, self.ctr.data_ptr(),
                            self.dst.data_ptr(), self.stats.data_ptr()))
        self.torch.cuda.synchronize()

    def _scratch(self):
        return self.scratch.cpu().numpy().view(np.uint64)

    def scan_out(self):
        """-> (ulist [nscan, KP] uint64, lbest [nscan] uint32)."""
        s = self._scratch()
        ul = s[self.ul // 8:self.ul // 8 + self.nscan * self.KP].reshape(self.nscan, self.KP).copy()
        lb = s.view(np.uint32)[self.lb // 4:self.lb // 4 + self.nscan].copy()
        return ul, lb

    def zero_cand(self):
        self.scratch[self.cd // 8:self.bytes // 8] = 0

    def cand(self):
        return self._scratch()[self.cd // 8:self.bytes // 8].copy()

    def keys(self):
        return self.dst[:self.k].cpu().numpy().view(np.uint64).copy()

    def counts(self):
        return tuple(int(x) for x in self.stats[:2].cpu().numpy().view(np.uint32))

    def check_guards(self):
        """Nothing written behind a buffer, and both counters back at 0."""
        assert np.all(self._scratch()[self.bytes // 8:] == POISON64), "wrote past the scratch"
        assert np.all(self.dst[self.k:].cpu().numpy().view(np.uint64) == POISON64), "wrote past dst[k]"
        ctr = self.ctr.cpu().numpy().view(np.uint32)
        assert np.all(ctr[2:] == POISON32), "wrote past ctr[2]"
        assert ctr[0] == 0 and ctr[1] == 0, ("ctr not left at zero", ctr[:2])
        assert np.all(self.stats[2:].cpu().numpy().view(np.uint32) == POISON32), "wrote past stats[2]"


def gemv_keys(kp, torch, coll, q, cosine, k, allow_ptr=0):
    """The plain GEMV's k keys for the raw query q (launch_gemv_one + launch_merge)."""
    bf16 = int(not coll.f32)
    maxl = kp.gemv_max_lists(coll.dim, bf16, coll.n, k)
    lists = torch.full((maxl * k + GUARD,), POISON64, dtype=torch.int64, device=St.DEV)
    out = torch.full((k + GUARD,), POISON64, dtype=torch.int64, device=St.DEV)
    nl = ctypes.c_uint32(0)
    kp.check(kp.gemv_one(coll.Xd.data_ptr(), bf16, coll.dim, coll.n, coll.row_base, q.data_ptr(), int(cosine),
                         allow_ptr, k, lists.data_ptr(), maxl, ctypes.byref(nl)))
    assert 1 <= nl.value <= maxl
    kp.check(kp.merge(lists.data_ptr(), nl.value, k, 0, 1, k, k, out.data_ptr()))
    torch.cuda.synchronize()
    assert np.all(lists[maxl * k:].cpu().numpy().view(np.uint64) == POISON64)
    o = out.cpu().numpy().view(np.uint64)
    assert np.all(o[k:] == POISON64)
    return o[:k].copy()
