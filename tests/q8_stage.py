"""Device buffers and launch sequences shared by the stage-level GPU tests
(tests/test_q8_stages_gpu.py, tests/test_spec_verify_gpu.py): a collection
with its int8 copy, a batch of queries with its int8 images, and the bf16 /
f32 reference pass and the int8 pass + select, each one launcher call through
tests/kprobe. Buffers are sized as the engine sizes them (whole 32-row tiles,
kMfmaQueries query slots); every read-back is numpy.
"""
import ctypes

import numpy as np

import q8_ref as R

INT_MIN = -2 ** 31
DEV = "cuda:0"


# ---- result keys (include/vsearch.h "Result key layout") ---------------------
def make_keys(s, rows):
    s = np.array(s, np.float32, ndmin=1)
    s[s == 0] = 0.0  # -0.0 ranks as +0.0
    u = s.view(np.uint32).astype(np.uint64)
    o = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000).astype(np.uint64)
    return (o << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(rows, np.uint64))


def key_scores(keys):
    o = (np.asarray(keys, np.uint64) >> np.uint64(32)).astype(np.uint64)
    u = np.where(o & 0x80000000, o & 0x7FFFFFFF, ~o & 0xFFFFFFFF).astype(np.uint32)
    return u.view(np.float32)


def key_rows(keys):
    return (np.uint64(0xFFFFFFFF) - (np.asarray(keys, np.uint64) & np.uint64(0xFFFFFFFF))).astype(np.int64)


def pack_allow(mask, words):
    """bool mask of local rows -> uint64 bitmap of `words` words (bit r of word r / 64)."""
    bits = np.zeros(words * 64, np.uint8)
    bits[:len(mask)] = mask
    return np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").ravel().view(np.uint64).copy()


def _to_dev(torch, a, f32):
    a = np.ascontiguousarray(a, np.float32)
    if f32:
        return torch.from_numpy(a).to(DEV)
    return torch.from_numpy(R.bf16_bits(a).view(np.int16)).to(DEV)


def _i64(torch, a_u64):
    return torch.from_numpy(np.ascontiguousarray(a_u64, np.uint64).view(np.int64)).to(DEV)


class Collection:
    """Rows X (fp32 values; bf16-representable unless f32) on the device with
    their int8 copy. X0: the rows the scale is computed from (a stale S)."""

    def __init__(self, kp, torch, X, f32, X0=None, row_base=0, poison_pad=False):
        self.kp, self.torch, self.f32, self.row_base = kp, torch, f32, row_base
        self.n, self.dim = X.shape
        self.tiles = (self.n + 31) // 32
        self.pad = self.tiles * 32
        self.X = np.ascontiguousarray(X, np.float32)
        # (two spare tiles behind the last one, which no launch should touch)
        self.Xd = torch.zeros((self.pad + 64, self.dim), dtype=torch.float32 if f32 else torch.int16, device=DEV)
        self.X8d = torch.full((self.pad + 64, self.dim), 0x55, dtype=torch.int8, device=DEV)
        self.meta = torch.full((self.tiles + 2, 2), -1.0, dtype=torch.float32, device=DEV)
        self.glob = torch.zeros(kp.q8_glob_bytes, dtype=torch.uint8, device=DEV)
        if poison_pad:  # dead rows of the last tile: nothing may read them
            self.Xd[self.n:self.pad] = _to_dev(torch, np.full((self.pad - self.n, self.dim), 3.0, np.float32), f32)
        self.upload(X if X0 is None else X0)
        self.fix_scale()
        if X0 is not None:
            self.upload(X)
        self.quantize()

    def upload(self, X, rows=None):
        d = _to_dev(self.torch, X, self.f32)
        if rows is None:
            self.Xd[:len(X)] = d
        else:
            self.Xd[self.torch.as_tensor(rows, device=DEV)] = d

    def fix_scale(self):
        kp = self.kp
        self.glob[:16] = 0
        kp.check(kp.q8_absmax(self.Xd.data_ptr(), int(self.f32), self.n * self.dim, self.glob.data_ptr()))
        kp.check(kp.q8_set_scale(self.glob.data_ptr()))

    def quantize(self, tiles=None):
        kp = self.kp
        if tiles is None:
            kp.check(kp.q8_quantize(self.Xd.data_ptr(), int(self.f32), self.n, self.dim, 0, 0, self.tiles,
                                    self.X8d.data_ptr(), self.meta.data_ptr(), self.glob.data_ptr()))
        else:
            t = self.torch.as_tensor(np.asarray(tiles, np.int32), device=DEV)
            kp.check(kp.q8_quantize(self.Xd.data_ptr(), int(self.f32), self.n, self.dim, t.data_ptr(), 0,
                                    len(tiles), self.X8d.data_ptr(), self.meta.data_ptr(),
                                    self.glob.data_ptr()))
            self.torch.cuda.synchronize()  # t outlives the launch

    def read(self):
        """-> (x8 int8 [pad, dim], meta fp32 [tiles, 2], glob fp32 [4])."""
        self.torch.cuda.synchronize()
        x8 = self.X8d.cpu().numpy()
        meta = self.meta.cpu().numpy()
        assert np.all(x8[self.pad:] == 0x55) and np.all(meta[self.tiles:] == -1.0), "wrote past the last tile"
        return x8[:self.pad], meta[:self.tiles], self.glob[:16].cpu().numpy().view(np.float32).copy()


class Queries:
    """A batch's queries Q (fp32 values, in the collection's dtype on the
    device: kMfmaQueries zero-padded slots), their int8 images and q8par."""

    def __init__(self, kp, torch, Q, f32):
        self.kp, self.torch, self.f32 = kp, torch, f32
        self.nq, self.dim = Q.shape
        self.Q = np.ascontiguousarray(Q, np.float32)
        slots = kp.mfma_query_slots
        self.Qd = torch.zeros((slots, self.dim), dtype=torch.float32 if f32 else torch.int16, device=DEV)
        self.Qd[:self.nq] = _to_dev(torch, Q, f32)
        self.q8 = torch.full((slots, self.dim), 0x55, dtype=torch.int8, device=DEV)
        self.par = torch.full((kp.q8_par_bytes // 4,), -7.0, dtype=torch.float32, device=DEV)
        self.gate = self.par[4 * slots:4 * slots + 16].view(torch.int32)
        self.gate[:] = 0x5A5A
        # the verify hand-over (one float4 a query) and its ticket, zero between launches
        self.vq_ptr = self.par.data_ptr() + 16 * slots + 64
        self.ticket_ptr = self.vq_ptr + 16 * slots
        self.par[4 * slots + 16:] = 0

    def quantize(self, coll):
        kp = self.kp
        kp.check(kp.q8_query(self.Qd.data_ptr(), int(self.f32), self.nq, self.dim, coll.glob.data_ptr(),
                             self.q8.data_ptr(), self.par.data_ptr(), self.gate.data_ptr()))
        return self

    def read(self):
        """-> (q8 int8 [nq, dim], par fp32 [nq, 4], gate words)."""
        self.torch.cuda.synchronize()
        return (self.q8[:self.nq].cpu().numpy(), self.par[:4 * self.nq].cpu().numpy().reshape(-1, 4),
                self.gate.cpu().numpy())


class Slabs:
    """The candidate buffers of one main pass at (workgroups, cap)."""

    def __init__(self, kp, torch, nwg, cap):
        slots = kp.mfma_query_slots
        self.nwg, self.cap, self.slots = nwg, cap, slots
        self.slabs = torch.zeros((nwg, slots, cap, 8), dtype=torch.int32, device=DEV)
        self.tile = torch.zeros((nwg, slots, cap), dtype=torch.int32, device=DEV)
        self.cnt = torch.zeros(nwg * slots * 4, dtype=torch.int32, device=DEV)
        self.cmx = torch.zeros(nwg * slots * 4, dtype=torch.int32, device=DEV)

    def decode(self, nq, i8):
        """Every admitted slab's rows and values for queries < nq ->
        (query [m], global row [m], value [m]) over the 8 entries of each slab.
        A slab's rows are tile + 16 (b >> 2) + 4 kq + (b & 3), kq its quarter;
        counts are [query][wg][4] after the int8 pass, [wg][query][4] after
        the bf16 / f32 pass."""
        nwg, cap, sub = self.nwg, self.cap, self.cap // 4
        cnt = self.cnt.cpu().numpy().view(np.uint32)
        if i8:
            cnt = cnt[:nq * nwg * 4].reshape(nq, nwg, 4).transpose(1, 0, 2)
        else:
            cnt = cnt.reshape(nwg, self.slots, 4)[:, :nq]
        sl = self.slabs[:, :nq].cpu().numpy().reshape(nwg, nq, 4, sub, 8)
        tl = self.tile[:, :nq].cpu().numpy().view(np.uint32).reshape(nwg, nq, 4, sub)
        assert cnt.max(initial=0) <= sub, "a quarter overflowed: the test's cap is too small"
        live = np.arange(sub)[None, None, None, :] < cnt[..., None]
        b = np.arange(8)
        kq = np.arange(4)[None, None, :, None, None]
        rows = tl[..., None].astype(np.int64) + (16 * (b >> 2) + (b & 3)) + 4 * kq
        qq = np.broadcast_to(np.arange(nq)[None, :, None, None, None], rows.shape)
        m = np.broadcast_to(live[..., None], rows.shape)
        vals = sl if i8 else sl.view(np.float32)
        return qq[m], rows[m], vals[m]


def cap_for(kp, n_rows, k=1):
    """A capacity no quarter can overflow: one slab a tile, and >= 4 k."""
    cap = max(64, 4 * kp.mfma_tiles_per_wg(n_rows), 4 * k)
    cap = (cap + 3) // 4 * 4
    assert cap <= kp.mfma_max_cand_cap
    return cap


def neg_inf(torch, n=256):
    return torch.full((n,), float("-inf"), dtype=torch.float32, device=DEV)


def ref_pass(kp, torch, coll, qs, k, cap=None, allow=None, select=True):
    """The bf16 / f32 pass with a -inf bound -> (keys [nq, k] or None, Slabs)."""
    cap = cap or cap_for(kp, coll.n, k)
    nwg = kp.mfma_max_lists(coll.n)
    S = Slabs(kp, torch, nwg, cap)
    nl = ctypes.c_uint32(0)
    ninf = neg_inf(torch)
    ap = allow.data_ptr() if allow is not None else 0
    kp.check(kp.mfma_cand(coll.Xd.data_ptr(), int(coll.f32), coll.dim, coll.n, coll.row_base,
                          qs.Qd.data_ptr(), qs.nq, k, ninf.data_ptr(), S.slabs.data_ptr(),
                          S.tile.data_ptr(), cap, S.cnt.data_ptr(), nwg, ctypes.byref(nl), ap, 0))
    assert nl.value == nwg
    keys = None
    if select:
        out = torch.full((qs.nq, k), -1, dtype=torch.int64, device=DEV)
        kp.check(kp.select_slabs(S.slabs.data_ptr(), S.tile.data_ptr(), S.cnt.data_ptr(), nwg, cap, qs.nq,
                                 k, out.data_ptr(), coll.row_base, ap, 0))
        torch.cuda.synchronize()
        keys = out.cpu().numpy().view(np.uint64)
    torch.cuda.synchronize()
    return keys, S


def q8_pass(kp, torch, coll, qs, k, bound=None, cap=None, allow=None):
    """The int8 pass (qs quantised against coll) -> Slabs. bound: a device
    tensor of per-query bounds, None = no bound (init_score null)."""
    cap = cap or cap_for(kp, coll.n, k)
    nwg = kp.mfma_max_lists(coll.n)
    S = Slabs(kp, torch, nwg, cap)
    nl = ctypes.c_uint32(0)
    kp.check(kp.mfma_cand_q8(coll.X8d.data_ptr(), coll.dim, coll.n, coll.row_base, qs.q8.data_ptr(), qs.nq,
                             k, bound.data_ptr() if bound is not None else 0, qs.par.data_ptr(),
                             coll.glob.data_ptr(), S.slabs.data_ptr(), S.tile.data_ptr(), cap,
                             S.cnt.data_ptr(), S.cmx.data_ptr(), nwg, ctypes.byref(nl), qs.gate.data_ptr(),
                             allow.data_ptr() if allow is not None else 0))
    assert nl.value == nwg
    torch.cuda.synchronize()
    return S


def q8_select(kp, torch, coll, qs, S, k, bound, allow=None, verify=None):
    """The int8 select over S -> keys [nq, k]. verify: (check, spec_k ptr, stat
    ptr, advice ptr, vq ptr, ticket ptr) for the check by the last workgroup."""
    out = torch.full((qs.nq, k), -1, dtype=torch.int64, device=DEV)
    v = verify or (0, 0, 0, 0, 0, 0)
    kp.check(kp.select_q8(S.slabs.data_ptr(), S.tile.data_ptr(), S.cnt.data_ptr(), S.cmx.data_ptr(), S.nwg,
                          S.cap, qs.nq, k, out.data_ptr(), coll.row_base, coll.Xd.data_ptr(),
                          qs.Qd.data_ptr(), int(coll.f32), coll.dim, qs.par.data_ptr(), coll.glob.data_ptr(),
                          coll.meta.data_ptr(), bound.data_ptr(), coll.X8d.data_ptr(), qs.q8.data_ptr(),
                          allow.data_ptr() if allow is not None else 0, coll.n, v[0], qs.gate.data_ptr(),
                          v[1], v[2], v[3], v[4], v[5]))
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64)


def interesting_rows(kp):
    """Row counts (a) under one tile, (b) one workgroup's ragged tile, a few
    one-tile workgroups, and (c) the smallest count at which several workgroups
    run with unequal tile counts and a partial last tile -- found by asking
    mfma_grid, which depends on the device's CU count."""
    def tiles_of(n):
        nwg, rpw = kp.grid(n)
        return nwg, [(min(n, (w + 1) * rpw) - w * rpw + 31) // 32 for w in range(nwg)]

    c = None
    n = 33
    while c is None and n < 200_000:
        if n % 32:
            nwg, t = tiles_of(n)
            if nwg > 1 and len(set(t)) > 1:
                c = n
        n += 1
    assert c is not None
    nwg, rpw = kp.grid(29)
    assert nwg == 1
    return dict(a=5, b=29, few=101, c=c)
