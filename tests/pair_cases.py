"""What the CPU and the GPU test of the pair stage (faqcs_pair_device, faqcs_render_pair_device) share: the catalogue of mate ids, the
random paired cases (two render_cases.Case, one per mate: own text, own defline spans, own arenas, own results), the host statements
(faqcs_pair_host, faqcs_render_pair_host) into sentinel-filled buffers, and the joined batch the paired rendering is held against."""
import ctypes as C

import numpy as np

import render_cases as rc
from faqcs_amd import _capi as capi
from faqcs_amd import driver

CANARY = rc.CANARY
FILES = (capi.FILE_QC1, capi.FILE_QC2, capi.FILE_UNPAIRED, capi.FILE_DISCARD)


def _long(n, seed):
    return bytes(((np.arange(n) * 7 + seed) % 26 + 97).astype(np.uint8))


def _flip(b, k):
    return b[:k] + bytes([b[k] ^ 1]) + b[k + 1:]


def matching():
    """(defline of mate 1, defline of mate 2) whose ids are equal"""
    c = [(b"", b""), (b"a", b"a"), (b"ab", b"ab"), (b"x/1", b"x/2"), (b"x.1", b"x/2"), (b"x/12", b"x/12"), (b"/1", b"/2"), (b"/1", b""), (b"a/1", b"a"),
         (b"a/1", b"a.2 other"), (b"@id comment/1", b"@id other comment/2"), (b"@id/1 comment/1", b"@id/2"), (b"@a\tb/1", b"@a\tb/2"),
         (b"@a\tb c", b"@a\tb d"), (b" ", b" x"), (b"1", b"1"), (b".1", b"/7"), (b"@r.1.2", b"@r.1/9"), (b"@r/a", b"@r/a extra")]
    for n in (15, 16, 17, 31, 32, 33, 300):
        x = _long(n, n)
        c += [(x, x), (x + b"/1", x + b"/2"), (x + b" one", x + b" two/2"), (x + b".1 c", x)]
    return c


def mismatching():
    """(defline of mate 1, defline of mate 2, id of mate 1, id of mate 2) whose ids differ"""
    c = [(b"", b"a"), (b"a", b"b"), (b"ab", b"a"), (b"x/12", b"x/13"), (b"x/12", b"x"), (b"/1", b"/"), (b"a/1", b"b/1"), (b"@a\tb", b"@a"), (b"@a\tb", b"@a b"),
         (b"@id x", b"@idx"), (b"1", b"2"), (b"@R20", b"@OTHER20"), (b"x.a", b"x/a")]
    for n in (15, 16, 17, 31, 32, 33, 300):
        x = _long(n, n + 1)
        c += [(x, _flip(x, 0)), (x, _flip(x, n - 1)), (x + b"/1", _flip(x, n - 1) + b"/2"), (x, x[:-1]), (x[: n // 2] + b" c", x), (x + b"y", x)]
    return [(a, b, driver.parse_id(a), driver.parse_id(b)) for a, b in c]


class PairCase:
    """Two mates, each a render_cases.Case of its own; deflines from the catalogue.  bad: indices of pairs that get mismatching ids."""

    def __init__(self, rng, n1, n2=None, bad=(), in_off=33, max_len=60, deflines=None, windows="random"):
        n2 = n1 if n2 is None else n2
        n = min(n1, n2)
        good, wrong = matching(), mismatching()
        r1, r2 = rc.random_reads(rng, n1, in_off, max_len=max_len), rc.random_reads(rng, n2, in_off, max_len=max_len)
        for i in range(n):
            if deflines is not None:
                a, b = deflines[i]
            elif i in bad:
                a, b = wrong[int(rng.integers(len(wrong)))][:2]
            else:
                a, b = good[int(rng.integers(len(good)))]
            if deflines is None and rng.random() < 0.5:
                a, b = b, a
            r1[i] = (a,) + r1[i][1:]
            r2[i] = (b,) + r2[i][1:]
        self.r1, self.r2 = r1, r2
        self.m = [rc.Case(rng, r1, windows=windows), rc.Case(rng, r2, windows=windows)]
        self.n = n

    def model_mates(self, with_res=True):
        return [dict(text=c.text, def_pos=c.def_pos, def_len=c.def_len, seq=c.seq, qual=c.qual, offset=c.offset, res=c.res if with_res else None) for c in self.m]


class HostMates:
    """capi.Mate x 2 of host pointers over a PairCase (keeps every array alive)."""

    def __init__(self, pc, with_res=(True, True)):
        self.keep, self.mates = [], []
        for c, wr in zip(pc.m, with_res):
            off = np.ascontiguousarray(c.offset, np.uint32)
            dpos, dlen = np.ascontiguousarray(c.def_pos, np.uint32), np.ascontiguousarray(c.def_len, np.uint32)
            b = capi.Batch(c.seq.ctypes.data, c.qual.ctypes.data, off.ctypes.data, c.n, 1, None, 0, None)
            m = capi.Mate(C.pointer(b), c.res.ctypes.data if wr else None, c.text.ctypes.data if len(c.text) else None, dpos.ctypes.data, dlen.ctypes.data)
            self.keep += [off, dpos, dlen, b, c]
            self.mates.append(m)


def info_dict(p):
    d = {f: int(getattr(p, f)) for f, _ in capi.PairInfo._fields_ if f != "id_len"}
    d["id_len"] = (int(p.id_len[0]), int(p.id_len[1]))
    return d


def pair_host(lib, pc, with_res=True, with_route=True):
    """One faqcs_pair_host with canaries around route -> (route or None, info dict)"""
    hm = HostMates(pc, (with_res, with_res))
    buf = np.full(64 + pc.n + 64, CANARY, np.uint8)
    info = capi.PairInfo(0xDEAD, 0xDEAD, 0xDEAD, 0xDEAD, (0xDEAD, 0xDEAD), 0xDEAD, 0xDEAD)
    rc_ = lib.faqcs_pair_host(C.byref(hm.mates[0]), C.byref(hm.mates[1]), buf[64:].ctypes.data if with_route else None, C.addressof(info))
    assert rc_ == 0, lib.faqcs_last_error()
    assert (buf[:64] == CANARY).all() and (buf[64 + pc.n:] == CANARY).all(), "bytes around route[0 .. n) were written"
    if not with_res:
        assert (buf == CANARY).all(), "check only: route was written"
    return (buf[64:64 + pc.n].copy() if with_res else None), info_dict(info)


def render_pair_host(lib, holder, pc, file, route, n_pairs, capacity=None, with_offset=True, with_index=True, with_res=(True, True)):
    """One faqcs_render_pair_host into sentinel-filled buffers; the WHOLE buffers come back, in the form of render_cases.render_host."""
    hm = HostMates(pc, with_res)
    nc = 2 * n_pairs
    cap = (len(pc.m[0].text) + len(pc.m[1].text) + 5 * nc) if capacity is None else capacity
    text = np.full(rc.FRONT + cap + 64, CANARY, np.uint8)
    shift = (-(text.ctypes.data + rc.FRONT)) % 16
    roff, ridx = np.full(nc + 2, rc.CAN32, np.uint32), np.full(nc + 1, rc.CAN32, np.uint32)
    info = capi.RenderInfo(0xDEAD, 0xDEAD, 0xDEAD)
    out = capi.RenderOut(text.ctypes.data + rc.FRONT + shift, cap, roff.ctypes.data if with_offset else None, ridx.ctypes.data if with_index else None,
                         C.addressof(info))
    route = np.ascontiguousarray(route, np.uint8)
    rc_ = lib.faqcs_render_pair_host(C.byref(holder.p), file, C.byref(hm.mates[0]), C.byref(hm.mates[1]), route.ctypes.data if n_pairs else None, n_pairs, C.byref(out))
    assert rc_ == 0, lib.faqcs_last_error()
    return {"text": text, "base": rc.FRONT + shift, "rec_offset": roff, "rec_index": ridx, "n_bytes": int(info.n_bytes), "n_reads": int(info.n_reads),
            "overflow": int(info.overflow), "with_offset": with_offset, "with_index": with_index, "exact": True}


def rendering(o):
    """(text, rec_offset, rec_index) of a rendering that fitted"""
    assert o["overflow"] == 0
    nb, nr = o["n_bytes"], o["n_reads"]
    return o["text"][o["base"]:o["base"] + nb].copy(), o["rec_offset"][:nr + 1].copy(), o["rec_index"][:nr].copy()


def joined_files(lib, holder, pc, route):
    """The four files from the EXISTING statement: faqcs_render_host on the joined batch (both mates in one batch, read i of mate 2 at m + i,
    text concatenated) with the masks and the interleave of render_cases.file_plans; pairs routed nowhere are masked out; rec_index mapped
    i -> 2 (i mod m) + (i >= m).  -> {file code: (text, rec_offset, rec_index)}"""
    m = pc.n
    r1, r2 = pc.r1[:m], pc.r2[:m]
    joined = rc.Case(np.random.default_rng(0), r1 + r2, windows=None)
    joined.res = np.concatenate([pc.m[0].res[:m], pc.m[1].res[:m]])
    valid = (joined.res["flags"] & capi.F_VALID) != 0
    v1, v2 = valid[:m], valid[m:]
    routed = np.asarray(route[:m]) != capi.ROUTE_NOWHERE
    inter = np.stack([np.arange(m), np.arange(m) + m], axis=1).ravel().astype(np.uint32)
    plans = rc.file_plans({"fastq": dict.fromkeys(capi.PAIR_FILES)}, m, True)
    out = {}
    for f in FILES:
        with_res, selfn, interleaved = plans[capi.PAIR_FILES[f]]
        sel = (selfn(v1, v2, lambda a, b: np.concatenate([a, b]), np.zeros(m, bool)) & np.concatenate([routed, routed])).astype(np.uint8)
        o = rc.render_host(lib, holder, joined, with_res, sel, inter if interleaved else None)
        text, roff, ridx = rendering(o)
        out[f] = (text, roff, (2 * (ridx % max(m, 1)) + (ridx >= m)).astype(np.uint32))
    return out
