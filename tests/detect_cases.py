"""What the CPU and the GPU test of faqcs_detect_* / faqcs_first_error_* share: one constructed list of cases at every edge of the find-first
kernel (faqcs_amd/csrc/faqcs_detect_kernel.hip) -- the dword, the 16-byte vector, the tile, the two masked ends of the range, the finishing
block's loop --, the calls of the host statements, and the buffers with hostile bytes around everything a call may load but must not
interpret.

A quality arena is filled with 'A' .. 'J' (65 .. 74: undecided, trim.cpp:599-617) and a case plants decisive bytes in it: '~' and 'K' (above
74: offset 64), '!' and ':' (below 59: offset 33) and 0x80 / 0xff (negative as the reference's signed char: 33).  The 16 bytes in front of the
arena and the 64 behind it (the padding contract of faqcs_batch) are decisive throughout, in every case."""
import ctypes as C
import functools

import numpy as np

from faqcs_amd import _capi as capi
from faqcs_amd import driver

# the tile of the kernels: DETECT_TILE_VECS (1 024) vectors of 16 bytes -- 16 384 quality bytes, or 2 048 results of 8 bytes -- and the
# threads of the finishing block, which loops when there are more partials than that (faqcs_detect_kernel.hip)
T = 16384
T_RESULTS = 2048
FINISH_THREADS = 1024

PAD_BEFORE, PAD_AFTER = capi.ARENA_PAD_BEFORE, capi.ARENA_PAD_AFTER
HI, LO, NEG80, NEGFF = ord("~"), ord("!"), 0x80, 0xFF
KINDS = {"hi": HI, "lo": LO, "x80": NEG80, "xff": NEGFF}
VERDICT = {HI: 64, ord("K"): 64, LO: 33, ord(":"): 33, NEG80: 33, NEGFF: 33}
SEED = 20261019


def split(rng, total, n):
    """n read lengths that sum to total, zero-length reads among them"""
    if n == 1:
        return [total]
    cuts = np.sort(rng.integers(0, total + 1, n - 1))
    cuts[rng.random(n - 1) < 0.2] = cuts[0]  # runs of empty reads
    cuts = np.sort(cuts)
    return np.diff(np.concatenate([[0], cuts, [total]])).astype(np.int64).tolist()


class DetectCase:
    """store = [16 hostile bytes | arena | 64 hostile bytes]; arena position p is store[16 + p].  plants: {arena position: byte}.
    deflines: None, or one bytes per read -- laid down back to back in `order` (a permutation of the reads) as the whole text."""

    def __init__(self, name, lens, first, count, plants=(), deflines=None, order=None, expect=None, seed=0, big=False):
        rng = np.random.Generator(np.random.PCG64([SEED, seed, len(name)]))
        self.name, self.first, self.count, self.expect, self.big = name, first, count, expect or {}, big
        lens = np.asarray(lens, np.int64)
        self.n = len(lens)
        self.offset = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
        total = int(self.offset[-1])
        store = rng.integers(ord("A"), ord("J") + 1, PAD_BEFORE + total + PAD_AFTER).astype(np.uint8)
        store[:PAD_BEFORE] = np.resize(np.array([LO, HI, NEGFF, HI], np.uint8), PAD_BEFORE)
        store[PAD_BEFORE + total:] = np.resize(np.array([HI, LO, HI, NEG80], np.uint8), PAD_AFTER)
        for p, b in dict(plants).items():
            store[PAD_BEFORE + p] = b
        self.store, self.qual, self.total = store, store[PAD_BEFORE:PAD_BEFORE + total], total
        self.text = self.def_pos = self.def_len = None
        if deflines is not None:
            order = list(range(self.n)) if order is None else order
            self.def_len = np.array([len(d) for d in deflines], np.uint32)
            self.def_pos = np.zeros(self.n, np.uint32)
            pos = 0
            for i in order:
                self.def_pos[i] = pos
                pos += len(deflines[i])
            self.text = np.frombuffer(b"".join(deflines[i] for i in order), np.uint8).copy()

    def model(self):
        return driver.detect_model(self.qual, self.offset, self.first, self.count, self.text, self.def_pos, self.def_len)

    def host(self, lib):
        """faqcs_detect_host on exactly these arrays (no padding is handed over: the host form needs none) -> dict"""
        qual = np.ascontiguousarray(self.qual) if self.total else np.zeros(1, np.uint8)
        b = capi.Batch(None, qual.ctypes.data, self.offset.ctypes.data, self.n, 0, None, 0, None)
        info = capi.DetectInfo(-1, 0xDEAD, 0xDEAD, 0xDEAD, 0xDEAD, 0xDEAD)
        t = self.text if self.text is None or len(self.text) else np.zeros(1, np.uint8)
        rc = lib.faqcs_detect_host(C.byref(b), self.first, self.count, t.ctypes.data if t is not None else None,
                                   self.def_pos.ctypes.data if t is not None else None, self.def_len.ctypes.data if t is not None else None, C.byref(info))
        assert rc == 0, lib.faqcs_last_error()
        return info_dict(info)


def info_dict(info):
    return {f: int(getattr(info, f)) for f, _ in type(info)._fields_}


def _single_hits():
    out = []
    rng = np.random.Generator(np.random.PCG64([SEED, 1]))
    total = 2 * T + 37
    for where, p in [("0", 0), ("1", 1), ("15", 15), ("16", 16), ("17", 17), ("T-1", T - 1), ("T", T), ("T+1", T + 1), ("last", total - 1)]:
        for kind, byte in KINDS.items():
            out.append(DetectCase("single_%s_%s" % (where, kind), split(rng, total, 40), 0, 40, {p: byte}, expect={"quality_offset": VERDICT[byte], "byte": byte}, seed=p))
    # a range that starts at arena positions 1 .. 15: the head of its first vector belongs to the read in front of it, which is decisive throughout
    for k in range(1, 16):
        for j, (kind, byte) in enumerate(KINDS.items()):
            for where, p in (("first", k), ("vec1", 16), ("T-1", (k & ~15) + T - 1), ("T", (k & ~15) + T))[j % 2::2]:
                plants = {q: (HI if q & 1 else LO) for q in range(k)}
                plants[p] = byte
                lens = [k] + split(rng, total, 9)
                i = int(np.searchsorted(np.cumsum(lens), p, side="right"))
                out.append(DetectCase("head_%d_%s_%s" % (k, where, kind), lens, 1, 9, plants,
                                      expect={"quality_offset": VERDICT[byte], "byte": byte, "read": i}, seed=100 + k))
    return out


def _two_hits():
    out = []
    rng = np.random.Generator(np.random.PCG64([SEED, 2]))
    total = 3 * T + 11
    places = {"adjacent": (21, 22), "same_dword": (4, 7), "same_vector": (35, 44), "same_tile": (100, 9000), "neighbouring_tiles": (T - 5, T + 5),
              "first_and_last_tile": (7, total - 3), "across_waves": (16 * 63, 16 * 64), "across_passes": (16 * 255 + 15, 16 * 256)}
    for name, (p, q) in places.items():
        for a, b in ((HI, LO), (LO, HI), (ord("K"), NEGFF), (ord(":"), ord("K"))):
            out.append(DetectCase("two_%s_%d_%d" % (name, a, b), split(rng, total, 25), 0, 25, {p: a, q: b},
                                  expect={"quality_offset": VERDICT[a], "byte": a}, seed=p))
    return out


def _outside():
    """decisive bytes in front of the range and behind it only -- in the padding, or in the neighbouring reads -- and the same with a hit inside"""
    out = []
    rng = np.random.Generator(np.random.PCG64([SEED, 3]))
    for inside in (False, True):
        for head in (0, 16, 21, 48):  # the bytes of the reads in front of the range (0: the range starts the arena; its neighbour is the padding)
            for body in (1, 16, 31, 64, T + 3):
                for tail in (0, 64, 77):
                    lens = ([head] if head else []) + split(rng, body, 5) + ([tail] if tail else [])
                    first = 1 if head else 0
                    plants = {p: (HI if p & 1 else LO) for p in range(max(head - 16, 0), head)}
                    plants.update({head + body + p: (LO if p & 1 else NEG80) for p in range(min(tail, 64))})
                    expect = {"quality_offset": 0, "read": first + 5, "pos": 0, "byte": 0}
                    if inside:
                        p = head + int(rng.integers(0, body))
                        plants[p] = HI
                        expect = {"quality_offset": 64, "byte": HI}
                    out.append(DetectCase("outside_%d_%d_%d_%d" % (inside, head, body, tail), lens, first, 5, plants, expect=expect, seed=head + body))
    return out


def _attribution():
    out = []
    none = {"quality_offset": 0, "pos": 0, "byte": 0}
    out.append(DetectCase("no_hit", [50, 0, 70, 3], 0, 4, expect=dict(none, read=4)))
    out.append(DetectCase("no_hit_one_byte", [1], 0, 1, expect=dict(none, read=1)))
    for first in (0, 3, 5):
        out.append(DetectCase("count0_first%d" % first, [20, 30, 0, 40, 50], first, 0, {0: LO, 50: HI, 90: LO}, expect=dict(none, read=first, next_seq=0),
                              deflines=[b"@NS1"] * 5))
    out.append(DetectCase("empty_batch", [], 0, 0, expect=dict(none, read=0)))
    out.append(DetectCase("only_empty_reads", [30, 0, 0, 0, 40], 1, 3, {29: LO, 30: HI}, expect=dict(none, read=4)))
    out.append(DetectCase("only_empty_reads_whole_batch", [0, 0, 0], 0, 3, expect=dict(none, read=3)))
    # empty reads directly in front of and behind the read that owns the hit
    for p, pos in ((40, 0), (44, 4), (49, 9)):
        out.append(DetectCase("owner_between_empty_reads_%d" % pos, [40, 0, 0, 10, 0, 0, 25], 0, 7, {p: LO}, expect={"quality_offset": 33, "read": 3, "pos": pos, "byte": LO}))
        out.append(DetectCase("owner_between_empty_reads_%d_first2" % pos, [40, 0, 0, 10, 0, 0, 25], 2, 4, {p: HI, 39: LO, 50: LO}, expect={"quality_offset": 64, "read": 3, "pos": pos, "byte": HI}))
    out.append(DetectCase("owner_is_last_read_behind_empty_reads", [12, 0, 0, 1], 0, 4, {12: NEGFF}, expect={"quality_offset": 33, "read": 3, "pos": 0, "byte": NEGFF}))
    out.append(DetectCase("owner_is_first_read_before_empty_reads", [0, 0, 5, 0, 0], 0, 5, {4: HI}, expect={"quality_offset": 64, "read": 2, "pos": 4, "byte": HI}))
    # first > 0: hits in front of the range and behind it belong to other calls
    out.append(DetectCase("first_gt0", [100, 150, 150, 150, 100], 2, 2, {5: LO, 120: LO, 249: LO, 333: HI, 550: LO, 600: LO}, expect={"quality_offset": 64, "read": 2, "pos": 83, "byte": HI}))
    out.append(DetectCase("first_gt0_last_read", [100, 150, 150], 2, 1, {5: LO, 249: LO, 399: ord("K")}, expect={"quality_offset": 64, "read": 2, "pos": 149, "byte": ord("K")}))
    # every byte value in turn as the only candidate: the signed compare, 59 and 74 included
    for b in (0, 1, 58, 59, 60, 73, 74, 75, 76, 127, 128, 129, 254, 255):
        v = 0 if 59 <= b <= 74 else (64 if 75 <= b <= 127 else 33)
        out.append(DetectCase("byte_%d" % b, [7, 9], 0, 2, {9: b}, expect={"quality_offset": v, "read": 1 if v else 2, "pos": 2 if v else 0, "byte": b if v else 0}))
    return out


def _big():
    """more tiles than the finishing block has threads: the only hit in the last tile, in tile 0, and none"""
    out = []
    total = (FINISH_THREADS + 2) * T + 5
    lens = [150] * (total // 150) + [total % 150]
    for name, p in (("last_tile", total - 2), ("tile0", 9), ("none", None)):
        expect = {"quality_offset": 33, "read": p // 150, "pos": p % 150, "byte": LO} if p is not None else {"quality_offset": 0, "read": len(lens)}
        out.append(DetectCase("big_" + name, lens, 0, len(lens), {p: LO} if p is not None else {}, expect=expect, big=True))
    return out


DEFLINES = [(b"@NS", 1), (b"@NS500:1", 1), (b"@N", 0), (b"", 0), (b"NS500", 0), (b"@ns", 0), (b"x@NS", 0)]


def _deflines():
    """the defline of read `first` at text position 0 and at the text's last bytes; the other reads' deflines would give the other answer"""
    out = []
    for d, want in DEFLINES:
        other = b"S@N" if want else b"S@NS500"  # (behind "@N" the text goes on with "S@NS...")
        for first in (0, 2):
            for where in ("start", "end"):
                n = 4
                deflines = [other] * n
                deflines[first] = d
                rest = [i for i in range(n) if i != first]
                order = [first] + rest if where == "start" else rest + [first]
                out.append(DetectCase("defline_%s_first%d_%s" % (d.decode() or "empty", first, where), [5, 0, 6, 7], first, n - first, {0: LO},
                                      deflines=deflines, order=order, expect={"next_seq": want}))
    # deflines given, but no read in the range
    out.append(DetectCase("defline_count0", [5, 5], 1, 0, deflines=[b"@NS", b"@NS"], expect={"next_seq": 0, "read": 1}))
    return out


@functools.lru_cache(maxsize=None)
def detect_cases():
    return tuple(_single_hits() + _two_hits() + _outside() + _attribution() + _deflines() + _big())


# ---- faqcs_first_error_* -----------------------------------------------------------------------------------------------------------------------

EQ, EB = capi.F_ERR_QUALITY, capi.F_ERR_BASE
NOISE = 0xFFFF & ~(EQ | EB)


class ErrorCase:
    """n results with random windows and adapters; flags = noise (the non-error bits, at random or all set) | the planted error bits"""

    def __init__(self, name, n, plants=(), noise="random", expect=None, big=False):
        rng = np.random.Generator(np.random.PCG64([SEED, 7, n, len(name)]))
        self.name, self.n, self.expect, self.big = name, n, expect, big
        res = np.zeros(n, dtype=capi.RESULT_DTYPE)
        res["start"] = rng.integers(0, 1 << 16, n)
        res["len"] = rng.integers(0, 1 << 16, n)
        res["adapter"] = rng.integers(0, 1 << 16, n)  # (0x0300 in the adapter field is no error)
        res["flags"] = (rng.integers(0, 1 << 16, n) & NOISE) if noise == "random" else NOISE
        for i, f in dict(plants).items():
            res["flags"][i] |= f
        self.res = res

    def model(self):
        return driver.first_error_model(self.res)

    def host(self, lib):
        info = capi.ErrorInfo(0xDEAD, 0xDEAD)
        rc = lib.faqcs_first_error_host(self.res.ctypes.data if self.n else None, self.n, C.byref(info))
        assert rc == 0, lib.faqcs_last_error()
        return int(info.n_good), int(info.flags)


@functools.lru_cache(maxsize=None)
def error_cases():
    out = []
    n = 2 * T_RESULTS + 5
    for fname, f in (("quality", EQ), ("base", EB)):
        for where, i in (("0", 0), ("1", 1), ("last", n - 1), ("T-1", T_RESULTS - 1), ("T", T_RESULTS), ("T+1", T_RESULTS + 1), ("2T-1", 2 * T_RESULTS - 1), ("2T", 2 * T_RESULTS)):
            out.append(ErrorCase("one_%s_%s" % (fname, where), n, {i: f}, expect=(i, f)))
    out.append(ErrorCase("both_flags_on_one_read", n, {777: EQ | EB}, expect=(777, EQ | EB)))
    out.append(ErrorCase("flagged_reads_behind_the_first", n, {300: EB, 301: EQ, 2047: EQ | EB, 2048: EQ, n - 1: EQ}, expect=(300, EB)))
    out.append(ErrorCase("flagged_reads_in_every_tile", n, {T_RESULTS - 1: EQ, T_RESULTS: EB, 2 * T_RESULTS + 1: EB}, expect=(T_RESULTS - 1, EQ)))
    out.append(ErrorCase("second_of_a_vector", n, {1001: EQ, 1002: EB}, expect=(1001, EQ)))
    out.append(ErrorCase("none", n, expect=(n, 0)))
    out.append(ErrorCase("n0", 0, expect=(0, 0)))
    out.append(ErrorCase("n1_none", 1, expect=(1, 0)))
    out.append(ErrorCase("n1_flagged", 1, {0: EB}, expect=(0, EB)))
    out.append(ErrorCase("odd_n_last", 2049, {2048: EQ}, expect=(2048, EQ)))
    out.append(ErrorCase("other_bits_everywhere_none", n, noise="all", expect=(n, 0)))
    out.append(ErrorCase("other_bits_everywhere_one", n, {n - 2: EB}, noise="all", expect=(n - 2, EB)))
    big = (FINISH_THREADS + 2) * T_RESULTS + 1
    out.append(ErrorCase("big_last_tile", big, {big - 1: EQ}, expect=(big - 1, EQ), big=True))
    out.append(ErrorCase("big_tile0", big, {5: EB, big - 1: EQ}, expect=(5, EB), big=True))
    out.append(ErrorCase("big_none", big, expect=(big, 0), big=True))
    return tuple(out)
