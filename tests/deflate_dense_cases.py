"""Texts and calls of the dense-mode deflate tests (faqcs_deflate_device_mode / faqcs_deflate_host_mode with FAQCS_DEFLATE_DENSE): the call
into canary-filled buffers in the form of deflate_cases.deflate_host, and texts CONSTRUCTED to reach one rule of the dense match finder each
(include/faqcs_mi.h at faqcs_deflate_device_mode), with the matches the rule demands.

How the texts are built: a filler of 24 letters in which no three bytes occur twice (deflate_cases.no_repeated_trigram), so that the filler
holds no match, and strings of RARE bytes (130 .. 249), every byte value used once per string and every placed string between two guard
bytes of its own.  The only repeats of a text are therefore the ones placed on purpose, and what the encoder must code follows from the
definition alone.  (A 12-bit hash can still collide: a filler position between a source and its copy that hashes like the copy takes the
source's place in a table.  The texts are fixed by their seed, and the tests would show it.)"""
import ctypes as C

import numpy as np

import deflate_cases as dc
import parse_cases as pc
from faqcs_amd import _capi as capi

FAST, DENSE = 0, 1
SUB, TILE = 256, 1024


def deflate_host_mode(lib, text, member_bytes=0, final=1, mode=DENSE, capacity=None, with_offsets=True, shift=0):
    """deflate_cases.deflate_host for faqcs_deflate_host_mode."""
    text = bytes(text)
    mb = member_bytes or dc.MAX_TEXT
    n = -(-len(text) // mb) + (1 if final else 0)
    cap = len(text) + 31 * n + 8 if capacity is None else capacity
    tb = np.zeros(shift + len(text) + 1, np.uint8)
    tb[shift:shift + len(text)] = np.frombuffer(text, np.uint8)
    comp = pc.aligned_bytes(dc.FRONT + cap + 64)
    moff = np.full(n + 2, dc.CAN32, np.uint32)
    info = capi.DeflateInfo(0xA5A5A5A5A5A5A5A5, 0xA5A5A5A5, 0xA5A5A5A5, 0xA5A5A5A5, 0xA5A5A5A5)
    out = capi.DeflateOut(comp.ctypes.data + dc.FRONT, cap, moff.ctypes.data if with_offsets else None, C.addressof(info))
    rc = lib.faqcs_deflate_host_mode(tb.ctypes.data + shift if len(text) else None, len(text), member_bytes, final, mode, C.byref(out))
    return rc, {"comp": comp, "member_offset": moff, "with_offsets": with_offsets, "cap": cap,
                "info": {f: int(getattr(info, f)) for f, _ in capi.DeflateInfo._fields_}}


class _Text:
    """A filler of n bytes and a pool of rare byte values handed out once each."""

    def __init__(self, rng, n):
        self.t = bytearray(dc.no_repeated_trigram(rng, n, 97, 121))
        self.pool = [int(v) for v in rng.permutation(np.arange(130, 250))]

    def rare(self, k):
        out, self.pool = bytes(self.pool[:k]), self.pool[k:]
        assert len(out) == k
        return out

    def place(self, at, s):
        """s at t[at ..), a guard byte of its own in front of it and one behind it (behind only where the text goes on)"""
        g = self.rare(2)
        assert at >= 1 and at + len(s) <= len(self.t)
        self.t[at - 1] = g[0]
        self.t[at:at + len(s)] = s
        if at + len(s) < len(self.t):
            self.t[at + len(s)] = g[1]

    def bytes(self):
        return bytes(self.t)


def _sub_tile(rng, P, D=100):
    """40 rare bytes at P - D and again at P.  Position P sees the source only when it lies in a sub-tile in front of P's own: at P = 255
    and P = 1 023 it does not, but position P + 1 -- the first of the next sub-tile -- sees source + 1."""
    x = _Text(rng, P + 300)
    s = x.rare(40)
    x.place(P - D, s)
    x.place(P, s)
    return x.bytes(), (([39], [D]) if P % SUB == SUB - 1 else ([40], [D]))


def _own_sub_tile(rng):
    """Source (270) and copy (330) in one sub-tile: no position of the copy sees any position of the source."""
    x = _Text(rng, 700)
    s = x.rare(40)
    x.place(270, s)
    x.place(330, s)
    return x.bytes(), ([], [])


def _own_sub_tile_run(rng):
    """40 equal bytes inside one sub-tile: the run candidate p - 1 needs no table."""
    x = _Text(rng, 700)
    x.place(300, x.rare(1) * 40)
    return x.bytes(), ([39], [1])


def _eight(rng, k):
    """The member ends k bytes behind p = 600.  Nine rare bytes R at 100, their first three -- the decoy, the latest position with p's three
    bytes -- at 200, and R[:k] at p.  k >= 8: the eight-byte table names position 100, the match is k long.  k = 7: position p neither
    enters nor looks up that table; it keeps the decoy's three bytes, position p + 1 finds six at 101 (the decoy ends there), and the lazy
    step gives p up."""
    p = 600
    x = _Text(rng, p + k)
    R = x.rare(9)
    x.place(100, R)
    x.place(200, R[:3])
    x.place(p, R[:k])
    return x.bytes(), (([k], [500]) if k >= 8 else ([6], [500]))


def _lazy_pair(rng, i):
    """len(i) = 5 by a source A = x y1 .. y4, len(i + 1) = 12 by a later source B = y1 .. y12.  Inside a tile position i becomes a
    literal; with i = 1 023, the last position of a tile, it keeps its match and the eight bytes behind it are found at B + 4."""
    x = _Text(rng, i + 40)
    s = x.rare(13)
    x.place(101, s[:5])
    x.place(151, s[1:])
    x.place(i, s)
    return x.bytes(), (([12], [i + 1 - 151]) if i % TILE != TILE - 1 else ([5, 8], [i - 101, i + 5 - 155]))


def _lazy_chain(rng):
    """len(i) = 4 < len(i + 1) = 8 < len(i + 2) = 16, by three sources A < B < C: on the lengths as found both i and i + 1 give way."""
    i = 600
    x = _Text(rng, i + 40)
    s = x.rare(18)  # a b c1 .. c16
    x.place(101, s[:4])
    x.place(151, s[1:9])
    x.place(201, s[2:])
    x.place(i, s)
    return x.bytes(), ([16], [i + 2 - 201])


def _lazy_equal(rng):
    """len(i) = len(i + 1) = 6: the rule does not fire."""
    i = 600
    x = _Text(rng, i + 40)
    s = x.rare(7)  # a c1 .. c6
    x.place(101, s[:6])
    x.place(151, s[1:])
    x.place(i, s)
    return x.bytes(), ([6], [i - 101])


def _tie(rng):
    """The same ten bytes at 101 and at 201, and at 600: equal lengths, the nearer source is coded."""
    x = _Text(rng, 640)
    s = x.rare(10)
    x.place(101, s)
    x.place(201, s)
    x.place(600, s)
    return x.bytes(), ([10], [399])


def far_by_eight(rng):
    """deflate_cases.far_repeat for candidate (b): 65 280 bytes of one filler byte, 40 rare bytes D = 32 768 and D = 32 769 in front of a
    tile's first position T and again at T, and 500 bytes in front of T a decoy -- the first three of them -- which takes the source's place
    in the three-byte table.  -> (text, [(T, D)])"""
    t = bytearray(b"z" * dc.MAX_TEXT)
    pool = rng.permutation(np.arange(130, 250))
    where = []
    for k, D in enumerate((32768, 32769)):
        T = TILE * (63 - 2 * k)
        src = bytes(int(v) for v in pool[40 * k:40 * k + 40])
        t[T - D:T - D + 40] = src
        t[T - 500:T - 497] = src[:3]
        t[T:T + 40] = src
        where.append((T, D))
    return bytes(t), where


def dense_edge_texts():
    """name -> (text, (lengths, distances) of the matches of its one member)"""
    rng = np.random.Generator(np.random.PCG64([239, dc.SEED]))
    out = {}
    for P in (255, 256, 257, 1023, 1024, 1025):
        out["sub_tile_%d" % P] = _sub_tile(rng, P)
    out["own_sub_tile"] = _own_sub_tile(rng)
    out["own_sub_tile_run"] = _own_sub_tile_run(rng)
    for k in (7, 8, 9):
        out["eight_bytes_%d" % k] = _eight(rng, k)
    out["lazy_pair"] = _lazy_pair(rng, 600)
    out["lazy_pair_across_tiles"] = _lazy_pair(rng, 1023)
    out["lazy_chain"] = _lazy_chain(rng)
    out["lazy_equal"] = _lazy_equal(rng)
    out["tie"] = _tie(rng)
    return out
