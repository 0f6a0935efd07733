"""The fixed part of trim_lds's S step ("the read's totals as a reduce-scatter"): the base counts of a read, which the 8-lane
shapes add up over the eight steps of a chunk and hand to the read's lane by a permutation behind the loop, and the adjacent-N test, which a
step enters only where a lane's own N count (and its neighbour's) allows two adjacent N.  Batches built so that a total in the wrong lane, a
pending level left out of a partial chunk, or a pair of N the gate does not let through changes a verdict, a composition bin or a
filter_stats sum: every counter and every per-read result against the oracle, at the four lane geometries of trim_lds.

Each case runs three launches in one engine (the position x base registers are spilled to LDS once in seven chunks)."""
import numpy as np
import pytest

from faqcs_amd import driver
from faqcs_amd.options import parse_args
from test_gpu_parity import SEED, compare_engines

pytestmark = pytest.mark.gpu

# read length -> (lanes per read, positions per lane) of the trim_lds shape that takes it
GEOMETRY = {150: (8, 19), 100: (8, 13), 75: (4, 19), 250: (16, 16)}
ACGT = np.frombuffer(b"ACGT", np.uint8)
HEADLINE = []                 # the headline variants: -n 2 tested inside the S loop
JUDGED = ["--avg_q", "40.5"]  # no read reaches the average: every read is judged for poly-N without being counted (chk)


def _read(seq, qual):
    return (b"@s", np.asarray(seq, np.uint8).tobytes(), (np.asarray(qual) + 33).astype(np.uint8).tobytes())


def _window_qual(L, lo, hi):
    """Qualities that BWA_plus trims to the kept window [lo, hi)."""
    q = np.full(L, 2)
    q[lo:hi] = 40
    return q


def _check(reads, args=()):
    opt = parse_args(["-u", "x", "-d", "y"] + list(args))
    seq, qual, offset, seg = driver.pack_segments([reads])
    hip, ora = compare_engines(opt, reads, R=256 if max(len(r[1]) for r in reads) <= 256 else 1024)
    for _ in range(2):
        r1 = hip.process(seq, qual, offset, seg)
        r2 = ora.process(seq, qual, offset, seg)
        bad = np.nonzero(r1 != r2)[0]
        assert len(bad) == 0, "later launch: first differing read %d: hip=%s oracle=%s seq=%r" % (bad[0], r1[bad[0]], r2[bad[0]], reads[bad[0]][1])
    c1, c2 = hip.counters(), ora.counters()
    bad = np.nonzero(c1 != c2)[0]
    assert len(bad) == 0, "counter block differs in %d places after three launches, first at %d: hip=%d oracle=%d" % (len(bad), bad[0] if len(bad) else -1,
                                                                                                                  c1[bad[0]] if len(bad) else 0, c2[bad[0]] if len(bad) else 0)
    hip.close()
    ora.close()


def _pair_reads(rng, L):
    """"NN" across every lane seam (kC - 1, kC) and in the middle of every lane, and the pairs that must not trip ("N.N", "nN", "Nn"), each
    under three kept windows: one that holds both N, one that ends between them, one that starts between them."""
    lpr, C = GEOMETRY[L]
    places = [k * C - 1 for k in range(1, lpr) if k * C < L - 1] + [k * C + C // 2 for k in range(lpr) if k * C + C // 2 + 2 < L]
    reads = []
    for p in places:
        for pat in (b"NN", b"N.N", b"nN", b"Nn"):
            s0 = ACGT[rng.integers(0, 4, L)].copy()
            second = p + len(pat) - 1
            s0[p] = pat[0]
            s0[second] = pat[-1]
            for lo, hi in ((max(0, p - 40), min(L, second + 41)), (max(0, p - 60), p + 1), (second, min(L, second + 60))):
                reads.append(_read(s0, _window_qual(L, lo, hi)))
    return reads


@pytest.mark.parametrize("args", [HEADLINE, JUDGED], ids=["headline", "judged_uncounted"])
@pytest.mark.parametrize("L", sorted(GEOMETRY))
def test_adjacent_n_at_every_lane_seam_and_inside_a_lane(L, args):
    rng = np.random.Generator(np.random.PCG64([1, L, SEED]))
    reads = _pair_reads(rng, L)
    # in two orders: the pattern meets every row of the wave and every step of a chunk
    order = rng.permutation(len(reads))
    _check(reads + [reads[i] for i in order], ["--min_L", "1"] + args)


@pytest.mark.parametrize("L", sorted(GEOMETRY))
def test_many_n_none_adjacent(L):
    """Reads with two or more N in every lane and no two adjacent (every step enters the test, none may trip), and reads with one N per lane
    at alternating ends of the lanes (every second seam holds a pair, split between two lanes that hold one N each), upper and lower case."""
    rng = np.random.Generator(np.random.PCG64([2, L, SEED]))
    lpr, C = GEOMETRY[L]
    reads = []
    for rep in range(40):
        s = ACGT[rng.integers(0, 4, L)].copy()
        for k in range(lpr):
            for o in (1, 3 + rep % 3, C - 2):
                if k * C + o < L:
                    s[k * C + o] = ord("N")
        reads.append(_read(s, _window_qual(L, rep % 5, L - rep % 7)))
        s = ACGT[rng.integers(0, 4, L)].copy()
        for k in range(lpr):
            p = k * C + (C - 1 if (k + rep) % 2 == 0 else 0)
            if p < L:
                s[p] = ord("n") if rep % 4 == 3 and k == 1 else ord("N")
        reads.append(_read(s, _window_qual(L, rep % 5, L - rep % 7)))
        # the same seams with the kept window cut at the pair
        cut = (1 + rep % (lpr - 1)) * C
        if cut < L:
            reads.append(_read(s, _window_qual(L, 0, cut)))
            reads.append(_read(s, _window_qual(L, cut, L)))
        reads.append(_read(ACGT[rng.integers(0, 4, L)], _window_qual(L, 0, L)))
    _check(reads, ["--min_L", "1"])


def _composed_read(rng, i, L=150):
    """Read i of a batch: a base composition of its own (and some N), a kept window of its own."""
    p = rng.dirichlet(np.full(4, 0.6))
    s = ACGT[rng.choice(4, L, p=p)].copy()
    s[rng.random(L) < 0.01 * (i % 4)] = ord("N")
    return _read(s, _window_qual(L, i % 9, L - (5 * i) % 41))


@pytest.mark.parametrize("n", list(range(1, 10)) + list(range(57, 66)) + [127, 128, 129])
def test_partial_chunks(n):
    """Every count of executed steps of the last chunk (n mod 64 = 1 ... 9: reads in 1 ... 8 rows and the first step of the next row's turn;
    57 ... 65; 127 ... 129), every position in the pair, four and eight grouping of the steps; every read has a composition of its own."""
    rng = np.random.Generator(np.random.PCG64([3, n, SEED]))
    _check([_composed_read(rng, i) for i in range(n)], ["--min_L", "1"])


@pytest.mark.parametrize("L", [150, 250, 300])
def test_totals_at_the_field_limits(L):
    """Reads of one base and of two bases: 19 (16) in a lane's field, the whole read in a read's field; the low-complexity and dinucleotide
    verdicts; a read of N only (at 300 bases: the N register of the widest shape)."""
    rng = np.random.Generator(np.random.PCG64([4, L, SEED]))
    reads = []
    for rep in range(6):
        for b in b"ACGTNacgtn":
            reads.append(_read(np.full(L, b, np.uint8), _window_qual(L, rep, L - 2 * rep)))
        for x, y in (b"AC", b"GT", b"AT", b"CG", b"TN", b"aG"):
            alt = np.where(np.arange(L) % 2 == 0, x, y).astype(np.uint8)
            half = np.where(np.arange(L) < L // 2, x, y).astype(np.uint8)
            runs = np.where((np.arange(L) // 3) % 2 == 0, x, y).astype(np.uint8)
            for s in (alt, half, runs):
                reads.append(_read(s, _window_qual(L, rep, L - rep)))
        reads.append(_read(ACGT[rng.integers(0, 4, L)], _window_qual(L, 0, L)))
    for args in (["--min_L", "1"], ["--min_L", "1", "--lc", "1.0", "-n", "2000"]):
        _check(reads, args)


@pytest.mark.parametrize("L", [150, 100])
def test_take_back_of_reads_vetoed_after_counting(L):
    """Most reads are rejected after their post-trim cells were counted (-n 1 on reads with 2 % N): the pass that takes them back (MODE 1)
    computes no totals and must leave the ones of the counting pass alone."""
    rng = np.random.Generator(np.random.PCG64([5, L, SEED]))
    n = 3000
    s = np.frombuffer(b"ACGTNacgt", np.uint8)[rng.choice(9, (n, L), p=[.2, .2, .2, .2, .02, .045, .045, .045, .045])]
    q = rng.integers(28, 41, (n, L))
    q[::7, L - 5:] = 1
    _check([_read(s[i], q[i]) for i in range(n)], ["--min_L", "1", "--avg_q", "20", "-n", "1"])


@pytest.mark.parametrize("L", [150, 100])
def test_recount_of_chunks_with_a_byte_that_is_no_base(L):
    """A byte >= 0x80 among the bases of some chunks: such a chunk is taken back (MODE 2), patched and counted again -- totals, pair hits and all."""
    rng = np.random.Generator(np.random.PCG64([6, L, SEED]))
    reads = []
    for i in range(1500):
        s = ACGT[rng.choice(4, L, p=rng.dirichlet(np.full(4, 0.8)))].copy()
        if i % 97 == 5:
            s[int(rng.integers(0, L))] = 0x80 + i % 128
        if i % 31 == 3:
            p = int(rng.integers(1, L - 1))
            s[p] = s[p + 1] = ord("N")
        reads.append(_read(s, _window_qual(L, i % 4, L - i % 23)))
    _check(reads, ["--min_L", "1"])
