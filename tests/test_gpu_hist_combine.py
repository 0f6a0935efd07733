"""The LDS adds that the lanes of a wave combine before they add ("LDS adds that land on one address"): the six histogram
cells of a trim_lds chunk's epilogue -- read length, int(average quality), bases per quality bin, before and after trimming -- and the
composition fold.  Batches built so that the lanes of a wave meet on one cell, on a few, on every bin, or on none, at the four shapes of
trim_lds (4, 8 and 16 lanes per read; 64 and 32 reads per chunk), every counter against the oracle.

Each case runs three launches in one engine: compare_engines() reads the counters behind the first, which folds its composition records
with the standalone kernel (composition_histogram); the third launch folds the records of the second in the tail of its blocks
(comp_fold_tail) where the shape's blocks do that.  Then the same again in a fresh engine with FAQCS_TAIL_FOLD=0, where
composition_histogram folds every launch's records beside the next launch."""
import numpy as np
import pytest

from faqcs_amd import _capi as capi
from faqcs_amd import driver
from faqcs_amd.options import parse_args
from test_gpu_parity import SEED, compare_engines

pytestmark = pytest.mark.gpu

SHAPES = [150, 100, 75, 250]  # 8, 8, 4 and 16 lanes per read (250: 32 reads per chunk, half the lanes of the epilogue own no read)
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _read(seq, qual):
    return (b"@h", np.asarray(seq, np.uint8).tobytes(), (np.asarray(qual) + 33).astype(np.uint8).tobytes())


def _bases(rng, L):
    return ACGT[rng.integers(0, 4, L)]


def _headline_qual(rng, L):
    """Good qualities with a low tail from a random breakpoint on, as the benchmark's reads have: the kept length is spread, the
    post-trim average sits on a few values."""
    q = rng.integers(30, 41, L)
    b = int(rng.integers(L // 2, L + 41))
    q[b:] = 2
    return q


def _check(reads, monkeypatch, args=()):
    opt = parse_args(["-u", "x", "-d", "y"] + list(args))
    seq, qual, offset, seg = driver.pack_segments([reads])
    for tail_fold in (None, "0"):
        if tail_fold is None:
            monkeypatch.delenv("FAQCS_TAIL_FOLD", raising=False)
        else:
            monkeypatch.setenv("FAQCS_TAIL_FOLD", tail_fold)
        hip, ora = compare_engines(opt, reads)
        for _ in range(2):
            r1 = hip.process(seq, qual, offset, seg)
            r2 = ora.process(seq, qual, offset, seg)
            assert (r1 == r2).all()
        c1, c2 = hip.counters(), ora.counters()
        bad = np.nonzero(c1 != c2)[0]
        assert len(bad) == 0, "FAQCS_TAIL_FOLD=%s: counter block differs in %d places after three launches, first at %d: hip=%d oracle=%d" % (
            tail_fold, len(bad), bad[0], c1[bad[0]], c2[bad[0]])
        hip.close()
        ora.close()


@pytest.mark.parametrize("n", [64, 65, 130])
@pytest.mark.parametrize("L", SHAPES)
def test_identical_reads(L, n, monkeypatch):
    """One cell of every histogram takes everything; the last chunk is partial (65, 130) or there is one full chunk (64)."""
    rng = np.random.Generator(np.random.PCG64([1, L, SEED]))
    s, q = _bases(rng, L), rng.integers(30, 41, L)
    _check([_read(s, q)] * n, monkeypatch)


@pytest.mark.parametrize("k", [1, 2, 17, 42])
@pytest.mark.parametrize("L", SHAPES)
def test_pre_trim_average_quality_on_k_values(L, k, monkeypatch):
    """Reads of one length whose int(average quality) before trimming takes 1, 2, 17 and 42 distinct values (42: every bin of the histogram)."""
    rng = np.random.Generator(np.random.PCG64([2, L, k, SEED]))
    values = {1: [35], 2: [40, 30], 17: list(range(25, 42)), 42: list(range(42))}[k]
    reads = []
    for _ in range(3000):
        v = values[int(rng.integers(0, len(values)))]
        q = np.full(L, v)
        if v < 41 and v > 0 and rng.random() < 0.5:  # (the same floor from another sum: one base a step higher)
            q[int(rng.integers(0, L))] += 1
        reads.append(_read(_bases(rng, L), q))
    _check(reads, monkeypatch)


@pytest.mark.parametrize("L", SHAPES)
def test_sixty_four_lengths_in_a_chunk(L, monkeypatch):
    """Every read of a chunk has a length of its own: no two lanes share a cell of the length histogram."""
    rng = np.random.Generator(np.random.PCG64([3, L, SEED]))
    reads = []
    for _ in range(12):
        for n in rng.permutation(np.arange(L - 63, L + 1)):
            reads.append(_read(_bases(rng, int(n)), _headline_qual(rng, int(n))))
    _check(reads, monkeypatch)


@pytest.mark.parametrize("L", SHAPES)
def test_two_lengths_alternating(L, monkeypatch):
    rng = np.random.Generator(np.random.PCG64([4, L, SEED]))
    reads = [_read(_bases(rng, L - (i & 1)), _headline_qual(rng, L - (i & 1))) for i in range(3000)]
    _check(reads, monkeypatch)


@pytest.mark.parametrize("L", SHAPES)
def test_every_read_rejected(L, monkeypatch):
    """No read survives trimming: the post-trim half of the epilogue has no lane."""
    rng = np.random.Generator(np.random.PCG64([5, L, SEED]))
    reads = [_read(_bases(rng, L), np.full(L, 2)) for _ in range(3000)]
    _check(reads, monkeypatch)


@pytest.mark.parametrize("L", SHAPES)
def test_every_read_with_a_quality_error(L, monkeypatch):
    """A score above 41 in every read: no lane of any chunk takes part in the histograms.  The batch is refused with E_QUALITY, as the
    oracle refuses it (its counters stop at the first such read, so there is no counter block to compare); both fold settings."""
    from faqcs_amd.engine import FaqcsError

    rng = np.random.Generator(np.random.PCG64([6, L, SEED]))
    reads = []
    for _ in range(2000):
        q = rng.integers(30, 41, L)
        q[int(rng.integers(0, L))] = 42
        reads.append(_read(_bases(rng, L), q))
    opt = parse_args(["-u", "x", "-d", "y"])
    for tail_fold in (None, "0"):
        if tail_fold is None:
            monkeypatch.delenv("FAQCS_TAIL_FOLD", raising=False)
        else:
            monkeypatch.setenv("FAQCS_TAIL_FOLD", tail_fold)
        with pytest.raises(FaqcsError) as ei:
            compare_engines(opt, reads)
        assert ei.value.code == capi.E_QUALITY


@pytest.mark.parametrize("L", SHAPES)
def test_base_counts_far_apart(L, monkeypatch):
    """Reads of one base next to reads of uniform composition: the base counts of a wave's records lie further apart than any 64-wide window."""
    rng = np.random.Generator(np.random.PCG64([7, L, SEED]))
    reads = []
    for i in range(3000):
        s = np.full(L, ord("ACGT"[(i >> 1) & 3]), np.uint8) if i & 1 else _bases(rng, L)
        reads.append(_read(s, _headline_qual(rng, L)))
    _check(reads, monkeypatch, ["--lc", "1.0"])  # (nothing is rejected for low complexity: the one-base reads reach the post-trim side too)


@pytest.mark.parametrize("L", SHAPES)
def test_reads_with_n(L, monkeypatch):
    rng = np.random.Generator(np.random.PCG64([8, L, SEED]))
    reads = []
    for _ in range(3000):
        s = _bases(rng, L).copy()
        s[rng.random(L) < (0.03 if rng.random() < 0.5 else 0.0)] = ord("N")
        reads.append(_read(s, _headline_qual(rng, L)))
    _check(reads, monkeypatch, ["-n", "20"])


@pytest.mark.parametrize("L", SHAPES)
def test_seventy_thousand_identical_reads(L, monkeypatch):
    """More reads on one cell than a 16-bit cell of the fold's table or of a block's histograms holds."""
    rng = np.random.Generator(np.random.PCG64([9, L, SEED]))
    s, q = _bases(rng, L), rng.integers(30, 41, L)
    _check([_read(s, q)] * 70000, monkeypatch)
