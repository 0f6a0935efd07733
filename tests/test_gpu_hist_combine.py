"""The LDS adds that the lanes of a wave combine before they add ("LDS adds that land on one address"): the six histogram
cells of a trim_lds chunk's epilogue -- read length, int(average quality), bases per quality bin, before and after trimming -- and the
composition fold.  Batches built so that the lanes of a wave meet on one cell, on a few, on every bin, or on none, at the four shapes of
trim_lds (4, 8 and 16 lanes per read; 64 and 32 reads per chunk), every counter against the oracle.

Each case runs two passes of three launches, each pass under both values of FAQCS_TAIL_FOLD:
    synced     HipEngine.process() is faqcs_submit + faqcs_sync, and faqcs_sync folds what is pending: composition_histogram on the compute
               stream folds every launch's records, whatever FAQCS_TAIL_FOLD says.  This pass is about the epilogue's cells.
    unsynced   the same three launches through faqcs_submit_device on a fresh engine with no sync between them, then one faqcs_finish:
               the second and the third launch fold the records of the one before in the tail of their blocks (comp_fold_tail) where the
               shape's blocks do that (105 ... 252 bases), else -- and always with FAQCS_TAIL_FOLD=0 -- composition_histogram folds them on
               the aux stream beside the launch; the last launch's records are folded by faqcs_finish.  faqcs_path_tallies_get() says so."""
import ctypes as C

import numpy as np
import pytest

from faqcs_amd import _capi as capi
from faqcs_amd import driver
from faqcs_amd.options import parse_args
import trim_dispatch_cases as td
from test_gpu_parity import SEED, compare_engines, hip_factory

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
        _unsynced(opt, args, seq, qual, offset, seg, tail_fold, c2)  # (the oracle's block behind the same three launches)


def _unsynced(opt, args, seq, qual, offset, seg, tail_fold, c2, launches=3):
    """The same batch `launches` times through faqcs_submit_device with nothing between the calls, one faqcs_finish: the whole block against
    the oracle's, and the arms the folds took."""
    import torch

    from faqcs_amd.engine import _check as check

    n, longest = len(offset) - 1, int(np.diff(offset.astype(np.int64)).max())
    dev = torch.device("cuda:0")
    front, total = 64, int(offset[-1])
    arenas = []
    for a in (seq, qual):
        h = np.full(front + total + 128, ord("N"), np.uint8)
        h[front:front + total] = a[:total]
        arenas.append(torch.from_numpy(h).to(dev))
    d_off = torch.from_numpy(np.ascontiguousarray(offset, np.uint32).view(np.int32)).to(dev)
    res = torch.zeros((n, 4), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    hip = hip_factory(opt, 256, 33)
    try:
        seg = np.ascontiguousarray(seg, np.uint32)
        b = capi.Batch(arenas[0].data_ptr() + front, arenas[1].data_ptr() + front, d_off.data_ptr(), n, len(seg) - 1, seg.ctypes.data, longest, None)
        for _ in range(launches):
            check(hip.lib, hip.lib.faqcs_submit_device(hip.ctx, C.byref(b), res.data_ptr()))
        c1 = hip.counters()
        bad = np.nonzero(c1 != c2)[0]
        assert len(bad) == 0, "FAQCS_TAIL_FOLD=%s, %d launches without a sync: counter block differs in %d places, first at %d: hip=%d oracle=%d" % (
            tail_fold, launches, len(bad), bad[0], c1[bad[0]], c2[bad[0]])
        t = capi.PathTallies()
        assert hip.lib.faqcs_path_tallies_get(hip.ctx, C.byref(t)) == 0
        folds = bool(td.expected_plan(dict(td.option_fields(list(args)), fold_n=n), longest, n, 256, td.DEFAULT_SWITCHES)["folds_tail"]) and tail_fold is None
        assert (t.folds_tail, t.folds_aux, t.folds_now, t.folds_dropped) == ((launches - 1, 0, 1, 0) if folds else (0, launches - 1, 1, 0)), \
            "FAQCS_TAIL_FOLD=%s, longest read %d: %d tail, %d aux, %d now" % (tail_fold, longest, t.folds_tail, t.folds_aux, t.folds_now)
    finally:
        hip.close()


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
