"""The adjacent-N test of trim_lds behind the S loop ("the adjacent-N test, deferred"): a step of the counting pass only
records, one bit per step, that some lane's gate tripped; a pass behind the loop reloads the flagged steps from the staged bases and runs the
test there.  Batches built so that a flagged step that is not looked at, a verdict handed to the wrong step's read, a flag mask or a verdict
that survives into the next chunk or into the recount of a patched chunk, or a pair seen across the edge of the kept window changes a
per-read result or a counter: everything against the oracle, at the four lane geometries of trim_lds.

Read i of a chunk belongs to step i mod TPR of its chunk (TPR = 4, 8, 8 and 5 steps at 50, 150, 250 and 300 bases; chunks of 64, 64, 32
and 20 reads)."""
import numpy as np
import pytest

from faqcs_amd import _capi as capi
from faqcs_amd import driver
from faqcs_amd.options import parse_args
from test_gpu_parity import SEED, hip_factory

pytestmark = pytest.mark.gpu

# read length -> (lanes per read, positions per lane, reads per chunk) of the trim_lds shape that takes it
GEOMETRY = {50: (4, 13, 64), 150: (8, 19, 64), 250: (16, 16, 32), 300: (16, 19, 20)}
LENGTHS = sorted(GEOMETRY)
ACGT = np.frombuffer(b"ACGT", np.uint8)
N = ord("N")


def _tpr(L):
    lpr, _, rpc = GEOMETRY[L]
    return rpc * lpr // 64


def _read(seq, qual):
    return (b"@s", np.asarray(seq, np.uint8).tobytes(), (np.asarray(qual) + 33).astype(np.uint8).tobytes())


def _window_qual(L, lo, hi):
    """Qualities that BWA_plus trims to the kept window [lo, hi)."""
    q = np.full(L, 2)
    q[lo:hi] = 40
    return q


def _run(batches, args=(), expect=None):
    """Every batch through one HIP and one oracle engine, one submission each: per-read results after each, the counter block at the end.
    expect[b][i] (headline options only): whether read i of batch b must carry the poly-N flag -- the oracle is held to it as well, so a
    case cannot quietly stop being the case it is named for."""
    from oracle_engine import OracleEngine

    opt = parse_args(["-u", "x", "-d", "y", "--min_L", "1"] + list(args))
    R = 256 if max(len(r[1]) for reads in batches for r in reads) <= 256 else 1024
    hip, ora = hip_factory(opt, R, 33), OracleEngine(opt, R, 33)
    try:
        for b, reads in enumerate(batches):
            seq, qual, offset, seg = driver.pack_segments([reads])
            r1, r2 = hip.process(seq, qual, offset, seg), ora.process(seq, qual, offset, seg)
            if expect is not None:
                want = np.asarray(expect[b], bool)
                got = (r2["flags"] & capi.F_POLY_N_SEEN) != 0
                assert (got == want).all(), "batch %d: the oracle's poly-N verdicts are not the constructed ones, first at read %d" % (b, np.nonzero(got != want)[0][0])
            bad = np.nonzero(r1 != r2)[0]
            assert len(bad) == 0, "batch %d (%d reads): first differing read %d: hip=%s oracle=%s seq=%r" % (b, len(reads), bad[0], r1[bad[0]], r2[bad[0]], reads[bad[0]][1])
        c1, c2 = hip.counters(), ora.counters()
        bad = np.nonzero(c1 != c2)[0]
        assert len(bad) == 0, "counter block differs in %d places, first at %d: hip=%d oracle=%d" % (len(bad), bad[0], c1[bad[0]], c2[bad[0]])
    finally:
        hip.close()
        ora.close()


def _plain(rng, L):
    return ACGT[rng.integers(0, 4, L)].copy()


def _hit_read(rng, L, k):
    """"NN" inside the kept window: at a lane seam (positions kC - 1 | kC) for even k, in the middle of lane k for odd k."""
    lpr, C, _ = GEOMETRY[L]
    lanes = (L + C - 1) // C
    k = k % lanes
    p = min(k * C + C // 2 if k % 2 else max(k, 2) * C - 1, L - 3)
    s = _plain(rng, L)
    s[p] = s[p + 1] = N
    return _read(s, _window_qual(L, max(0, p - 20), min(L, p + 22)))


# reads that trip the gate of a step (two N of any case in a lane, or one on each side of a lane seam) and must not hit
DECOYS = ("N.N", "Nn", "nN", "nn", "NN|end", "NN|start", "N_last", "N.N_seam")


def _decoy_read(rng, L, kind, k):
    lpr, C, _ = GEOMETRY[L]
    lanes = (L + C - 1) // C
    k = 1 + k % (lanes - 1)          # a seam with a lane on either side: positions kC - 1 | kC
    s = _plain(rng, L)
    lo, hi = 0, L
    if kind == "N.N":                # two N in one lane, one base between them
        s[k * C - 5] = s[k * C - 3] = N
    elif kind == "N.N_seam":         # the lane's last base and the next lane's second
        s[k * C - 1] = s[k * C + 1] = N
    elif kind in ("Nn", "nN", "nn"): # across the seam: lower case is no N for -n
        s[k * C - 1], s[k * C] = kind.encode()
    elif kind == "NN|end":           # the kept window ends between the two N (at the seam, and inside a lane)
        p = k * C - 1 if k % 2 else k * C - 4
        s[p] = s[p + 1] = N
        lo, hi = max(0, p - 30), p + 1
    elif kind == "NN|start":         # the kept window starts between them
        p = k * C - 1 if k % 2 else k * C - 4
        s[p] = s[p + 1] = N
        lo, hi = p + 1, min(L, p + 31)
    elif kind == "N_last":           # N at the lane's last position and at its first, the next lane starts with a base
        s[k * C - 1] = s[(k - 1) * C] = N
    return _read(s, _window_qual(L, lo, hi))


def _flagged_chunk(rng, L, hit_steps):
    """One chunk in which every step holds a read that trips the gate; the reads of row 2 hit in the steps of `hit_steps`, no other read does.
    -> (reads, expected hits)"""
    rpc, tpr = GEOMETRY[L][2], _tpr(L)
    reads, want = [], []
    for i in range(rpc):
        t, row = i % tpr, i // tpr
        if row == 2 and t in hit_steps:
            reads.append(_hit_read(rng, L, t))
            want.append(True)
        else:
            kind = "N.N" if row == 1 else DECOYS[(row + 3 * t) % len(DECOYS)]
            reads.append(_decoy_read(rng, L, kind, t + row))
            want.append(False)
    return reads, want


def _hit_sets(L):
    tpr = _tpr(L)
    return {"first_and_last": {0, tpr - 1}, "two_in_the_middle": {tpr // 2 - 1, tpr // 2}, "all": set(range(tpr))}


# ---- 1. one chunk, every step flagged, some reads hit --------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["first_and_last", "two_in_the_middle", "all"])
@pytest.mark.parametrize("L", LENGTHS)
def test_every_step_flagged_some_reads_hit(L, which):
    rng = np.random.Generator(np.random.PCG64([11, L, SEED]))
    reads, want = _flagged_chunk(rng, L, _hit_sets(L)[which])
    assert len(reads) == GEOMETRY[L][2]
    _run([reads], expect=[want])


@pytest.mark.parametrize("L", LENGTHS)
def test_every_decoy_at_every_seam(L):
    """Each kind of read that trips the gate without a pair, at every lane seam of the read, one chunk after the other."""
    rng = np.random.Generator(np.random.PCG64([12, L, SEED]))
    lanes = (L + GEOMETRY[L][1] - 1) // GEOMETRY[L][1]
    reads = [_decoy_read(rng, L, kind, k) for k in range(lanes - 1) for kind in DECOYS]
    _run([reads], expect=[[False] * len(reads)])


# ---- 2. partial chunks, several chunks: nothing of a chunk survives into the next ----------------------------------------------------------
@pytest.mark.parametrize("count", list(range(1, 10)) + list(range(57, 66)) + [127, 128, 129])
@pytest.mark.parametrize("L", LENGTHS)
def test_partial_chunks_behind_a_flagged_chunk(L, count):
    """A chunk in which every step was flagged and every read of a row hit, then `count` reads of which one alone holds "NN": the last one, the
    first one, the last of the first chunk or the first of the second."""
    rng = np.random.Generator(np.random.PCG64([13, L, count, SEED]))
    rpc = GEOMETRY[L][2]
    head, head_want = _flagged_chunk(rng, L, _hit_sets(L)["all"])
    batches, expect = [], []
    for at in sorted({count - 1, 0, rpc - 1, rpc} & set(range(count))):
        reads = [_read(_plain(rng, L), _window_qual(L, i % 3, L - i % 5)) for i in range(count)]
        reads[at] = _hit_read(rng, L, at)
        batches.append(head + reads)
        expect.append(head_want + [i == at for i in range(count)])
    _run(batches, expect=expect)


# ---- 3. the recount of a chunk that holds a byte >= 0x80 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LENGTHS)
def test_recount_takes_the_verdicts_again(L):
    """One read of the chunk holds a byte >= 0x80: the chunk is taken back, patched and counted again, the flagged steps looked at again.  "NN"
    sits in another read of the same step and in a read of another step; one read holds N, the byte, N -- no pair before the patch or after it."""
    rng = np.random.Generator(np.random.PCG64([14, L, SEED]))
    rpc, tpr, C = GEOMETRY[L][2], _tpr(L), GEOMETRY[L][1]
    batches, expect = [], []
    for step in (0, tpr - 1):
        reads = [_read(_plain(rng, L), _window_qual(L, i % 3, L - i % 5)) for i in range(rpc)]
        want = [False] * rpc
        s = _plain(rng, L)
        s[C + 2] = 0x80 + 7 * step
        reads[step] = _read(s, _window_qual(L, 0, L))
        reads[step + tpr] = _hit_read(rng, L, step)                    # the same step, the next row
        reads[(step + 1) % tpr + 2 * tpr] = _hit_read(rng, L, step + 1)  # another step
        want[step + tpr] = want[(step + 1) % tpr + 2 * tpr] = True
        for p in (C - 2, 2 * C - 1):                                   # inside a lane, and with the byte on the far side of a seam
            s = _plain(rng, L)
            s[p - 1], s[p], s[p + 1] = N, 0xC1, N
            reads[(step + 2) % tpr + tpr * (1 if p < C else 2)] = _read(s, _window_qual(L, 0, L))
        batches.append(reads)
        expect.append(want)
    # ... and behind a chunk whose every step was flagged, with the patched read and the pair in the partial chunk
    head, head_want = _flagged_chunk(rng, L, _hit_sets(L)["first_and_last"])
    batches.append(head + batches[0][:tpr + 1])
    expect.append(head_want + expect[0][:tpr + 1])
    _run(batches, expect=expect)


# ---- 4. reads judged without being counted, and the variants beside the headline one, at -n 2 ----------------------------------------------
def _seam_reads(rng, L):
    """"NN" across every lane seam of the read and the pairs that must not trip there, under a window that holds the pair, one that ends
    between the two and one that starts between them."""
    lpr, C, _ = GEOMETRY[L]
    reads = []
    for p in [k * C - 1 for k in range(1, lpr) if k * C < L - 1]:
        for pat in (b"NN", b"N.N", b"nN", b"Nn"):
            s = _plain(rng, L)
            second = p + len(pat) - 1
            s[p], s[second] = pat[0], pat[-1]
            for lo, hi in ((max(0, p - 25), min(L, second + 26)), (max(0, p - 30), p + 1), (second, min(L, second + 30))):
                reads.append(_read(s, _window_qual(L, lo, hi)))
    return reads


VARIANTS = {
    "judged_uncounted": ["--avg_q", "40.5"],      # no read reaches the average: every read is judged for poly-N without being counted (chk)
    "avg_q": ["--avg_q", "20"],                    # EXT, some reads fail the average
    "trim5_mid_lane": ["--5end", "7"],             # WINDOWED: the window starts in the middle of the first lane
    "trim5_trim3": ["--5end", "3", "--3end", "9"], # WINDOWED, both ends
    "avg_q_trim5": ["--avg_q", "20", "--5end", "7"],
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("L", LENGTHS)
def test_seam_pairs_in_the_other_variants(L, variant):
    rng = np.random.Generator(np.random.PCG64([15, L, SEED]))
    reads = _seam_reads(rng, L)
    chunk, _ = _flagged_chunk(rng, L, _hit_sets(L)["two_in_the_middle"])
    order = rng.permutation(len(reads))
    _run([chunk + reads, [reads[i] for i in order] + chunk], VARIANTS[variant])


# ---- 5. any other -n: the path that judges behind the loop from the staged bases is not touched ---------------------------------------------
@pytest.mark.parametrize("poly_n", ["0", "3"])
def test_other_poly_n_lengths_answer_as_before(poly_n):
    L = 150
    rng = np.random.Generator(np.random.PCG64([16, L, SEED]))
    chunks = [_flagged_chunk(rng, L, hs)[0] for hs in _hit_sets(L).values()]
    runs = []
    for k in (2, 3, 4):  # runs of 2, 3 and 4 N across a seam and inside a lane
        for p in (18, 19 * 3 + 6):
            s = _plain(rng, L)
            s[p:p + k] = N
            runs.append(_read(s, _window_qual(L, 0, L)))
            runs.append(_read(s, _window_qual(L, p + 1, L)))
    _run([chunks[0] + runs, chunks[1] + chunks[2] + _seam_reads(rng, L)], ["-n", poly_n])
