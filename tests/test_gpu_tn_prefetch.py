"""trim_lds fetches a read's terminal-N flags byte a whole chunk before the chunk that uses it (with the chunk's offsets), and carries
it to the next iteration of the wave's chunk loop.  A byte fetched for the wrong chunk, or for the wrong read of the right chunk, gives a
read that starts or ends with N the treatment of one that does not (and the other way round), so these tests put such reads on the chunk
boundaries -- the last two reads of a chunk and the first two of the next, the last read of a launch -- of batches big enough for every
wave to take a second chunk, and of launches of one read, fewer than a chunk, exactly one chunk and a chunk and a bit; with the batch's flags
and without them (the kernel then looks at the two bases itself), at 150 bases (8 lanes per read, chunks of 64 reads) and at 250 bases
(16 lanes per read, chunks of 32).  HipEngine against the oracle, bit-exact, per-read results and counter block."""
import numpy as np
import pytest

from faqcs_amd import _capi as capi
from faqcs_amd.options import parse_args

SEED = int(__import__("os").environ.get("FAQCS_TEST_SEED", "0"))

# reads per chunk of the trim_lds variant that takes reads of this length, and the waves (= chunks per group) of its blocks
RPC = {150: 64, 250: 32}
NW = 12
# a wave takes a second chunk only when its block takes a second group: more groups than the device has compute units (256 on an MI355X)
MAX_CU = 256


def boundary_batch(n, L, seed):
    """n reads of L - 5 ... L random bases with quality 40 throughout.  Reads on the chunk boundaries of about half of the chunks, the first
    and the last read of the batch among them, start with 1 ... 3 upper-case N, end with 1 ... 3, or both.  Returns (reads, lead, trail):
    the N runs put at the two ends of every read (0 for most)."""
    rng = np.random.Generator(np.random.PCG64([23, n, L, seed, SEED]))
    rpc = RPC[L]
    lens = rng.integers(L - 5, L + 1, n)
    off = np.concatenate([[0], np.cumsum(lens)])
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(off[-1]))].copy()
    qual = np.full(int(off[-1]), 33 + 40, np.uint8)
    lead = np.zeros(n, np.int64)
    trail = np.zeros(n, np.int64)
    n_chunks = (n + rpc - 1) // rpc
    marked = np.nonzero(rng.random(n_chunks) < 0.5)[0]
    idx = np.concatenate([marked * rpc + d for d in (-2, -1, 0, 1)] + [np.array([0, n - 1])])
    idx = np.unique(idx[(idx >= 0) & (idx < n)])
    kind = rng.integers(1, 4, len(idx))  # 1: starts with N, 2: ends with N, 3: both
    lead[idx] = np.where(kind & 1, rng.integers(1, 4, len(idx)), 0)
    trail[idx] = np.where(kind & 2, rng.integers(1, 4, len(idx)), 0)
    for i in idx:
        seq[off[i]:off[i] + lead[i]] = ord("N")
        seq[off[i + 1] - trail[i]:off[i + 1]] = ord("N")
    reads = [(b"@x", seq[off[i]:off[i + 1]].tobytes(), qual[off[i]:off[i + 1]].tobytes()) for i in range(n)]
    return reads, lead, trail


def launch_sizes(L):
    rpc = RPC[L]
    big = 2 * MAX_CU * NW * rpc + 3 * rpc + 7  # every wave of every block takes two chunks, some a third; the last chunk is a partial one
    return [1, rpc - 24, rpc - 1, rpc, rpc + 1, 2 * rpc, big]


def oracle_run(opt, reads, R=256):
    from oracle_engine import OracleEngine

    from faqcs_amd import driver

    seq, qual, offset, seg = driver.pack_segments([reads])
    ora = OracleEngine(opt, R, 33)
    return (seq, qual, offset, seg), ora.process(seq, qual, offset, seg), ora.counters()


@pytest.mark.parametrize("L", [150, 250])
def test_the_oracle_trims_the_terminal_n_runs_of_these_batches(L):
    """(no GPU) What the GPU tests below compare against: on these inputs -- quality 40 everywhere, so that nothing but the terminal-N rule
    (mask_quality_terminal_N: the quality of an N run at either end reads as 0) can make BWA_plus cut -- the oracle keeps exactly the
    bases between the two N runs of a marked read and all of every other read."""
    opt = parse_args(["-u", "x", "-d", "y", "--ascii", "33"])
    for n in launch_sizes(L)[:-1] + [40 * RPC[L] + 5]:
        reads, lead, trail = boundary_batch(n, L, 1)
        _, res, _ = oracle_run(opt, reads)
        lens = np.array([len(r[1]) for r in reads])
        assert (lead + trail > 0).any() and lead[n - 1] + trail[n - 1] > 0
        assert ((res["flags"] & 1) == 1).all()
        assert (res["start"] == lead).all()
        assert (res["len"] == lens - lead - trail).all()


@pytest.mark.gpu
@pytest.mark.parametrize("use_flags", [True, False], ids=["flags", "noflags"])
@pytest.mark.parametrize("L", [150, 250])
def test_terminal_n_reads_on_chunk_boundaries_match_the_oracle(L, use_flags):
    from faqcs_amd import driver
    from faqcs_amd.engine import HipEngine

    opt = parse_args(["-u", "x", "-d", "y", "--ascii", "33"])
    for k, n in enumerate(launch_sizes(L)):
        reads, lead, trail = boundary_batch(n, L, k)
        (seq, qual, offset, seg), want, want_counters = oracle_run(opt, reads)
        assert (want["start"] == lead).all()  # (the terminal-N runs are what is trimmed: see the test above)
        flags = driver.terminal_n_flags(seq, offset) if use_flags else None
        if use_flags:
            assert ((flags & 1) == (lead > 0)).all() and ((flags >> 1) == (trail > 0)).all()
        hip = HipEngine(opt, 256, 33, device=0)
        got = hip.process(seq, qual, offset, seg, flags)
        kt = capi.KernelTimes()
        hip.lib.faqcs_kernel_report(hip.ctx, __import__("ctypes").byref(kt))
        assert (kt.trim_kernel or b"").decode() == "trim_lds"
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, "%d reads: %d differ, the first is read %d (read %d of chunk %d): hip=%s oracle=%s" % (
            n, len(bad), bad[0], bad[0] % RPC[L], bad[0] // RPC[L], got[bad[0]], want[bad[0]])
        assert (hip.counters() == want_counters).all(), "%d reads: counter block" % n
