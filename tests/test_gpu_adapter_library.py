"""Adapter / contaminant libraries past one group of the pre-pass (more than 64 targets, or targets of more than 8 192 bases): the HIP
path against the CPU oracle, per read and the whole counter block (adapter_stats included), bit-exact, on seeded libraries and reads; the
group boundaries by hand; the native command line against the real reference on a committed library; and the limits."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from faqcs_amd import _capi as capi
from faqcs_amd.options import BUILTIN_ADAPTERS, parse_args, reverse_complement
from test_gpu_parity import SEED, compare_engines, hip_factory

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBRARY_FA = os.path.join(ROOT, "tests", "golden", "adapter_library", "library.fa")
ACGT = np.frombuffer(b"ACGT", np.uint8)
IUPAC = np.frombuffer(b"RYSWKMBDHVN", np.uint8)


def _rand_target(rng, n, iupac=0.03):
    s = ACGT[rng.integers(0, 4, n)].copy()
    k = rng.random(n) < iupac
    s[k] = IUPAC[rng.integers(0, len(IUPAC), int(k.sum()))]
    return s.tobytes().decode()


def random_library(rng, n, lo=12, hi=80):
    """The built-in adapters, then random lo ... hi-mers with IUPAC codes and reverse complements of earlier targets: n targets."""
    lib = list(BUILTIN_ADAPTERS)[:n]
    while len(lib) < n:
        if rng.random() < 0.2:
            j = int(rng.integers(0, len(lib)))
            lib.append(("rc%d" % len(lib), reverse_complement(lib[j][1])))
        else:
            lib.append(("t%d" % len(lib), _rand_target(rng, int(rng.integers(lo, hi + 1)))))
    return lib


def _plant(rng, s, target, mutate=0.04):
    """s with a piece of `target` (IUPAC codes resolved to a base they match) written over a random place, a few bases mutated."""
    t = np.frombuffer(target.upper().encode(), np.uint8).copy()
    amb = ~np.isin(t, ACGT)
    t[amb] = ACGT[rng.integers(0, 4, int(amb.sum()))]
    L = len(s)
    k = int(rng.integers(min(10, len(t)), len(t) + 1))
    a = int(rng.integers(0, len(t) - k + 1))
    piece = t[a:a + k][:L]
    mut = rng.random(len(piece)) < mutate
    piece[mut] = ACGT[rng.integers(0, 4, int(mut.sum()))]
    p = int(rng.integers(-len(piece) // 3, L - 2 * len(piece) // 3 + 1))  # (partial overlaps at either end of the read)
    lo, hi = max(p, 0), min(p + len(piece), L)
    s[lo:hi] = piece[lo - p:hi - p]


def library_reads(rng, lib, n, shape, plant_from=64, frac=0.45):
    """n reads of `shape` (a length, or (lo, hi) for ragged lengths); a fraction carries a piece of a target of index >= plant_from."""
    import make_fixtures

    reads = []
    for i in range(n):
        L = shape if isinstance(shape, int) else int(rng.integers(shape[0], shape[1] + 1))
        if i % 4 == 3:
            s, q = make_fixtures._adv_read(rng, L)
            s, q = s.copy(), q.copy()
        else:
            s = ACGT[rng.integers(0, 4, L)].copy()
            q = (rng.integers(15, 42, L) + 33).astype(np.uint8)
        if len(s) and rng.random() < frac:
            j = int(rng.integers(min(plant_from, len(lib) - 1), len(lib)))
            _plant(rng, s, lib[j][1])
            if rng.random() < 0.3:  # a second target in the same read: masks of two groups
                _plant(rng, s, lib[int(rng.integers(0, len(lib)))][1])
        reads.append((b"@a", s.tobytes(), q.tobytes()))
    return reads


def options(args, lib):
    opt = parse_args(["-u", "x", "-d", "y", "--adapter"] + args)
    opt.adapter = list(lib)
    return opt


def _credited(hip):
    """adapter_stats of the HIP engine's counter block: reads credited per target."""
    lay = capi.python_layout(hip.holder.max_read_length, hip.holder.n_adapters)
    o, n = lay["adapter_stats"]
    return hip.counters()[o:o + n:2]


OPTS = {"default": [], "rate0.3": ["--rate", "0.3"], "qc_only": ["--qc_only"], "ends": ["--5end", "4", "--3end", "3", "--min_L", "20"]}
LONG = (1025, 9000)


@pytest.mark.parametrize("n_targets,shape,n_reads,opts", [
    (65, 150, 400, "default"), (65, 150, 300, "rate0.3"), (65, 150, 300, "qc_only"), (65, 150, 300, "ends"),
    (200, 150, 300, "default"), (200, 300, 120, "rate0.3"), (200, 1024, 40, "default"), (200, LONG, 24, "ends"),
    (1000, 150, 160, "default"), (1000, 300, 60, "qc_only"), (1000, 1024, 20, "rate0.3")],
    ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_library_matches_oracle(n_targets, shape, n_reads, opts):
    rng = np.random.Generator(np.random.PCG64([61, n_targets, shape if isinstance(shape, int) else 1, n_reads, SEED]))
    lib = random_library(rng, n_targets)
    reads = library_reads(rng, lib, n_reads, shape)
    R = 256 if shape == 150 else (1024 if isinstance(shape, int) else 9000)
    hip, _ = compare_engines(options(OPTS[opts], lib), reads, R=R, seg_size=37)  # ragged segments: tail groups of 8 reads
    assert _credited(hip)[64:].sum() > 0, "no read was credited to a target past the first group"


def test_stale_range_across_the_group_boundary():
    """Target 63 (last of group 1) masks the read; target 64 (first of group 2) has no matching cell (reads of G / T only, a target of
    A / C only), so the reference reuses target 63's range (H2) -- the range is carried over the boundary."""
    rng = np.random.Generator(np.random.PCG64([62, SEED]))
    lib = random_library(rng, 63, 20, 40)
    t63 = "T" * 30 + "GT" * 6
    lib.append(("t63", t63))
    lib.append(("ac", "ACCACACAACCA" * 2))             # 64: shares no base with a read of G / T only ...
    lib.extend(random_library(rng, 40, 20, 40)[9:])    # ... and a later group
    reads = []
    for i in range(48):
        L = int(rng.integers(60, 151))
        s = np.frombuffer(b"GT", np.uint8)[rng.integers(0, 2, L)].copy()
        if i % 2 == 0:
            _plant(rng, s, t63, mutate=0.0)
        reads.append((b"@s", s.tobytes(), bytes([33 + 37]) * L))
    reads += library_reads(rng, lib, 40, 150, plant_from=60)
    for args in ([], ["--rate", "0.5"]):
        compare_engines(options(args, lib), reads, R=256, seg_size=13)


def test_equal_best_scores_in_two_groups_keep_the_earlier_target():
    """The same sequence at index 10 (group 1) and 100 (group 2), and again at 140: every credit goes to index 10 (strict >)."""
    rng = np.random.Generator(np.random.PCG64([63, SEED]))
    lib = random_library(rng, 150, 20, 60)
    dup = _rand_target(rng, 36, 0.0)
    for j in (10, 100, 140):
        lib[j] = ("dup%d" % j, dup)
    reads = []
    for i in range(200):
        s = ACGT[rng.integers(0, 4, 150)].copy()
        if i % 2 == 0:
            _plant(rng, s, dup, mutate=0.0 if i % 4 else 0.05)
        reads.append((b"@d", s.tobytes(), bytes([33 + 36]) * 150))
    hip, _ = compare_engines(options([], lib), reads, R=256, seg_size=29)
    cr = _credited(hip)
    assert cr[10] > 0 and cr[100] == 0 and cr[140] == 0, (cr[10], cr[100], cr[140])


def test_whole_group_skipped_then_a_target_without_a_matching_cell():
    """Group 1 of random 60 ... 80-mers that every read meets somewhere but none can reach (the whole-read skip, which leaves "stale range
    of target 63, not yet computed"); target 64 shares no base with the reads, target 65 neither: the range of target 63 has to be computed
    in the next group's launch from the earlier group's target."""
    rng = np.random.Generator(np.random.PCG64([64, SEED]))
    lib = [("g%d" % j, _rand_target(rng, int(rng.integers(60, 81)), 0.0)) for j in range(64)]
    lib += [("cc", "C" * 25), ("cc2", "CCCCGGGGCCCC"), ("tail", _rand_target(rng, 30, 0.0))]
    lib += random_library(rng, 80, 20, 50)[9:]
    reads = []
    for i in range(160):
        L = int(rng.integers(20, 151))
        s = np.frombuffer(b"AT", np.uint8)[rng.integers(0, 2, L)].copy()  # no C / G: targets 64 and 65 have no matching cell
        if i % 3 == 0:  # a piece of target 63 (with its C / G turned into A / T) so that its stale range masks
            t = np.frombuffer(lib[63][1].encode(), np.uint8).copy()
            t[(t == ord("C")) | (t == ord("G"))] = ord("A")
            _plant(rng, s, t.tobytes().decode(), mutate=0.0)
        reads.append((b"@w", s.tobytes(), bytes([33 + 35]) * L))
    for args in ([], ["--rate", "0.6"], ["--rate", "0.9"]):
        compare_engines(options(args, lib), reads, R=256, seg_size=11)


def test_bad_base_against_a_library_of_200_targets():
    """A read with a base the aligner rejects, aligned against 200 targets (four groups): FAQCS_F_ERR_BASE on that read and on no
    other, and the submission fails with FAQCS_E_BASE, as with one group; the batch without it matches the oracle."""
    import ctypes as C

    from faqcs_amd import driver

    rng = np.random.Generator(np.random.PCG64([65, SEED]))
    lib = random_library(rng, 200)
    reads = library_reads(rng, lib, 40, 150)
    s = bytearray(reads[17][1])
    s[5] = ord("X")
    bad = (reads[17][0], bytes(s), reads[17][2])
    seq, qual, offset, seg = driver.pack_segments([reads[:17] + [bad] + reads[18:]])
    hip = hip_factory(options([], lib), 256, 33)
    res = np.zeros(len(reads), dtype=capi.RESULT_DTYPE)
    b = capi.Batch(seq.ctypes.data, qual.ctypes.data, offset.ctypes.data, len(reads), len(seg) - 1, seg.ctypes.data, 0, None)
    assert hip.lib.faqcs_submit(hip.ctx, C.byref(b), res.ctypes.data) == 0
    assert hip.lib.faqcs_sync(hip.ctx) == capi.E_BASE
    flagged = np.nonzero(res["flags"] & capi.F_ERR_BASE)[0]
    assert list(flagged) == [17], flagged
    compare_engines(options([], lib), reads[:17] + reads[18:], R=256, seg_size=9)


@pytest.mark.parametrize("tlen", [8193, 16384, 32767])
@pytest.mark.parametrize("shape,n_reads", [(150, 60), (300, 30), (5000, 8)])
@pytest.mark.parametrize("with_short", [False, True], ids=["alone", "with_short"])
def test_long_targets_match_oracle(tlen, shape, n_reads, with_short):
    rng = np.random.Generator(np.random.PCG64([66, tlen, shape, with_short, SEED]))
    long_t = _rand_target(rng, tlen, 0.002)
    lib = ([("builtin%d" % j, s) for j, (_, s) in enumerate(BUILTIN_ADAPTERS)] if with_short else []) + [("long", long_t)]
    if with_short:
        lib += random_library(rng, 20, 12, 60)[9:]
    reads = library_reads(rng, lib, n_reads, shape, plant_from=0, frac=0.0)
    for i in range(0, n_reads, 2):  # segments of the long target planted into every other read: a whole read's worth, or a piece
        s = np.frombuffer(reads[i][1], np.uint8).copy()
        if i % 4 == 0:
            a = int(rng.integers(0, tlen - len(s)))
            t = np.frombuffer(long_t[a:a + len(s)].upper().encode(), np.uint8).copy()
            t[~np.isin(t, ACGT)] = ord("A")
            mut = rng.random(len(s)) < 0.02
            t[mut] = ACGT[rng.integers(0, 4, int(mut.sum()))]
            s[:] = t
        else:
            _plant(rng, s, long_t[int(rng.integers(0, tlen - 400)):][:400])
        reads[i] = (reads[i][0], s.tobytes(), reads[i][2])
    R = 256 if shape == 150 else (1024 if shape <= 1024 else 8192)
    hip, _ = compare_engines(options([], lib), reads, R=R, seg_size=9)  # (a tail group takes the whole target as its threshold)
    assert _credited(hip)[[n for n, _ in lib].index("long")] > 0


_REF_BIN = os.path.join(ROOT, "oracle", "_ref", "FaQCs_ref")
_HIP_REF_BIN = os.path.join(ROOT, "oracle", "_ref", "FaQCs_hip")
_CLI_BIN = os.path.join(ROOT, "faqcs_amd", "faqcs_mi")


def test_native_cli_with_a_contaminant_library_equals_the_reference(tmp_path):
    """faqcs_mi and the reference's own driver linked against the library (FaQCs_hip) with --artifactFile pointing at the committed
    200-record library (a 20 000-base record wrapped over many lines, duplicate deflines, lower case): every output file byte-identical
    to the real reference's on seeded 2x150 pairs that carry pieces of the library."""
    if not os.path.exists(_REF_BIN):
        pytest.skip("oracle/_ref/FaQCs_ref not built (needs the reference sources at build time: make -C oracle ref)")
    import make_fixtures

    from faqcs_amd.options import parse_artifact_file

    lib = parse_artifact_file(LIBRARY_FA)
    rng = np.random.Generator(np.random.PCG64([67, SEED]))
    p1, p2 = str(tmp_path / "l_1.fastq"), str(tmp_path / "l_2.fastq")
    r1, r2 = [], []
    for i in range(2500):
        for rr in (r1, r2):
            s, q = make_fixtures._adv_read(rng, 150)
            s = s.copy()
            if len(s) >= 20 and rng.random() < 0.4:
                j = 0 if rng.random() < 0.3 else int(rng.integers(1, len(lib)))
                t = lib[j][1]
                a = int(rng.integers(0, max(1, len(t) - 150)))
                _plant(rng, s, t[a:a + 150])
            rr.append((b"@P%d" % i, s.tobytes(), q.tobytes()))
    make_fixtures.write_fastq(p1, r1)
    make_fixtures.write_fastq(p2, r2)
    bins = [("ref", _REF_BIN), ("mi", _CLI_BIN)] + ([("hip", _HIP_REF_BIN)] if os.path.exists(_HIP_REF_BIN) else [])
    outs = {}
    for name, binary in bins:
        out = str(tmp_path / name)
        for _ in range(6):  # (the reference can die of SIGPIPE feeding the absent R: see make_golden.py)
            subprocess.run(["rm", "-rf", out])
            r = subprocess.run([binary, "-1", p1, "-2", p2, "-d", out, "--debug", "-t", "1", "--artifactFile", LIBRARY_FA],
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
            if r.returncode != -13:
                break
        assert r.returncode == 0, (name, r.returncode, r.stderr.decode(errors="replace")[-800:])
        outs[name] = {fn: hashlib.md5(open(os.path.join(out, fn), "rb").read()).hexdigest() for fn in sorted(os.listdir(out)) if not fn.endswith(".pdf")}
    stats = [fn for fn in outs["ref"] if fn.endswith("stats.txt")]
    assert stats
    for name in outs:
        assert outs[name].keys() == outs["ref"].keys(), (name, sorted(outs[name]), sorted(outs["ref"]))
        bad = [fn for fn in outs["ref"] if outs["ref"][fn] != outs[name][fn]]
        assert not bad, (name, bad)
    assert any(b"primer_" in open(os.path.join(str(tmp_path / "ref"), fn), "rb").read() or b"vector_backbone" in
               open(os.path.join(str(tmp_path / "ref"), fn), "rb").read() for fn in stats), "no library record was credited"


def test_library_limits():
    """65 534 targets are taken (and a read credited to the last of them), 65 535 are refused; a 32 767-base target is taken, 32 768
    bases are refused -- loudly, never truncated; the counter layout of 65 534 targets is the python statement's."""
    import ctypes

    from faqcs_amd import driver
    from faqcs_amd.engine import FaqcsError

    rng = np.random.Generator(np.random.PCG64([68, SEED]))
    n = 65534
    lib = [("m%d" % j, _rand_target(rng, 12, 0.0)) for j in range(n)]
    last = _rand_target(rng, 40, 0.0)
    lib[-1] = ("last", last)
    s = ACGT[rng.integers(0, 4, 150)].copy()
    s[50:90] = np.frombuffer(last.encode(), np.uint8)
    reads = [(b"@l", s.tobytes(), bytes([33 + 38]) * 150)]
    seq, qual, offset, seg = driver.pack_segments([reads])
    hip = hip_factory(options([], lib), 256, 33)
    res = hip.process(seq, qual, offset, seg)
    assert res["adapter"][0] == n  # 1 + index of the last target
    lay = capi.Layout()
    assert hip.lib.faqcs_counters_layout(256, n, ctypes.byref(lay)) == 0
    py = capi.python_layout(256, n)
    assert int(lay.adapter_stats) == py["adapter_stats"][0] and int(lay.total) == py["total"]
    with pytest.raises(FaqcsError) as e:
        hip_factory(options([], lib + [("one_more", "ACGTACGTACGT")]), 256, 33)
    assert "65534" in str(e.value)
    hip_factory(options([], [("longest", _rand_target(rng, 32767, 0.0))]), 256, 33)
    with pytest.raises(FaqcsError) as e:
        hip_factory(options([], [("too_long", _rand_target(rng, 32768, 0.0))]), 256, 33)
    assert "32768" in str(e.value)

