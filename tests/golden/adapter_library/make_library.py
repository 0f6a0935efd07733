"""Writes library.fa next to this file: the ~200-record contaminant library of tests/test_gpu_adapter_library.py (a seeded, hand-shaped
--artifactFile).  One 20 000-base record wrapped over many lines, random 12 ... 80-mers with IUPAC codes, reverse complements, lower-case
bases and a few deflines that occur twice (the adapter stats merge by name)."""
import os

import numpy as np

IUPAC = b"RYSWKMBDHVN"
COMP = bytes.maketrans(b"ACGTacgtRYSWKMBDHVNryswkmbdhvn", b"TGCAtgcaYRSWMKVHDBNyrswmkvhdbn")


def records(seed=20261016):
    rng = np.random.Generator(np.random.PCG64(seed))
    acgt = np.frombuffer(b"ACGT", np.uint8)

    def rand(n, iupac=0.03):
        s = acgt[rng.integers(0, 4, n)].copy()
        k = rng.random(n) < iupac
        s[k] = np.frombuffer(IUPAC, np.uint8)[rng.integers(0, len(IUPAC), int(k.sum()))]
        return s.tobytes()

    long_rec = bytearray(rand(20000, 0.001))
    long_rec[5000:5600] = long_rec[5000:5600].lower()
    out = [(b"vector_backbone_20k", bytes(long_rec))]
    for i in range(1, 200):
        u = rng.random()
        if u < 0.2 and len(out) > 2:
            j = int(rng.integers(1, len(out)))
            out.append((b"rc_of_%d" % j, out[j][1].translate(COMP)[::-1][:80]))
        else:
            s = rand(int(rng.integers(12, 81)))
            if rng.random() < 0.1:
                s = s.lower()
            out.append((b"primer_%d" % i, s))
    for i in (17, 90, 151):  # duplicate deflines: the stats of both records go to one name
        out[i] = (out[i - 1][0], out[i][1])
    return out


def write(path):
    with open(path, "wb") as f:
        for name, s in records():
            f.write(b">" + name + b" test library record\n")
            for k in range(0, len(s), 70):
                f.write(s[k:k + 70] + b"\n")


if __name__ == "__main__":
    write(os.path.join(os.path.dirname(os.path.abspath(__file__)), "library.fa"))
