"""Diagnostic (not a test): A/B of two faqcs_mi binaries end to end, e.g. the parent commit's against the tree's, on the files
tools/e2e_big.py generates (synthetic 2x150 FASTQ in /dev/shm, also as gzip and as bgzip): five input shapes, the two binaries
alternate on the same files, `reps` runs each.  The second binary's median is set against the first one's own min - max range of the
same call; a range wider than 15 % of its median decides nothing.
python tools/e2e_ab.py <faqcs_mi A> <faqcs_mi B> [pairs] [reps]      -> profiles/cli_stream/ab_e2e.txt"""
import os
import statistics
import struct
import subprocess
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_fixtures  # noqa: E402

n = int(float(sys.argv[3])) if len(sys.argv) > 3 else 8_000_000
REPS = int(sys.argv[4]) if len(sys.argv) > 4 else 5
L = 150
base = "/dev/shm/faqcs_ab_e2e"
os.makedirs(base, exist_ok=True)


def say(s):
    print(s, flush=True)


blk = 500_000
seqs, quals = make_fixtures.headline_arrays(2 * blk, L)  # (as tools/e2e_big.py)
paths = []
for mate in (1, 2):
    p = os.path.join(base, "r%d.fq" % mate)
    paths.append(p)
    with open(p, "wb") as f:
        done = 0
        while done < n:
            m = min(blk, n - done)
            idw = 9
            head = np.frombuffer(b"@SYN:", np.uint8)
            tail = np.frombuffer(b"/%d\n" % mate, np.uint8)
            a = np.empty((m, len(head) + idw + len(tail) + L + 3 + L + 1), np.uint8)
            c = 0
            a[:, c:c + len(head)] = head; c += len(head)
            ids = np.arange(done, done + m, dtype=np.int64)
            for k in range(idw):
                a[:, c + idw - 1 - k] = 48 + (ids // 10 ** k) % 10
            c += idw
            a[:, c:c + len(tail)] = tail; c += len(tail)
            lo = (mate - 1) * blk
            a[:, c:c + L] = seqs[lo:lo + m]; c += L
            a[:, c:c + 3] = np.frombuffer(b"\n+\n", np.uint8); c += 3
            a[:, c:c + L] = quals[lo:lo + m]; c += L
            a[:, c] = 10
            a.tofile(f)
            done += m
say("generated %d pairs" % n)


def member(raw):
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    body = c.compress(raw) + c.flush()
    return struct.pack("<4BI2BH2BHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, 12 + 6 + len(body) + 8 - 1) + body + struct.pack("<II", zlib.crc32(raw) & 0xffffffff, len(raw))


gz = {"bgzf": [], "gzip": []}
with ThreadPoolExecutor(16) as pool:
    for p in paths:
        data = open(p, "rb").read()
        blocks = [data[o:o + 65280] for o in range(0, len(data), 65280)] + [b""]
        with open(p + ".bgzf.gz", "wb") as f:
            for m in pool.map(member, blocks, chunksize=64):
                f.write(m)
        gz["bgzf"].append(p + ".bgzf.gz")
        c = zlib.compressobj(1, zlib.DEFLATED, 31)
        with open(p + ".plain.gz", "wb") as f:
            for o in range(0, len(data), 1 << 24):
                f.write(c.compress(data[o:o + (1 << 24)]))
            f.write(c.flush())
        gz["gzip"].append(p + ".plain.gz")
        del data
say("compressed")

bins = [("parent", os.path.abspath(sys.argv[1])), ("change", os.path.abspath(sys.argv[2]))]
shapes = [("mapped", ["-1", paths[0], "-2", paths[1]], {}, 2 * n),
          ("forced streaming", ["-1", paths[0], "-2", paths[1]], {"FAQCS_MI_STREAMING": "1"}, 2 * n),
          ("gzip", ["-1", gz["gzip"][0], "-2", gz["gzip"][1]], {}, 2 * n),
          ("bgzip", ["-1", gz["bgzf"][0], "-2", gz["bgzf"][1]], {}, 2 * n),
          ("one gzip file unpaired", ["-u", gz["gzip"][0]], {}, n)]
out = os.path.join(base, "out")
rows = []
for shape, inputs, env, reads in shapes:
    t = {"parent": [], "change": []}
    for rep in range(REPS):
        for name, cli in bins:
            subprocess.run(["rm", "-rf", out])
            t0 = time.perf_counter()
            r = subprocess.run([cli] + inputs + ["-d", out, "--ascii", "33", "-q", "5", "--min_L", "50", "--trim_only"],
                               env=dict(os.environ, **env), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=120)
            dt = time.perf_counter() - t0
            if r.returncode != 0:  # nothing more on the GPU after a failure
                say("%s %s: rc %d\n%s" % (shape, name, r.returncode, r.stderr.decode(errors="replace")[-800:]))
                subprocess.run(["rm", "-rf", base])
                sys.exit(1)
            t[name].append(reads / dt / 1e6)
    p, c = sorted(t["parent"]), sorted(t["change"])
    med_p, med_c = statistics.median(p), statistics.median(c)
    width = (p[-1] - p[0]) / med_p
    verdict = "not decided (parent's range is %.0f %% of its median)" % (100 * width) if width > 0.15 else ("within" if p[0] <= med_c <= p[-1] else ("above the parent's range" if med_c > p[-1] else "BELOW the parent's range"))
    rows.append((shape, p, c, med_p, med_c, verdict))
    say("%-24s parent %s  change %s" % (shape, " ".join("%.1f" % x for x in t["parent"]), " ".join("%.1f" % x for x in t["change"])))
say("")
say("M reads/s, %d runs each, alternating, %d pairs 2x%d, wall time of the whole process" % (REPS, n, L))
say("%-24s %-28s %-10s %s" % ("shape", "parent min / median / max", "change med", "change's median against the parent's range"))
for shape, p, c, med_p, med_c, verdict in rows:
    say("%-24s %5.1f / %5.1f / %5.1f          %5.1f      %s" % (shape, p[0], med_p, p[-1], med_c, verdict))
subprocess.run(["rm", "-rf", base])
