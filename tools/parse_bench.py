"""Diagnostic (not a test): faqcs_parse_device on a device-resident FASTQ text of 2x150-shaped records just under 4 GiB, against a
device-to-device copy of the same text in the same run, and against faqcs_parse_host over the same text cut into ranges on 16 threads
(what the command line's host parse pays today).  Prints one JSON line; --out FILE also writes it there.

    python tools/parse_bench.py [--records N] [--reps 7] [--host-threads 16] [--out profiles/parse/parse_bench.json]

The text is built on the device from faqcs_synth_fill arenas with fixed-width deflines (synth_text below).  Index +
records and gather are timed apart (HIP events on the library's compute stream, median of --reps after a warm-up); GB/s counts the text
once."""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEF_WIDTH = 16  # '@' + 15 hex digits of the record's index


def record_bytes(L, W=DEF_WIDTH):
    return W + 1 + L + 1 + 2 + L + 1  # defline \n bases \n + \n qualities \n


def synth_text(lib, dev, n, L=150, W=DEF_WIDTH, seed=20260101):
    """n records of L synthetic bases (faqcs_synth_fill) as FASTQ text in device memory.  -> (storage tensor whose byte 64 is the text's
    byte 0, with 64 spare bytes behind; n_text; the base arena and the quality arena the text was made from, [n, L] each)"""
    import torch

    from faqcs_amd.engine import _check

    R = record_bytes(L, W)
    seq = torch.empty(n * L + 192, dtype=torch.uint8, device=dev)
    qual = torch.empty_like(seq)
    piece, done = (1 << 31) // L, 0
    while done < n:  # (filled in pieces of whole reads: the generator's offsets are 32 bits wide)
        m = min(piece, n - done)
        scratch = torch.empty(m + 1, dtype=torch.int32, device=dev)
        _check(lib, lib.faqcs_synth_fill(0, seq.data_ptr() + 64 + done * L, qual.data_ptr() + 64 + done * L, scratch.data_ptr(), m, L, seed, done, 0.0))
        done += m
    torch.cuda.synchronize()
    store = torch.full((64 + n * R + 64,), 10, dtype=torch.uint8, device=dev)  # (the padding holds '\n': it must not be interpreted)
    rec = store[64:64 + n * R].view(n, R)
    s2, q2 = seq[64:64 + n * L].view(n, L), qual[64:64 + n * L].view(n, L)
    idx = torch.arange(n, dtype=torch.int64, device=dev)
    rec[:, 0] = ord("@")
    for j in range(W - 1):
        d = (idx >> (4 * (W - 2 - j))) & 15
        rec[:, 1 + j] = torch.where(d < 10, d + 48, d + 87).to(torch.uint8)
    del idx
    rec[:, W + 1:W + 1 + L] = s2
    rec[:, W + 2 + L] = ord("+")
    rec[:, W + 4 + L:W + 4 + 2 * L] = q2
    torch.cuda.synchronize()
    return store, n * R, s2, q2


def parse_buffers(dev, cap_bytes, cap_reads, with_def=True):
    """Output arrays of one faqcs_parse_device on `dev` -> (capi.ParseOut, dict of the tensors); the arenas proper start 64 bytes in."""
    import torch

    from faqcs_amd import _capi as capi

    t = {"seq": torch.empty(64 + cap_bytes + 64, dtype=torch.uint8, device=dev), "qual": torch.empty(64 + cap_bytes + 64, dtype=torch.uint8, device=dev),
         "offset": torch.empty(cap_reads + 1, dtype=torch.int32, device=dev), "terminal_n": torch.empty(cap_reads + 1, dtype=torch.uint8, device=dev),
         "def_pos": torch.empty(cap_reads + 1, dtype=torch.int32, device=dev), "def_len": torch.empty(cap_reads + 1, dtype=torch.int32, device=dev),
         "info": torch.zeros(4, dtype=torch.int64, device=dev)}
    out = capi.ParseOut(t["seq"].data_ptr() + 64, t["qual"].data_ptr() + 64, cap_bytes, cap_reads, t["offset"].data_ptr(), t["terminal_n"].data_ptr(),
                        t["def_pos"].data_ptr() if with_def else None, t["def_len"].data_ptr() if with_def else None, t["info"].data_ptr())
    return out, t


def read_info(info):
    """faqcs_parse_info from its 32 bytes on the device."""
    from faqcs_amd import _capi as capi

    p = capi.ParseInfo.from_buffer_copy(info.cpu().numpy().tobytes())
    return {f: int(getattr(p, f)) for f, _ in capi.ParseInfo._fields_}


def host_parse_ms(lib, text, R, n, threads):
    """faqcs_parse_host over `threads` ranges of whole records at once, one thread each (ctypes releases the GIL) -> wall ms."""
    from faqcs_amd import _capi as capi

    bounds = [n * i // threads for i in range(threads + 1)]
    jobs = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        m = b - a
        cap = m * R // 2
        seq, qual = np.empty(cap + 128, np.uint8), np.empty(cap + 128, np.uint8)
        off, tn, dp, dl = np.empty(m + 1, np.uint32), np.empty(m + 1, np.uint8), np.empty(m + 1, np.uint32), np.empty(m + 1, np.uint32)
        info = capi.ParseInfo()
        so, qo = (-seq.ctypes.data) % 16, (-qual.ctypes.data) % 16
        out = capi.ParseOut(seq.ctypes.data + so, qual.ctypes.data + qo, cap, m, off.ctypes.data, tn.ctypes.data, dp.ctypes.data, dl.ctypes.data, C.addressof(info))
        jobs.append((text.ctypes.data + a * R, m * R, out, info, (seq, qual, off, tn, dp, dl), m))
    rc = [None] * threads

    def run(i):
        rc[i] = lib.faqcs_parse_host(jobs[i][0], jobs[i][1], 1, C.byref(jobs[i][2]))

    ts = [threading.Thread(target=run, args=(i,)) for i in range(threads)]
    t0 = time.perf_counter()
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    ms = (time.perf_counter() - t0) * 1e3
    assert all(r == 0 for r in rc) and all(j[3].n_reads == j[5] and j[3].error == 0 and j[3].overflow == 0 for j in jobs)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--records", type=int, default=0, help="default: as many as fit below 2^32 bytes of text")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    torch.cuda.init()  # before libfaqcs_mi.so (torch ships its own HIP runtime)
    from faqcs_amd import _capi as capi
    from faqcs_amd.engine import HipEngine
    from faqcs_amd.options import parse_args
    from tools.source_hash import source_hash

    L = a.length
    R = record_bytes(L)
    n = a.records or ((1 << 32) - 1) // R
    assert n * R < (1 << 32)
    dev = torch.device("cuda:0")
    lib = capi.load_library()
    store, n_text, s2, q2 = synth_text(lib, dev, n, L)
    del s2, q2
    torch.cuda.empty_cache()
    eng = HipEngine(parse_args(["-u", "x", "-d", "y", "--ascii", "33"]), 256, 33, device=0)
    out, t = parse_buffers(dev, n * L, n)
    copy_dst = torch.empty(n_text, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    index, gather, copy = [], [], []
    for rep in range(a.reps + 1):  # the first round warms up (and grows the scratch)
        eng.parse_device(store.data_ptr() + 64, n_text, True, out)
        eng.sync()
        i, g = eng.parse_time_ms()
        index.append(i)
        gather.append(g)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        copy_dst.copy_(store[64:64 + n_text])
        e1.record()
        torch.cuda.synchronize()
        copy.append(e0.elapsed_time(e1))
    info = read_info(t["info"])
    assert info == {"n_bytes": n * L, "consumed": n_text, "n_reads": n, "max_read_len": L, "overflow": 0, "error": 0}, info
    im, gm, cm = float(np.median(index[1:])), float(np.median(gather[1:])), float(np.median(copy[1:]))
    ratios = [(x + y) / z for x, y, z in zip(index[1:], gather[1:], copy[1:])]
    del copy_dst
    host = store[64:64 + n_text].cpu().numpy()
    hm = min(host_parse_ms(lib, host, R, n, a.host_threads) for _ in range(2))
    ms = im + gm
    result = {"bench": "parse", "records": n, "length": L, "text_bytes": n_text, "reps": a.reps, "source_hash": source_hash(),
              "index_ms": round(im, 4), "gather_ms": round(gm, 4), "parse_ms": round(ms, 4), "copy_text_ms": round(cm, 4),
              "parse_over_copy": round(ms / cm, 3), "parse_over_copy_median_of_reps": round(float(np.median(ratios)), 3),
              "text_GB_per_s": round(n_text / ms / 1e6, 1), "copy_GB_per_s": round(2 * n_text / cm / 1e6, 1), "M_reads_per_s": round(n / ms / 1e3, 1),
              "host_threads": a.host_threads, "host_parse_ms": round(hm, 2), "host_text_GB_per_s": round(n_text / hm / 1e6, 2),
              "host_over_device": round(hm / ms, 1)}
    eng.close()
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
