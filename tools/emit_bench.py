"""Diagnostic (not a test): faqcs_emit_device on device-resident synthetic 2x150 reads (faqcs_synth_fill) against a
device-to-device copy of the two input arenas in the same run.  Prints one JSON line; --out FILE also writes it there.

    python tools/emit_bench.py [--reads 28600000] [--reps 7] [--out profiles/emit/emit_bench.json]

Per configuration (default options; --replace_to_N_q 15 --out_ascii 64): scan and gather time apart (HIP events on the library's compute
stream, median of --reps after a warm-up), the copy, their ratio, GB/s counted as (input arena bytes + 2 x emitted bytes + 24 B/read) /
time, and M reads/s."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=28_600_000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    torch.cuda.init()  # before libfaqcs_mi.so (torch ships its own HIP runtime)
    from faqcs_amd import _capi as capi
    from faqcs_amd.engine import HipEngine, _check
    from faqcs_amd.options import parse_args
    from tools.source_hash import source_hash

    n, L = a.reads, a.length
    assert n * L < (1 << 32) - 4096, "one arena holds less than 4 GiB"
    dev = torch.device("cuda:0")
    lib = capi.load_library()
    cap = n * L
    seq = torch.empty(64 + cap + 128, dtype=torch.uint8, device=dev)
    qual = torch.empty_like(seq)
    off = torch.from_numpy((np.arange(n + 1, dtype=np.uint64) * L).astype(np.uint32).view(np.int32)).to(dev)
    piece, done = (1 << 31) // L, 0
    while done < n:  # (filled in pieces of whole reads: the generator's offsets are 32 bits wide)
        m = min(piece, n - done)
        scratch = torch.empty(m + 1, dtype=torch.int32, device=dev)
        _check(lib, lib.faqcs_synth_fill(0, seq.data_ptr() + 64 + done * L, qual.data_ptr() + 64 + done * L, scratch.data_ptr(), m, L, 20260101, done, 0.0))
        done += m
    res = torch.zeros((n, 4), dtype=torch.int16, device=dev)
    o_seq = torch.empty(64 + cap + 64, dtype=torch.uint8, device=dev)
    o_qual = torch.empty_like(o_seq)
    o_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
    o_idx = torch.empty(n, dtype=torch.int32, device=dev)
    info = torch.zeros(2, dtype=torch.int64, device=dev)
    tn = torch.empty(n + 64, dtype=torch.uint8, device=dev)
    _check(lib, lib.faqcs_terminal_n_flags(0, seq.data_ptr() + 64, off.data_ptr(), n, tn.data_ptr()))
    torch.cuda.synchronize()
    seg = np.array([0, n], dtype=np.uint32)
    out = capi.EmitOut(o_seq.data_ptr() + 64, o_qual.data_ptr() + 64, cap, o_off.data_ptr(), o_idx.data_ptr(), info.data_ptr())
    result = {"bench": "emit", "reads": n, "length": L, "reps": a.reps, "source_hash": source_hash(), "configs": {}}
    copy_ms = []
    for name, extra in (("default", []), ("replaceN15_out64", ["--replace_to_N_q", "15", "--out_ascii", "64"])):
        eng = HipEngine(parse_args(["-u", "x", "-d", "y", "--ascii", "33"] + extra), 256, 33, device=0)
        b = capi.Batch(seq.data_ptr() + 64, qual.data_ptr() + 64, off.data_ptr(), n, 1, seg.ctypes.data, L, tn.data_ptr())
        _check(lib, lib.faqcs_submit_device(eng.ctx, C.byref(b), res.data_ptr()))
        eng.sync()
        scan, gather = [], []
        for rep in range(a.reps + 1):  # the first round warms up
            eng.emit_device(b, res.data_ptr(), out)
            eng.sync()
            s, g = eng.emit_time_ms()
            scan.append(s)
            gather.append(g)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            o_seq[64:64 + cap].copy_(seq[64:64 + cap])
            o_qual[64:64 + cap].copy_(qual[64:64 + cap])
            e1.record()
            torch.cuda.synchronize()
            copy_ms.append(e0.elapsed_time(e1))
        # (the copy overwrote the emission: emit once more so that info / outputs are the emission's)
        eng.emit_device(b, res.data_ptr(), out)
        eng.sync()
        h = info.cpu().numpy().view(np.uint64)
        n_bytes, n_emit = int(h[0]), int(h[1] & np.uint64(0xFFFFFFFF))
        sm, gm = float(np.median(scan[1:])), float(np.median(gather[1:]))
        cm = float(np.median(copy_ms[-a.reps:]))
        ms = sm + gm
        moved = 2 * cap + 2 * n_bytes + 24 * n
        result["configs"][name] = {"scan_ms": round(sm, 4), "gather_ms": round(gm, 4), "emit_ms": round(ms, 4), "copy_both_arenas_ms": round(cm, 4),
                                   "emit_over_copy": round(ms / cm, 3), "emitted_reads": n_emit, "emitted_bytes": n_bytes,
                                   "GB_per_s": round(moved / ms / 1e6, 1), "copy_GB_per_s": round(4 * cap / cm / 1e6, 1),
                                   "M_reads_per_s": round(n / ms / 1e3, 1)}
        eng.close()
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
