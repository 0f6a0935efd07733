"""Diagnostic (not a test): faqcs_render_device on a device-resident batch of 2x150-shaped records whose FASTQ text lies just under 4 GiB,
against a device-to-device copy of exactly the rendered bytes in the same run.  Two option sets: the default (the copy-only gather) and
--replace_to_N_q 15 --out_ascii 64 (the editing gather); for each the trimmed rendering of every valid read and, once, the original
records (the discard form) of all reads.  Prints one JSON line; --out FILE also writes it there.

    python tools/render_bench.py [--records N] [--reps 7] [--out profiles/render/render_bench.json]

The text is built on the device from faqcs_synth_fill arenas with fixed-width deflines (tools/parse_bench.py synth_text).  Scan and gather are
timed apart (HIP events on the library's compute stream, median of --reps after a warm-up); GB/s counts the rendered text once."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OPTION_SETS = {"default": [], "replaceN15_out64": ["--replace_to_N_q", "15", "--out_ascii", "64"]}


def measure(eng, b, d_res, store, dpos, dlen, out, info, o_text, copy_dst, reps):
    import torch

    scan, gather, copy = [], [], []
    n_bytes = n_rec = 0
    for rep in range(reps + 1):  # the first round warms up (and grows the scratch)
        eng.render_device(b, d_res, store.data_ptr() + 64, dpos.data_ptr(), dlen.data_ptr(), out)
        eng.sync()
        s, g = eng.render_time_ms()
        scan.append(s)
        gather.append(g)
        h = info.cpu().numpy().view(np.uint64)
        n_bytes, n_rec = int(h[0]), int(h[1] & np.uint64(0xFFFFFFFF))
        assert int(h[1] >> np.uint64(32)) == 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        copy_dst[:n_bytes].copy_(o_text[64:64 + n_bytes])
        e1.record()
        torch.cuda.synchronize()
        copy.append(e0.elapsed_time(e1))
    sm, gm, cm = float(np.median(scan[1:])), float(np.median(gather[1:])), float(np.median(copy[1:]))
    ratios = [(x + y) / z for x, y, z in zip(scan[1:], gather[1:], copy[1:])]
    ms = sm + gm
    return {"records": n_rec, "text_bytes": n_bytes, "scan_ms": round(sm, 4), "gather_ms": round(gm, 4), "render_ms": round(ms, 4),
            "copy_ms": round(cm, 4), "render_over_copy": round(ms / cm, 3), "render_over_copy_median_of_reps": round(float(np.median(ratios)), 3),
            "text_GB_per_s": round(n_bytes / ms / 1e6, 1), "copy_GB_per_s": round(2 * n_bytes / cm / 1e6, 1), "M_records_per_s": round(n_rec / ms / 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--records", type=int, default=0, help="default: as many as fit below 2^32 bytes of text")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    torch.cuda.init()  # before libfaqcs_mi.so (torch ships its own HIP runtime)
    from faqcs_amd import _capi as capi
    from faqcs_amd.engine import HipEngine, _check
    from faqcs_amd.options import parse_args
    from tools.parse_bench import DEF_WIDTH, record_bytes, synth_text
    from tools.source_hash import source_hash

    L = a.length
    R = record_bytes(L)
    n = a.records or ((1 << 32) - 1) // R
    assert n * R < (1 << 32)
    dev = torch.device("cuda:0")
    lib = capi.load_library()
    store, n_text, s2, q2 = synth_text(lib, dev, n, L)
    off = torch.from_numpy((np.arange(n + 1, dtype=np.uint64) * L).astype(np.uint32).view(np.int32)).to(dev)
    dpos = torch.from_numpy((np.arange(n, dtype=np.uint64) * R).astype(np.uint32).view(np.int32)).to(dev)
    dlen = torch.full((n,), DEF_WIDTH, dtype=torch.int32, device=dev)
    tn = torch.zeros(n, dtype=torch.uint8, device=dev)
    _check(lib, lib.faqcs_terminal_n_flags(0, s2.data_ptr(), off.data_ptr(), n, tn.data_ptr()))
    res = torch.zeros((n, 4), dtype=torch.int16, device=dev)
    o_text = torch.empty(64 + n_text + 64, dtype=torch.uint8, device=dev)
    roff = torch.empty(n + 1, dtype=torch.int32, device=dev)
    info = torch.zeros(2, dtype=torch.int64, device=dev)
    out = capi.RenderOut(o_text.data_ptr() + 64, n_text, roff.data_ptr(), None, info.data_ptr())
    copy_dst = torch.empty(n_text, dtype=torch.uint8, device=dev)
    seg = np.array([0, n], dtype=np.uint32)
    b = capi.Batch(s2.data_ptr(), q2.data_ptr(), off.data_ptr(), n, 1, seg.ctypes.data, L, tn.data_ptr())
    result = {"bench": "render", "reads": n, "length": L, "input_text_bytes": n_text, "reps": a.reps, "source_hash": source_hash()}
    for name, args in OPTION_SETS.items():
        eng = HipEngine(parse_args(["-u", "x", "-d", "y", "--ascii", "33"] + args), 256, 33, device=0)
        _check(lib, lib.faqcs_submit_device(eng.ctx, C.byref(b), res.data_ptr()))
        eng.sync()
        result[name] = measure(eng, b, res.data_ptr(), store, dpos, dlen, out, info, o_text, copy_dst, a.reps)
        if name == "default":
            result["original_records"] = measure(eng, b, None, store, dpos, dlen, out, info, o_text, copy_dst, a.reps)
            assert result["original_records"]["text_bytes"] == n_text
        eng.close()
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
