"""Diagnostic (not a test): the pair stage on two device-resident mates of 2x150-shaped records with 16-byte deflines -- faqcs_pair_device
(ids, route, counters) against a device-to-device copy of the two texts, and the four faqcs_render_pair_device calls of a paired run against
copies of exactly the rendered bytes, with a single-source faqcs_render_device of one mate alongside -- all in the same run.  Prints one JSON
line; --out FILE also writes it there.

    python tools/pair_bench.py [--pairs N] [--reps 7] [--out profiles/pair/pair_bench.json]

The texts are built on the device from faqcs_synth_fill arenas with fixed-width deflines (tools/parse_bench.py synth_text, one seed per
mate); the results are those of two faqcs_submit_device (default options), so the four files have the sizes of a real run.  Every stage is
timed with HIP events on the library's compute stream, median of --reps after a warm-up."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--pairs", type=int, default=4_000_000)
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

    L, n = a.length, a.pairs
    R = record_bytes(L)
    n_text = n * R
    assert 2 * n_text < (1 << 32)
    dev = torch.device("cuda:0")
    lib = capi.load_library()
    eng = HipEngine(parse_args(["-1", "x", "-2", "y", "-d", "z", "--ascii", "33"]), 256, 33, device=0)
    off = torch.from_numpy((np.arange(n + 1, dtype=np.uint64) * L).astype(np.uint32).view(np.int32)).to(dev)
    dpos = torch.from_numpy((np.arange(n, dtype=np.uint64) * R).astype(np.uint32).view(np.int32)).to(dev)
    dlen = torch.full((n,), DEF_WIDTH, dtype=torch.int32, device=dev)
    seg = np.array([0, n], dtype=np.uint32)
    keep, mates, batches, stores, results = [], [], [], [], []
    for s in range(2):
        store, _, s2, q2 = synth_text(lib, dev, n, L, seed=20260101 + s)
        tn = torch.zeros(n, dtype=torch.uint8, device=dev)
        _check(lib, lib.faqcs_terminal_n_flags(0, s2.data_ptr(), off.data_ptr(), n, tn.data_ptr()))
        res = torch.zeros((n, 4), dtype=torch.int16, device=dev)
        b = capi.Batch(s2.data_ptr(), q2.data_ptr(), off.data_ptr(), n, 1, seg.ctypes.data, L, tn.data_ptr())
        _check(lib, lib.faqcs_submit_device(eng.ctx, C.byref(b), res.data_ptr()))
        eng.sync()
        mates.append(capi.Mate(C.pointer(b), res.data_ptr(), store.data_ptr() + 64, dpos.data_ptr(), dlen.data_ptr()))
        keep += [s2, q2, tn]
        batches.append(b)
        stores.append(store)
        results.append(res)
    route = torch.empty(n, dtype=torch.uint8, device=dev)
    d_info = torch.zeros(5, dtype=torch.int64, device=dev)
    dst = [torch.empty(n_text, dtype=torch.uint8, device=dev) for _ in range(2)]
    torch.cuda.synchronize()

    def timed_copy(pairs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for d, s in pairs:
            d.copy_(s)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    med = lambda v: float(np.median(v[1:]))  # noqa: E731  (the first round warms up and grows the scratch)
    check, finish, copy = [], [], []
    for rep in range(a.reps + 1):
        eng.pair_device(mates[0], mates[1], route.data_ptr(), d_info.data_ptr())
        eng.sync()
        c, f = eng.pair_time_ms()
        check.append(c)
        finish.append(f)
        copy.append(timed_copy([(dst[s], stores[s][64:64 + n_text]) for s in range(2)]))
    p = capi.PairInfo.from_buffer_copy(d_info.cpu().numpy().tobytes())
    assert (p.n_pairs, p.mismatch) == (n, 0)
    pm, cm = med(check) + med(finish), med(copy)
    result = {"bench": "pair", "pairs": n, "length": L, "text_bytes_per_mate": n_text, "reps": a.reps, "source_hash": source_hash(),
              "pair": {"check_ms": round(med(check), 4), "finish_ms": round(med(finish), 4), "pair_ms": round(pm, 4), "copy_two_texts_ms": round(cm, 4),
                       "pair_over_copy": round(pm / cm, 3), "M_pairs_per_s": round(n / pm / 1e3, 1), "paired_read_number": int(p.paired_read_number),
                       "n_one_valid": int(p.n_one_valid), "n_none_valid": int(p.n_none_valid)}}
    o_text = torch.empty(64 + 2 * n_text + 64, dtype=torch.uint8, device=dev)
    roff = torch.empty(2 * n + 1, dtype=torch.int32, device=dev)
    info = torch.zeros(2, dtype=torch.int64, device=dev)
    out = capi.RenderOut(o_text.data_ptr() + 64, 2 * n_text, roff.data_ptr(), None, info.data_ptr())
    copy_dst = torch.empty(2 * n_text, dtype=torch.uint8, device=dev)

    def rendering(call, times):
        scan, gather, copy = [], [], []
        n_bytes = n_rec = 0
        for rep in range(a.reps + 1):
            call()
            eng.sync()
            s, g = times()
            scan.append(s)
            gather.append(g)
            h = info.cpu().numpy().view(np.uint64)
            n_bytes, n_rec = int(h[0]), int(h[1] & np.uint64(0xFFFFFFFF))
            assert int(h[1] >> np.uint64(32)) == 0
            copy.append(timed_copy([(copy_dst[:n_bytes], o_text[64:64 + n_bytes])]) if n_bytes else 0.0)
        ms, cm = med(scan) + med(gather), med(copy)
        return {"records": n_rec, "text_bytes": n_bytes, "scan_ms": round(med(scan), 4), "gather_ms": round(med(gather), 4), "render_ms": round(ms, 4),
                "copy_ms": round(cm, 4), "render_over_copy": round(ms / cm, 3) if cm else None, "text_GB_per_s": round(n_bytes / ms / 1e6, 1)}

    for f, name in enumerate(capi.PAIR_FILES):
        result[name] = rendering(lambda: eng.render_pair_device(f, mates[0], mates[1], route.data_ptr(), n, out), eng.render_pair_time_ms)
    result["single_source_mate1"] = rendering(lambda: eng.render_device(batches[0], results[0].data_ptr(), stores[0].data_ptr() + 64, dpos.data_ptr(), dlen.data_ptr(), out),
                                              eng.render_time_ms)
    eng.close()
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
