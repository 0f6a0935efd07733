"""A diagnostic, not a test: faqcs_deflate_device on 256 MiB of text (64 MiB distinct) of two kinds -- tools/inflate_bench.shaped_text and the
Illumina-shaped text of tests/deflate_cases.py -- as medians of 7 HIP-event timings after a warm-up, beside a torch device-to-device copy of
the text, one zlib thread at levels 1 and 6 in the same process, and the compressed size next to zlib's at level 1, level 6 and Huffman-only.
Writes profiles/deflate/deflate_bench.json; with --mode dense (faqcs_deflate_device_mode, FAQCS_DEFLATE_DENSE) profiles/deflate/deflate_bench_dense.json.

    python tools/deflate_bench.py [--mode fast|dense] [--mib 256] [--distinct-mib 64] [--out profiles/deflate/deflate_bench.json]
"""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from faqcs_amd import _capi as capi  # noqa: E402

MAX_TEXT = 65280


def deflate_buffers(dev, n_text, member_bytes=0, final=True):
    """(capi.DeflateOut, tensors) for a text of n_text bytes: room for the stored form of every member."""
    import torch

    mb = member_bytes or MAX_TEXT
    n = -(-n_text // mb) + (1 if final else 0)
    cap = n_text + 31 * n + 16
    t = {"comp": torch.empty(cap + 64, dtype=torch.uint8, device=dev), "member_offset": torch.zeros(n + 1, dtype=torch.int32, device=dev),
         "info": torch.zeros(3, dtype=torch.int64, device=dev)}
    assert t["comp"].data_ptr() % 16 == 0
    return capi.DeflateOut(t["comp"].data_ptr(), cap, t["member_offset"].data_ptr(), t["info"].data_ptr()), t


def read_info(info):
    p = capi.DeflateInfo.from_buffer_copy(info.cpu().numpy().tobytes())
    return {f: int(getattr(p, f)) for f, _ in capi.DeflateInfo._fields_}


def zlib_thread_ms(text, level, strategy=zlib.Z_DEFAULT_STRATEGY, sizes=None):
    """ms one thread needs to deflate `text` (uint8 array) as raw streams of 65 280 bytes of text each; sizes: a list that takes the total."""
    view = memoryview(text)
    total = 0
    t0 = time.perf_counter()
    for a in range(0, len(view), MAX_TEXT):
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        total += len(co.compress(view[a:a + MAX_TEXT])) + len(co.flush())
    ms = (time.perf_counter() - t0) * 1e3
    if sizes is not None:
        sizes.append(total)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--distinct-mib", type=int, default=64)
    ap.add_argument("--mode", choices=("fast", "dense"), default="fast")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "deflate", "deflate_bench.json" if a.mode == "fast" else "deflate_bench_dense.json")
    mode = capi.DEFLATE_DENSE if a.mode == "dense" else capi.DEFLATE_FAST
    import torch

    import deflate_cases as dc
    from faqcs_amd.engine import HipEngine
    from faqcs_amd.options import parse_args
    from tools.inflate_bench import shaped_text

    dev = torch.device("cuda:0")
    eng = HipEngine(parse_args(["-u", "x", "-d", "y", "--ascii", "33"]), 256, 33, device=0)
    result = {"device": torch.cuda.get_device_name(0), "mib": a.mib, "distinct_mib": a.distinct_mib, "mode": a.mode, "texts": {}}
    reps = max(1, a.mib // a.distinct_mib)
    for name in ("shaped", "illumina"):
        distinct = shaped_text(a.distinct_mib << 20) if name == "shaped" else np.frombuffer(dc.illumina_text(a.distinct_mib << 20), np.uint8)
        distinct = np.ascontiguousarray(distinct[:a.distinct_mib << 20])
        d_text = torch.from_numpy(distinct.copy()).to(dev).repeat(reps)
        n_text = int(d_text.numel())
        out, t = deflate_buffers(dev, n_text)
        torch.cuda.synchronize()
        enc, gat = [], []
        for rep in range(8):
            eng.deflate_device(d_text.data_ptr(), n_text, 0, 1, out, mode=mode)
            eng.sync()
            e, g = eng.deflate_time_ms()
            enc.append(e), gat.append(g)
        info = read_info(t["info"])
        copy = []
        dst = torch.empty_like(d_text)
        for rep in range(8):
            a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a0.record(); dst.copy_(d_text); a1.record(); torch.cuda.synchronize()
            copy.append(a0.elapsed_time(a1))
        sizes = {}
        row = {"n_text": n_text, "n_bytes": info["n_bytes"], "n_members": info["n_members"], "n_stored": info["n_stored"],
               "encode_ms": float(np.median(enc[1:])), "gather_ms": float(np.median(gat[1:])), "d2d_copy_ms": float(np.median(copy[1:]))}
        row["device_ms"] = row["encode_ms"] + row["gather_ms"]
        row["device_GBps_of_text"] = n_text / row["device_ms"] / 1e6
        for key, level, strat in (("zlib1", 1, zlib.Z_DEFAULT_STRATEGY), ("zlib6", 6, zlib.Z_DEFAULT_STRATEGY), ("zlib_huffman_only", 1, zlib.Z_HUFFMAN_ONLY)):
            s = []
            ms = zlib_thread_ms(distinct, level, strat, s)
            row[key + "_thread_ms"] = ms * reps
            sizes[key] = s[0] * reps
        ours = info["n_bytes"] - 26 * (info["n_members"] - 1) - 28
        row["stream_bytes"] = ours
        row["zlib_stream_bytes"] = sizes
        row["ratio_to_zlib1"], row["ratio_to_zlib6"] = ours / sizes["zlib1"], ours / sizes["zlib6"]
        row["zlib1_thread_over_device"] = row["zlib1_thread_ms"] / row["device_ms"]
        result["texts"][name] = row
        print(name, json.dumps(row))
        del d_text, dst, t
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    eng.close()


if __name__ == "__main__":
    main()
