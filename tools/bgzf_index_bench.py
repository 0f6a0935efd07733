"""Diagnostic (not a test): faqcs_bgzf_index_device against what it replaces for a caller whose compressed bytes are in HBM already --
the device-to-host copy of the bytes, faqcs_bgzf_index_host over them, the upload of the offsets -- in the same process.  Two inputs:
members of 65 280 bytes of 2x150-shaped text at zlib level 6 (tools/inflate_bench.py builds them), and as many bytes of 28-byte empty
members, the densest chain there is.  Prints one JSON line; --out FILE also writes it there.

    python tools/bgzf_index_bench.py [--kib 64,1024,65536] [--reps 9] [--out profiles/inflate/bgzf_index_bench.json]

--kib: the sizes of the compressed input, each measured on both inputs (65 536 KiB = 64 MiB is the size the issue of this tool names;
the smaller ones show where the launches of the device form weigh more than the copy it saves).

The device call is timed with HIP events on the library's compute stream (faqcs_bgzf_index_time_ms: candidates, chain) and, because the
events do not see what the host spends enqueueing some thirty launches, also with the wall clock around the call and faqcs_sync(); the
host path with the wall clock around its three steps, each step also on its own, the copies into and out of pinned memory.  Medians of --reps after a
warm-up round (which also grows the scratch)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def inputs(kib, members):
    """-> {name: compressed bytes as a uint8 array}: whole members of `members` (16 MiB of text, distinct; the file repeats them) up to at
    least `kib` KiB, and as many bytes of empty members"""
    n, sizes = kib << 10, np.array([len(m) for m in members])
    k = int(np.searchsorted(np.cumsum(sizes), n)) + 1
    one = np.frombuffer(b"".join(members[:k]), np.uint8)
    return {"members_of_65280_text_bytes_level_6": np.tile(one, -(-n // len(one))) if k >= len(members) else one,
            "empty_members_of_28_bytes": np.tile(np.frombuffer(EOF_MEMBER, np.uint8), -(-n // 28))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kib", default="64,1024,65536")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    torch.cuda.init()  # before libfaqcs_mi.so (torch ships its own HIP runtime)
    from faqcs_amd import _capi as capi
    from faqcs_amd.engine import HipEngine
    from faqcs_amd.options import parse_args
    from tools.source_hash import source_hash

    dev = torch.device("cuda:0")
    eng = HipEngine(parse_args(["-u", "x", "-d", "y", "--ascii", "33"]), 256, 33, device=0)
    from tools.inflate_bench import bgzf_members, shaped_text

    members = bgzf_members(shaped_text(16 << 20), 6)
    result = {"bench": "bgzf_index", "reps": a.reps, "source_hash": source_hash(), "compressed_KiB": {}}
    for kib, name, comp in [(kib, name, comp) for kib in [int(x) for x in a.kib.split(",")] for name, comp in inputs(kib, members).items()]:
        n = len(comp)
        cap = n // 26 + 1
        store = torch.empty(n + 16, dtype=torch.uint8, device=dev)
        store[1:1 + n] = torch.from_numpy(comp.copy()).to(dev)  # one byte off dword alignment
        d_comp = store[1:1 + n]
        d_moff = torch.empty(cap + 1, dtype=torch.int32, device=dev)
        d_info = torch.zeros(3, dtype=torch.int64, device=dev)
        h_comp = torch.empty(n, dtype=torch.uint8).pin_memory()
        h_moff = torch.empty(cap + 1, dtype=torch.int32).pin_memory()
        d_moff2 = torch.empty(cap + 1, dtype=torch.int32, device=dev)
        hinfo = capi.BgzfIndexInfo()
        torch.cuda.synchronize()
        cand, chain, wall, d2h, walk, h2d, whole = [], [], [], [], [], [], []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            eng.bgzf_index_device(d_comp.data_ptr(), n, True, d_moff.data_ptr(), cap, d_info.data_ptr())
            eng.sync()
            wall.append((time.perf_counter() - t0) * 1e3)
            c, j = eng.bgzf_index_time_ms()
            cand.append(c)
            chain.append(j)
            t0 = time.perf_counter()
            h_comp.copy_(d_comp)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            rc = eng.lib.faqcs_bgzf_index_host(h_comp.data_ptr(), n, 1, h_moff.data_ptr(), cap, C.byref(hinfo))
            t2 = time.perf_counter()
            d_moff2[:hinfo.n_members + 1].copy_(h_moff[:hinfo.n_members + 1])
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            assert rc == 0
            d2h.append((t1 - t0) * 1e3)
            walk.append((t2 - t1) * 1e3)
            h2d.append((t3 - t2) * 1e3)
            whole.append((t3 - t0) * 1e3)
        p = capi.BgzfIndexInfo.from_buffer_copy(d_info.cpu().numpy().tobytes())
        k = int(p.n_members)
        assert (p.consumed, k, p.overflow, p.error) == (hinfo.consumed, hinfo.n_members, 0, hinfo.error), "the device index differs from the host statement"
        assert torch.equal(d_moff[:k + 1], d_moff2[:k + 1]), "the device offsets differ from the host statement's"
        med = lambda v: float(np.median(v[1:]))
        dev_ms, host_ms = med(cand) + med(chain), med(whole)
        result["compressed_KiB"].setdefault(str(kib), {})[name] = {
            "compressed_bytes": n, "members": k, "consumed": int(p.consumed), "error": int(p.error),
            "device_candidates_ms": round(med(cand), 4), "device_chain_ms": round(med(chain), 4), "device_ms": round(dev_ms, 4),
            "device_GB_per_s": round(n / dev_ms / 1e6, 1), "device_call_and_sync_wall_ms": round(med(wall), 4),
            "host_path_ms": round(host_ms, 4), "copy_to_host_ms": round(med(d2h), 4), "host_walk_ms": round(med(walk), 4), "offsets_upload_ms": round(med(h2d), 4),
            "host_path_over_device": round(host_ms / dev_ms, 2), "host_path_over_device_wall": round(host_ms / med(wall), 2)}
        del store, d_comp, d_moff, d_moff2, h_comp, h_moff
        torch.cuda.empty_cache()
    eng.close()
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
