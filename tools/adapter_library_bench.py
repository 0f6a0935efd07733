"""Cost of the adapter pre-pass per library size: faqcs_kernel_report().adapter_ms of one submission of
device-resident synthetic 2x150 reads (faqcs_synth_fill) for

  builtin        the built-in adapter set (--adapter)
  rand64 ...     64, 128, 640 and 2 560 random 20 ... 60-mers (one, two, ten and forty groups of the pre-pass)
  builtin+32767  the built-in set plus one random 32 767-base target

and prints one JSON line per set: adapter ms per submission and M reads/s of the pre-pass alone.

    python tools/adapter_library_bench.py [--reads 4194304] [--steps 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1 << 22)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--sets", default="builtin,rand64,rand128,rand640,rand2560,builtin+32767")
    a = ap.parse_args()

    import torch

    from faqcs_amd import _capi as capi
    from faqcs_amd.engine import HipEngine, _check
    from faqcs_amd.options import BUILTIN_ADAPTERS, parse_args

    lib = capi.load_library()
    dev = torch.device("cuda", 0)
    n, L = a.reads, 150
    seq_buf = torch.empty(n * L + 16 + 64, dtype=torch.uint8, device=dev)  # (FAQCS_ARENA_PAD_BEFORE / _AFTER)
    qual_buf = torch.empty(n * L + 16 + 64, dtype=torch.uint8, device=dev)
    off = torch.empty(n + 1, dtype=torch.int32, device=dev)
    res = torch.empty((n, 4), dtype=torch.int16, device=dev)
    seq, qual = seq_buf.data_ptr() + 16, qual_buf.data_ptr() + 16
    _check(lib, lib.faqcs_synth_fill(0, seq, qual, off.data_ptr(), n, L, 20260101, 0, 0.0))
    torch.cuda.synchronize()
    segs = np.append(np.arange(0, n, capi.SEGMENT_READS), n).astype(np.uint32)

    rng = np.random.Generator(np.random.PCG64(4242))
    acgt = np.frombuffer(b"ACGT", np.uint8)
    rand = lambda k: acgt[rng.integers(0, 4, k)].tobytes().decode()  # noqa: E731

    for name in a.sets.split(","):
        if name == "builtin":
            targets = list(BUILTIN_ADAPTERS)
        elif name.startswith("rand"):
            targets = [("r%d" % j, rand(int(rng.integers(20, 61)))) for j in range(int(name[4:]))]
        elif name == "builtin+32767":
            targets = list(BUILTIN_ADAPTERS) + [("long", rand(32767))]
        else:
            raise SystemExit("unknown set " + name)
        opt = parse_args(["-u", "x", "-d", "y", "--adapter"])
        opt.adapter = targets
        eng = HipEngine(opt, L, 33)
        bt = capi.Batch(seq, qual, off.data_ptr(), n, len(segs) - 1, segs.ctypes.data, L, None)
        _check(lib, lib.faqcs_submit_device(eng.ctx, C.byref(bt), res.data_ptr()))  # warm-up
        _check(lib, lib.faqcs_sync(eng.ctx))
        kt = capi.KernelTimes()
        lib.faqcs_kernel_report(eng.ctx, C.byref(kt))  # (reads and resets the timers)
        for _ in range(a.steps):
            _check(lib, lib.faqcs_submit_device(eng.ctx, C.byref(bt), res.data_ptr()))
        _check(lib, lib.faqcs_sync(eng.ctx))
        _check(lib, lib.faqcs_kernel_report(eng.ctx, C.byref(kt)))
        ms = float(kt.adapter_ms)
        print(json.dumps({"set": name, "targets": len(targets), "reads": n, "adapter_ms": round(ms, 3), "M_reads_per_s": round(n / ms / 1e3, 1) if ms > 0 else None}), flush=True)
        del eng


if __name__ == "__main__":
    main()
