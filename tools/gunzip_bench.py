"""Diagnostic (not a test): faqcs_gunzip_device on ordinary gzip of 2x150-shaped FASTQ text at zlib levels 1 and 6, at piece_bytes of 64, 128
and 256 KiB, against, in the same process: (a) ONE zlib thread (zlib.decompressobj(31)) over the same file; (b) faqcs_inflate_device on the
same text as BGZF members of 65 280 bytes -- what the second pass and the probe cost --; (c) a torch device-to-device copy of the text.
Prints one JSON line; --out FILE also writes it there.

    python tools/gunzip_bench.py [--mib 256] [--distinct-mib 64] [--reps 7] [--chunks 4,16] [--out profiles/inflate/gunzip_bench.json]

--chunks N[,N..] also feeds the same input as N equal chunks through device.GunzipStream (faqcs_gunzip_stream_device) at the first piece
size and reports the total wall time, its ratio to the single call of the same run, and the rounds of every call.

The text is inflate_bench.shaped_text; --distinct-mib of it are one gzip member, and the file holds that member --mib / --distinct-mib
times (`cat` of equal files).  The three stage times are the library's (HIP events around every pass: faqcs_gunzip_time_ms), `call_ms` is
the wall time of the blocking call -- stages, the walk on the host and the copies between them --; medians of --reps after a warm-up; GB/s
counts the text.  resolve_share is the resolve stage -- the serial part, one step per piece -- over the wall time."""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.inflate_bench import BLOCK, bgzf_members, inflate_buffers, shaped_text, upload  # noqa: E402


def gzip_member(text, level):
    co = zlib.compressobj(level, zlib.DEFLATED, 31)
    return co.compress(text) + co.flush()


def zlib_thread_ms(member):
    t0 = time.perf_counter()
    d = zlib.decompressobj(31)
    n = len(d.decompress(member))
    assert d.eof
    return (time.perf_counter() - t0) * 1e3, n


def streamed(eng, d_comp, n_chunks, piece_bytes, reps, n_text, n_members, single_ms):
    """The same input as n_chunks equal chunks through device.GunzipStream (faqcs_gunzip_stream_device): every call gets the bytes from
    the previous call's consumed to the next chunk end.  -> the total wall time (median of reps after a warm-up), its ratio to the single
    call of the same build, and the rounds of every call of the last repetition"""
    from faqcs_amd.device import GunzipStream

    n_comp = int(d_comp.numel())
    ends = [n_comp * (k + 1) // n_chunks for k in range(n_chunks)]
    cap = int(1.5 * n_text / n_chunks) + (8 << 20)
    wall, rounds = [], []
    for rep in range(reps + 1):
        gzs = GunzipStream(eng, piece_bytes=piece_bytes)
        at, rounds, total = 0, [], 0.0
        for k, end in enumerate(ends):
            t0 = time.perf_counter()
            text, info = gzs.feed(d_comp[at:end], k == n_chunks - 1, capacity=cap)
            total += (time.perf_counter() - t0) * 1e3
            assert info.error == 0, info.error
            at += int(info.consumed)
            rounds.append(int(info.n_rounds))
            del text
        assert (gzs.state.total_bytes, gzs.state.members, gzs.state.total_comp, gzs.state.phase) == (n_text, n_members, n_comp, 0), "the streamed run differs"
        wall.append(total)
    wm = float(np.median(wall[1:]))
    return {"call_ms_total": round(wm, 3), "over_single_call": round(wm / single_ms, 3), "n_rounds_per_call": rounds, "text_GB_per_s": round(n_text / wm / 1e6, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--distinct-mib", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--levels", default="1,6")
    ap.add_argument("--pieces-kib", default="64,128,256")
    ap.add_argument("--chunks", default="", help="N[,N..]: also feed the input as N equal chunks through GunzipStream, at the first piece size")
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
    result = {"bench": "gunzip", "text_MiB": a.mib, "distinct_MiB": a.distinct_mib, "reps": a.reps, "source_hash": source_hash(), "levels": {}}
    text = shaped_text(a.distinct_mib << 20)
    copies = -(-(a.mib << 20) // len(text))
    n_text = len(text) * copies
    for level in [int(x) for x in a.levels.split(",")]:
        member = gzip_member(text.tobytes(), level)
        comp = np.tile(np.frombuffer(member, np.uint8), copies)
        store = torch.empty(len(comp) + 16, dtype=torch.uint8, device=dev)
        store[1:1 + len(comp)] = torch.from_numpy(comp).to(dev)  # one byte off dword alignment
        o_text = torch.empty(64 + n_text + 64, dtype=torch.uint8, device=dev)
        info = torch.zeros(5, dtype=torch.int64, device=dev)
        out = capi.GunzipOut(o_text.data_ptr() + 64, n_text, info.data_ptr())
        copy_dst = torch.empty(n_text, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        row = {"members": copies, "compressed_bytes": len(comp), "text_bytes": n_text, "ratio": round(n_text / len(comp), 3), "pieces": {}}
        for kib in [int(x) for x in a.pieces_kib.split(",")]:
            stage, wall = [], []
            for rep in range(a.reps + 1):  # the first round warms up (and grows the scratch)
                t0 = time.perf_counter()
                eng.gunzip_device(store.data_ptr() + 1, len(comp), out, kib << 10, 0)
                wall.append((time.perf_counter() - t0) * 1e3)
                stage.append(eng.gunzip_time_ms())
            p = capi.GunzipInfo.from_buffer_copy(info.cpu().numpy().tobytes())
            assert (p.n_bytes, p.n_members, p.overflow, p.error) == (n_text, copies, 0, 0), (p.n_bytes, p.n_members, p.overflow, p.error)
            assert (o_text[64:64 + len(text)].cpu().numpy() == text).all(), "the text differs from the input"
            cm, dm, rm = (float(np.median([s[k] for s in stage[1:]])) for k in range(3))
            wm = float(np.median(wall[1:]))
            row["pieces"][str(kib)] = {"n_pieces": int(p.n_pieces), "n_fixups": int(p.n_fixups), "n_rounds": int(p.n_rounds), "count_ms": round(cm, 3),
                                       "decode_ms": round(dm, 3), "resolve_ms": round(rm, 3), "call_ms": round(wm, 3), "resolve_share": round(rm / wm, 3),
                                       "text_GB_per_s": round(n_text / wm / 1e6, 2)}
        for n_chunks in [int(x) for x in a.chunks.split(",") if x]:
            row.setdefault("chunks", {})[str(n_chunks)] = streamed(eng, store[1:1 + len(comp)], n_chunks, int(a.pieces_kib.split(",")[0]) << 10, a.reps, n_text, copies,
                                                                  row["pieces"][a.pieces_kib.split(",")[0]]["call_ms"])
        copy = []
        for rep in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            copy_dst.copy_(o_text[64:64 + n_text])
            e1.record()
            torch.cuda.synchronize()
            copy.append(e0.elapsed_time(e1))
        row["copy_text_ms"] = round(float(np.median(copy[1:])), 4)
        zms = min(zlib_thread_ms(member)[0] for _ in range(2)) * copies
        row["zlib_one_thread_ms"] = round(zms, 1)
        row["zlib_text_GB_per_s"] = round(n_text / zms / 1e6, 3)
        del store, copy_dst, o_text
        torch.cuda.empty_cache()
        # (b) the same text as BGZF members through faqcs_inflate_device
        distinct = bgzf_members(text, level)
        n_members = len(distinct) * copies
        bstore, d_comp, n_comp, d_moff = upload(dev, distinct, copies)
        bout, t = inflate_buffers(dev, n_text, n_members)
        torch.cuda.synchronize()
        bg = []
        for rep in range(a.reps + 1):
            eng.inflate_device(d_comp, n_comp, d_moff.data_ptr(), n_members, bout)
            eng.sync()
            bg.append(sum(eng.inflate_time_ms()))
        row["bgzf_inflate_ms"] = round(float(np.median(bg[1:])), 3)
        row["bgzf_member_text_bytes"] = BLOCK
        best = min(row["pieces"].values(), key=lambda r: r["call_ms"])
        row["gunzip_over_bgzf"] = round(best["call_ms"] / row["bgzf_inflate_ms"], 2)
        row["zlib_over_gunzip"] = round(zms / best["call_ms"], 1)
        result["levels"][str(level)] = row
        del bstore, t, bout
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
