"""Diagnostic (not a test): faqcs_inflate_device on BGZF members of 2x150-shaped FASTQ text at zlib levels 1, 6 and 9, against a torch
device-to-device copy of the produced text in the same run and against ONE zlib thread (zlib.decompressobj(-15) per member) over the
same members in the same process.  Prints one JSON line; --out FILE also writes it there.

    python tools/inflate_bench.py [--mib 256] [--distinct-mib 64] [--reps 7] [--out profiles/inflate/inflate_bench.json]

The text is made on the host (shaped_text below: fixed-width deflines, uniform bases, qualities from a skewed distribution), cut into
members of 65 280 bytes as bgzip does, compressed by Python's zlib; --distinct-mib of it are distinct, the file repeats them up to --mib.
Scan and decode are timed apart (HIP events on the library's compute stream, median of --reps after a warm-up); GB/s counts the text."""
import argparse
import json
import os
import struct
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BLOCK = 65280  # text bytes of a member, as bgzip cuts them


def shaped_text(n_bytes, L=150, seed=20260101):
    """At least n_bytes of FASTQ text of L-base records: '@' + 15 hex digits, uniform ACGT, qualities 2 .. 41 skewed towards the top."""
    W = 16
    R = W + 1 + L + 1 + 2 + L + 1
    n = -(-n_bytes // R)
    rng = np.random.Generator(np.random.PCG64(seed))
    rec = np.full((n, R), 10, np.uint8)
    rec[:, 0] = ord("@")
    idx = np.arange(n, dtype=np.int64)
    for j in range(W - 1):
        d = (idx >> (4 * (W - 2 - j))) & 15
        rec[:, 1 + j] = np.where(d < 10, d + 48, d + 87)
    rec[:, W + 1:W + 1 + L] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, L))]
    rec[:, W + 2 + L] = ord("+")
    q = 41 - np.minimum(rng.geometric(0.35, (n, L)) - 1, 39)
    rec[:, W + 4 + L:W + 4 + 2 * L] = (q + 33).astype(np.uint8)
    return rec.reshape(-1)


def bgzf_member(text, level):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    data = co.compress(text) + co.flush()
    total = 18 + len(data) + 8
    assert total <= 65536
    return struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, total - 1) + data + struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF, len(text))


def bgzf_members(text, level, block=BLOCK):
    """The members of `text` (bytes-like) cut every `block` bytes."""
    mv = memoryview(text)
    return [bgzf_member(bytes(mv[a:a + block]), level) for a in range(0, len(mv), block)]


def zlib_thread_ms(members):
    """One zlib thread over the members: raw inflate of each deflate stream and its CRC, as a reader has to -> (ms, text bytes)."""
    t0 = time.perf_counter()
    n = 0
    for m in members:
        d = zlib.decompressobj(-15)
        t = d.decompress(m[18:-8])
        assert zlib.crc32(t) & 0xFFFFFFFF == struct.unpack_from("<I", m, len(m) - 8)[0]
        n += len(t)
    return (time.perf_counter() - t0) * 1e3, n


def inflate_buffers(dev, cap_bytes, n_members):
    """Output arrays of one faqcs_inflate_device on `dev` -> (capi.InflateOut, dict of the tensors); the text proper starts 64 bytes in."""
    import torch

    from faqcs_amd import _capi as capi

    t = {"text": torch.empty(64 + cap_bytes + 64, dtype=torch.uint8, device=dev), "member_text_offset": torch.empty(n_members + 1, dtype=torch.int32, device=dev),
         "info": torch.zeros(3, dtype=torch.int64, device=dev)}
    assert (t["text"].data_ptr() + 64) % 16 == 0
    return capi.InflateOut(t["text"].data_ptr() + 64, cap_bytes, t["member_text_offset"].data_ptr(), t["info"].data_ptr()), t


def read_info(info):
    """faqcs_inflate_info from its 24 bytes on the device."""
    from faqcs_amd import _capi as capi

    p = capi.InflateInfo.from_buffer_copy(info.cpu().numpy().tobytes())
    return {f: int(getattr(p, f)) for f, _ in capi.InflateInfo._fields_ if f != "reserved"}


def build_file(level, mib, distinct_mib, seed=20260101):
    """-> (members of the distinct part, how often the file repeats them, text bytes of the distinct part)"""
    text = shaped_text(distinct_mib << 20, seed=seed)
    distinct = bgzf_members(text, level)
    reps = -(-(mib << 20) // len(text))
    return distinct, reps, len(text), text


def upload(dev, distinct, reps):
    """The file in device memory, one byte off dword alignment, and its member offsets -> (storage, device address, n_comp, offsets tensor)"""
    import torch

    one = np.frombuffer(b"".join(distinct), np.uint8)
    comp = np.tile(one, reps)
    moff = np.concatenate([[0], np.cumsum(np.tile([len(m) for m in distinct], reps))])
    assert moff[-1] == len(comp) < (1 << 32)
    store = torch.empty(len(comp) + 16, dtype=torch.uint8, device=dev)
    store[1:1 + len(comp)] = torch.from_numpy(comp).to(dev)
    d_moff = torch.from_numpy(moff.astype(np.uint32).view(np.int32)).to(dev)
    return store, store.data_ptr() + 1, len(comp), d_moff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--distinct-mib", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--levels", default="1,6,9")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    torch.cuda.init()  # before libfaqcs_mi.so (torch ships its own HIP runtime)
    from faqcs_amd.engine import HipEngine
    from faqcs_amd.options import parse_args
    from tools.source_hash import source_hash

    dev = torch.device("cuda:0")
    eng = HipEngine(parse_args(["-u", "x", "-d", "y", "--ascii", "33"]), 256, 33, device=0)
    result = {"bench": "inflate", "text_MiB": a.mib, "distinct_MiB": a.distinct_mib, "reps": a.reps, "member_text_bytes": BLOCK, "source_hash": source_hash(), "levels": {}}
    for level in [int(x) for x in a.levels.split(",")]:
        distinct, reps, n_distinct, text = build_file(level, a.mib, a.distinct_mib)
        n_text, n_members = n_distinct * reps, len(distinct) * reps
        store, d_comp, n_comp, d_moff = upload(dev, distinct, reps)
        out, t = inflate_buffers(dev, n_text, n_members)
        copy_dst = torch.empty(n_text, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        scan, decode, copy = [], [], []
        for rep in range(a.reps + 1):  # the first round warms up (and grows the scratch)
            eng.inflate_device(d_comp, n_comp, d_moff.data_ptr(), n_members, out)
            eng.sync()
            s, d = eng.inflate_time_ms()
            scan.append(s)
            decode.append(d)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            copy_dst.copy_(t["text"][64:64 + n_text])
            e1.record()
            torch.cuda.synchronize()
            copy.append(e0.elapsed_time(e1))
        info = read_info(t["info"])
        assert info == {"n_bytes": n_text, "n_members": n_members, "overflow": 0, "error": 0}, info
        got = t["text"][64:64 + n_distinct].cpu().numpy()
        assert (got == text).all(), "the inflated text differs from the input"
        zms = min(zlib_thread_ms(distinct)[0] for _ in range(2)) * reps
        sm, dm, cm = float(np.median(scan[1:])), float(np.median(decode[1:])), float(np.median(copy[1:]))
        ms = sm + dm
        result["levels"][str(level)] = {
            "members": n_members, "compressed_bytes": n_comp, "text_bytes": n_text, "ratio": round(n_text / n_comp, 3),
            "scan_ms": round(sm, 4), "decode_ms": round(dm, 4), "inflate_ms": round(ms, 4), "copy_text_ms": round(cm, 4),
            "inflate_over_copy": round(ms / cm, 2), "text_GB_per_s": round(n_text / ms / 1e6, 2),
            "zlib_one_thread_ms": round(zms, 1), "zlib_text_GB_per_s": round(n_text / zms / 1e6, 3), "zlib_over_device": round(zms / ms, 1),
            "ns_per_text_byte_per_wave": round(dm * 1e6 / (n_text / min(n_members, eng_waves(eng))), 2)}
        del store, copy_dst, t, out
        torch.cuda.empty_cache()
    eng.close()
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def eng_waves(eng):
    """decoder waves in flight: 24 blocks of one wave per compute unit (faqcs_inflate_kernel.hip)"""
    import torch

    return 24 * torch.cuda.get_device_properties(0).multi_processor_count


if __name__ == "__main__":
    main()
