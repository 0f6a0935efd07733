"""Torch-facing helpers of the device seam: inputs and outputs are torch tensors that live on the GPU; the work is the
library's HIP kernels (faqcs_emit_device, faqcs_render_device, faqcs_pair_device, faqcs_render_pair_device, faqcs_bgzf_index_device, faqcs_inflate_device,
faqcs_gunzip_device, faqcs_deflate_device, faqcs_detect_device), never torch ops."""
import ctypes as C

from . import _capi as capi
from .engine import FaqcsError


def trimmed_reads(engine, seq, qual, offset, results, keep=None, terminal_n=None):
    """The trimmed, edited reads of a device-resident batch, packed back to back on the device.

    seq / qual: uint8 CUDA tensors whose element 0 is the batch's byte 0 (padding contract of faqcs_batch: 16 readable bytes in
    front, 64 behind -- pass a view into a larger tensor); offset: int32 / uint32 tensor [n + 1]; results: the (n, 4) int16 tensor
    faqcs_submit_device() filled on `engine`; keep: optional uint8 / bool tensor [n] (0 = do not emit); terminal_n: optional uint8
    tensor [n] (faqcs_batch.terminal_n).  Returns (seq, qual, offset, index): uint8 [n_bytes] x 2, int32 [n_emitted + 1] (bit
    pattern of uint32), int32 [n_emitted] (input index of every emitted read).  The returned seq / qual are views that start
    16-byte aligned, 64 bytes into their storage, with 64 spare bytes behind: a valid input batch for faqcs_submit_device()."""
    import torch

    n = int(offset.numel()) - 1
    dev = seq.device
    cap = int(seq.numel())  # an emission never exceeds the input bytes
    front = 64
    o_seq = torch.empty(front + cap + capi.ARENA_PAD_AFTER + 16, dtype=torch.uint8, device=dev)
    o_qual = torch.empty_like(o_seq)
    o_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
    o_idx = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    info = torch.zeros(2, dtype=torch.int64, device=dev)
    shift = [(-(t.data_ptr() + front)) % 16 for t in (o_seq, o_qual)]
    if keep is not None:
        keep = keep.to(torch.uint8).contiguous()
    batch = capi.Batch(seq.data_ptr(), qual.data_ptr(), offset.data_ptr(), n, 0, None, 0,
                       terminal_n.data_ptr() if terminal_n is not None and n else None)
    out = capi.EmitOut(o_seq.data_ptr() + front + shift[0], o_qual.data_ptr() + front + shift[1], cap, o_off.data_ptr(),
                       o_idx.data_ptr(), info.data_ptr())
    torch.cuda.current_stream(dev).synchronize()  # the library's compute stream is its own: the inputs must be complete
    engine.emit_device(batch, results.data_ptr(), out, keep.data_ptr() if keep is not None and n else None)
    engine.sync()
    h = info.cpu().numpy()
    n_bytes, n_emit, overflow = int(h[0]), int(h[1]) & 0xFFFFFFFF, int(h[1]) >> 32
    if overflow:
        raise FaqcsError(capi.E_INVAL, "faqcs_emit_device: the emission needs %d bytes, the output arenas hold %d" % (n_bytes, cap))
    a, b = front + shift[0], front + shift[1]
    return o_seq[a:a + n_bytes], o_qual[b:b + n_bytes], o_off[:n_emit + 1], o_idx[:n_emit]


def rendered_fastq(engine, text, def_pos, def_len, seq, qual, offset, results=None, select=None, order=None, terminal_n=None, capacity=None):
    """The FASTQ text of one output file of a device-resident batch, assembled on the device (faqcs_render_device).

    text: uint8 CUDA tensor whose element 0 is byte 0 of the FASTQ text faqcs_parse_device() indexed (its padding: 16 readable bytes in
    front, 64 behind -- pass a view into a larger tensor); def_pos / def_len: int32 / uint32 tensors [n], the defline spans that parse
    delivered; seq / qual / offset / terminal_n: the batch, as for trimmed_reads(); results: the (n, 4) int16 tensor faqcs_submit_device()
    filled on `engine` -- the trimmed, edited records -- or None for the original records (the discard stream); select: optional uint8 /
    bool tensor [n] (0 = do not render); order: optional int32 tensor [n], candidate j is read order[j].  capacity: bytes of text to make
    room for (default: the input text's size plus 5 bytes per read, which no rendering of distinct reads exceeds).
    Returns (text, rec_offset): uint8 [n_bytes] -- a view that starts 16-byte aligned --, int32 [n_rendered + 1] (bit pattern of uint32)."""
    import torch

    n = int(offset.numel()) - 1
    dev = seq.device
    cap = int(text.numel()) + 5 * n if capacity is None else int(capacity)
    o_text = torch.empty(cap + capi.ARENA_PAD_AFTER + 16, dtype=torch.uint8, device=dev)
    o_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
    info = torch.zeros(2, dtype=torch.int64, device=dev)
    shift = (-o_text.data_ptr()) % 16
    if select is not None:
        select = select.to(torch.uint8).contiguous()
    if order is not None:
        order = order.to(torch.int32).contiguous()
    batch = capi.Batch(seq.data_ptr(), qual.data_ptr(), offset.data_ptr(), n, 0, None, 0,
                       terminal_n.data_ptr() if terminal_n is not None and n else None)
    out = capi.RenderOut(o_text.data_ptr() + shift, cap, o_off.data_ptr(), None, info.data_ptr())
    torch.cuda.current_stream(dev).synchronize()  # the library's compute stream is its own: the inputs must be complete
    engine.render_device(batch, results.data_ptr() if results is not None else None, text.data_ptr(), def_pos.data_ptr(), def_len.data_ptr(), out,
                         select.data_ptr() if select is not None and n else None, order.data_ptr() if order is not None and n else None)
    engine.sync()
    h = info.cpu().numpy()
    n_bytes, n_rec, overflow = int(h[0]), int(h[1]) & 0xFFFFFFFF, int(h[1]) >> 32
    if overflow:
        raise FaqcsError(capi.E_INVAL, "faqcs_render_device: the text needs %d bytes, the output holds %d" % (n_bytes, cap))
    return o_text[shift:shift + n_bytes], o_off[:n_rec + 1]


class DeviceMate:
    """One mate of a paired run in device memory, as faqcs_parse_device + faqcs_submit_device left it: text (uint8 CUDA tensor whose element
    0 is byte 0 of the text the parse indexed, with that text's padding), def_pos / def_len (int32 / uint32 [n]), seq / qual / offset /
    terminal_n (the batch, as for rendered_fastq()), results (the (n, 4) int16 tensor of the submission, or None before it)."""

    def __init__(self, text, def_pos, def_len, seq, qual, offset, results=None, terminal_n=None):
        self.text, self.def_pos, self.def_len, self.seq, self.qual, self.offset = text, def_pos, def_len, seq, qual, offset
        self.results, self.terminal_n = results, terminal_n
        self.n = int(offset.numel()) - 1

    def capi(self):
        """-> capi.Mate (it keeps its capi.Batch alive)"""
        n = self.n
        b = capi.Batch(self.seq.data_ptr(), self.qual.data_ptr(), self.offset.data_ptr(), n, 0, None, 0,
                       self.terminal_n.data_ptr() if self.terminal_n is not None and n else None)
        m = capi.Mate(C.pointer(b), self.results.data_ptr() if self.results is not None else None, self.text.data_ptr(),
                      self.def_pos.data_ptr(), self.def_len.data_ptr())
        m._batch = b
        return m


def first_buffer_decisions(engine, mate1, mate2=None, first=0, count=None):
    """The decisions the reference takes on its first buffer, for device-resident mates (DeviceMate each; faqcs_detect_device): the
    quality-offset auto-detect and the NextSeq look at the first defline over reads [first, first + count) of each mate (count None: up
    to capi.SEGMENT_READS reads, the reference's buffer).  Only the infos come back to the host.  Returns the dict of the
    faqcs_detect_info fields of mate1, or a tuple of two dicts when mate2 is given (the caller compares the two verdicts: the reference
    stops with "Inconsistent quality offset detection between reads one and two")."""
    import torch

    mates = [m for m in (mate1, mate2) if m is not None]
    dev = mate1.text.device
    d_info = torch.zeros((len(mates), 6), dtype=torch.int32, device=dev)
    torch.cuda.current_stream(dev).synchronize()  # the library's compute stream is its own: the inputs must be complete
    keep = []
    for k, m in enumerate(mates):
        c = max(0, min(m.n - first, capi.SEGMENT_READS)) if count is None else int(count)
        cm = m.capi()
        keep.append(cm)
        engine.detect_device(cm._batch, first, c, d_info[k].data_ptr(), m.text.data_ptr(), m.def_pos.data_ptr(), m.def_len.data_ptr())
    engine.sync()
    h = d_info.cpu().numpy()
    out = []
    for k in range(len(mates)):
        p = capi.DetectInfo.from_buffer_copy(h[k].tobytes())
        out.append({f: int(getattr(p, f)) for f, _ in capi.DetectInfo._fields_})
    return out[0] if mate2 is None else tuple(out)


def pair_route(engine, mate1, mate2):
    """The pair stage of two device-resident mates (DeviceMate each; faqcs_pair_device): the id check of FaQCs.cpp:382-389, the route of
    every pair and the two FilterStat slots that depend on both mates.  With results on neither mate only the ids are checked and route is
    None.  Returns (route, info): uint8 CUDA tensor [min(n1, n2)] of capi.ROUTE_* bits (pairs behind a mismatch: ROUTE_NOWHERE) and a dict
    of the faqcs_pair_info fields; with info["mismatch"] the ids of pair info["n_pairs"] are the first info["id_len"][s] bytes of mate s's
    defline, and info["ids"] holds them (downloaded for the reference's message)."""
    import torch

    dev = mate1.text.device
    n = min(mate1.n, mate2.n)
    routed = mate1.results is not None
    route = torch.empty(max(n, 1), dtype=torch.uint8, device=dev) if routed else None
    d_info = torch.zeros(5, dtype=torch.int64, device=dev)
    torch.cuda.current_stream(dev).synchronize()  # the library's compute stream is its own: the inputs must be complete
    engine.pair_device(mate1.capi(), mate2.capi(), route.data_ptr() if routed else None, d_info.data_ptr())
    engine.sync()
    p = capi.PairInfo.from_buffer_copy(d_info.cpu().numpy().tobytes())
    info = {f: int(getattr(p, f)) for f, _ in capi.PairInfo._fields_ if f != "id_len"}
    info["id_len"] = (int(p.id_len[0]), int(p.id_len[1]))
    if info["mismatch"]:
        i = info["n_pairs"]
        info["ids"] = tuple(bytes(m.text[int(m.def_pos[i]) & 0xFFFFFFFF:(int(m.def_pos[i]) & 0xFFFFFFFF) + ln].cpu().numpy())
                            for m, ln in zip((mate1, mate2), info["id_len"]))
    return (route[:n] if routed else None), info


def paired_files(engine, mate1, mate2, route, n_pairs, files=(capi.FILE_QC1, capi.FILE_QC2, capi.FILE_UNPAIRED, capi.FILE_DISCARD), capacity=None):
    """The FASTQ text of the files of a paired run from two device-resident mates (DeviceMate each) and the route pair_route() delivered,
    assembled on the device (faqcs_render_pair_device, one call per file).  files: capi.FILE_* codes; capacity: bytes of text to make room
    for per file (default: both input texts plus 5 bytes per read, which no file exceeds).
    Returns {file: (text, rec_offset)}: uint8 [n_bytes] -- a view that starts 16-byte aligned --, int32 [n_rendered + 1] (bit pattern of uint32)."""
    import torch

    dev = mate1.text.device
    n_pairs = int(n_pairs)
    cap = int(mate1.text.numel()) + int(mate2.text.numel()) + 10 * n_pairs if capacity is None else int(capacity)
    m1, m2 = mate1.capi(), mate2.capi()
    torch.cuda.current_stream(dev).synchronize()  # the library's compute stream is its own: the inputs must be complete
    outs = {}
    for f in files:
        o_text = torch.empty(cap + capi.ARENA_PAD_AFTER + 16, dtype=torch.uint8, device=dev)
        o_off = torch.empty(2 * n_pairs + 1, dtype=torch.int32, device=dev)
        info = torch.zeros(2, dtype=torch.int64, device=dev)
        shift = (-o_text.data_ptr()) % 16
        out = capi.RenderOut(o_text.data_ptr() + shift, cap, o_off.data_ptr(), None, info.data_ptr())
        torch.cuda.current_stream(dev).synchronize()
        engine.render_pair_device(f, m1, m2, route.data_ptr() if n_pairs else None, n_pairs, out)
        outs[f] = (o_text, o_off, info, shift)
    engine.sync()
    res = {}
    for f, (o_text, o_off, info, shift) in outs.items():
        h = info.cpu().numpy()
        n_bytes, n_rec, overflow = int(h[0]), int(h[1]) & 0xFFFFFFFF, int(h[1]) >> 32
        if overflow:
            raise FaqcsError(capi.E_INVAL, "faqcs_render_pair_device: the text needs %d bytes, the output holds %d" % (n_bytes, cap))
        res[f] = (o_text[shift:shift + n_bytes], o_off[:n_rec + 1])
    return res


def bgzf_index(engine, comp, final=True, capacity=None):
    """Where the BGZF members of `comp` are, found on the device (faqcs_bgzf_index_device): `comp` never leaves the card.

    comp: uint8 CUDA tensor, the compressed bytes (any alignment); final: an incomplete last member is an error (True) or left to the
    caller (False); capacity: members to make room for (default: one per 16 KiB and 64 more, and the call is repeated once with what
    info asks for when that is too little).  Returns (member_offset, n_members, consumed, error): int32 CUDA tensor [n_members + 1] (bit
    pattern of uint32) -- member k is comp[member_offset[k] : member_offset[k + 1]] --, where the next chunk starts, and a capi.INFLATE_*
    code, the error of member n_members: field for field what engine.bgzf_index_host() returns for the same bytes."""
    import torch

    dev = comp.device
    comp = comp.contiguous()
    n_comp = int(comp.numel())
    cap = n_comp // 16384 + 64 if capacity is None else int(capacity)
    info = torch.zeros(3, dtype=torch.int64, device=dev)
    torch.cuda.current_stream(dev).synchronize()  # the library's compute stream is its own: the input must be complete
    for attempt in range(2):
        moff = torch.empty(cap + 1, dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        engine.bgzf_index_device(comp.data_ptr() if n_comp else None, n_comp, final, moff.data_ptr(), cap, info.data_ptr())
        engine.sync()
        p = capi.BgzfIndexInfo.from_buffer_copy(info.cpu().numpy().tobytes())
        if not p.overflow:
            return moff[:p.n_members + 1], int(p.n_members), int(p.consumed), int(p.error)
        if attempt:
            raise FaqcsError(capi.E_INVAL, "faqcs_bgzf_index_device: %d members, the offsets hold %d" % (p.n_members, cap))
        cap = int(p.n_members)


def inflated_text(engine, comp, member_offset=None, capacity=None, index="host"):
    """The text of BGZF-compressed input, inflated on the device (faqcs_inflate_device).

    comp: uint8 CUDA tensor, the compressed bytes (whole members; any alignment); member_offset: int32 / uint32 tensor or numpy array
    [n_members + 1], or None: the members are found on the host (index="host": faqcs_bgzf_index_host, which copies `comp` there -- a
    caller that uploads a file has those bytes on the host already and passes the offsets) or on the device (index="device":
    faqcs_bgzf_index_device, `comp` never leaves the card).  capacity: bytes of text to make room for (default
    65 536 per member, which no member exceeds).  Returns (text, member_text_offset): uint8 [n_bytes] -- a view that starts 16-byte
    aligned, 64 bytes into its storage, with 64 spare bytes behind: a valid d_text for faqcs_parse_device() --, int32 [n_members + 1]
    (bit pattern of uint32).  A bad member raises FaqcsError with faqcs_inflate_error_text and the member's index."""
    import numpy as np
    import torch

    dev = comp.device
    if index not in ("host", "device"):
        raise ValueError("index: 'host' or 'device'")
    if member_offset is None and index == "device":
        member_offset, n_mem, consumed, err = bgzf_index(engine, comp, True)
        if err:
            raise FaqcsError(capi.E_INVAL, "member %d: %s" % (n_mem, engine.lib.faqcs_inflate_error_text(err).decode()))
    if member_offset is None:
        from .engine import bgzf_index_host
        moff, consumed, err = bgzf_index_host(comp.cpu().numpy(), True, engine.lib)
        if err:
            raise FaqcsError(capi.E_INVAL, "member %d: %s" % (len(moff) - 1, engine.lib.faqcs_inflate_error_text(err).decode()))
        member_offset = moff
    if isinstance(member_offset, np.ndarray):
        member_offset = torch.from_numpy(member_offset.astype(np.int64).astype(np.uint32).view(np.int32)).to(dev)
    member_offset = member_offset.contiguous()
    n = int(member_offset.numel()) - 1
    cap = 65536 * n if capacity is None else int(capacity)
    front = 64
    o_text = torch.empty(front + cap + capi.ARENA_PAD_AFTER + 16, dtype=torch.uint8, device=dev)
    o_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
    info = torch.zeros(3, dtype=torch.int64, device=dev)
    shift = (-(o_text.data_ptr() + front)) % 16
    out = capi.InflateOut(o_text.data_ptr() + front + shift, cap, o_off.data_ptr(), info.data_ptr())
    torch.cuda.current_stream(dev).synchronize()  # the library's compute stream is its own: the inputs must be complete
    engine.inflate_device(comp.data_ptr(), int(comp.numel()), member_offset.data_ptr(), n, out)
    engine.sync()
    h = info.cpu().numpy()
    n_bytes, n_mem, overflow, error = int(h[0]), int(h[1]) & 0xFFFFFFFF, int(h[1]) >> 32, int(h[2]) & 0xFFFFFFFF
    if overflow:
        raise FaqcsError(capi.E_INVAL, "faqcs_inflate_device: the text needs %d bytes, the output holds %d" % (n_bytes, cap))
    if error:
        raise FaqcsError(capi.E_INVAL, "member %d: %s" % (n_mem, engine.lib.faqcs_inflate_error_text(error).decode()))
    a = front + shift
    return o_text[a:a + n_bytes], o_off[:n_mem + 1]


def gunzipped_text(engine, comp, capacity=None, piece_bytes=0, max_rounds=0):
    """The text of ordinary gzip input, inflated by pieces on the device (faqcs_gunzip_device); the call blocks.

    comp: uint8 CUDA tensor, the compressed bytes (one or more whole gzip members -- gzip, pigz, bgzip output alike; any alignment);
    capacity: bytes of text to make room for (default: four times the compressed bytes, and the call is repeated once with what info
    asks for when that is too little); piece_bytes / max_rounds: 0 for the defaults.  Returns the text: uint8 [n_bytes] -- a view that
    starts 16-byte aligned, 64 bytes into its storage, with 64 spare bytes behind: a valid d_text for faqcs_parse_device().  A bad member
    raises FaqcsError with the member's index and faqcs_inflate_error_text (capi.INFLATE_E_SERIAL: inflate this input on the host)."""
    import torch

    dev = comp.device
    comp = comp.contiguous()
    n_comp = int(comp.numel())
    cap = 4 * n_comp + 4096 if capacity is None else int(capacity)
    front = 64
    info = torch.zeros(5, dtype=torch.int64, device=dev)
    torch.cuda.current_stream(dev).synchronize()  # the library's compute stream is its own: the input must be complete
    for attempt in range(2):
        o_text = torch.empty(front + cap + capi.ARENA_PAD_AFTER + 16, dtype=torch.uint8, device=dev)
        shift = (-(o_text.data_ptr() + front)) % 16
        out = capi.GunzipOut(o_text.data_ptr() + front + shift, cap, info.data_ptr())
        torch.cuda.current_stream(dev).synchronize()
        engine.gunzip_device(comp.data_ptr() if n_comp else None, n_comp, out, piece_bytes, max_rounds)
        p = capi.GunzipInfo.from_buffer_copy(info.cpu().numpy().tobytes())
        if not p.overflow:
            break
        if attempt or p.n_bytes >= 1 << 32:
            raise FaqcsError(capi.E_INVAL, "faqcs_gunzip_device: the text needs %d bytes, the output holds %d" % (p.n_bytes, cap))
        cap = int(p.n_bytes)
    if p.error:
        raise FaqcsError(capi.E_INVAL, "member %d: %s" % (p.n_members, engine.lib.faqcs_inflate_error_text(p.error).decode()))
    a = front + shift
    return o_text[a:a + int(p.n_bytes)]


class GunzipStream:
    """One ordinary gzip file fed to the device in chunks (faqcs_gunzip_stream_device).  It owns what goes from call to call: the state
    (host memory) and the 32 KiB window (device memory).  Two files are two GunzipStreams on one engine, fed in any order."""

    def __init__(self, engine, device=None, piece_bytes=0, max_rounds=0):
        import torch

        self.engine, self.piece_bytes, self.max_rounds = engine, piece_bytes, max_rounds
        self.window = torch.zeros(capi.GUNZIP_WINDOW, dtype=torch.uint8, device=device if device is not None else "cuda")
        self.state = capi.GunzipState()
        self.state.window = self.window.data_ptr()

    def feed(self, comp, final, capacity=None):
        """comp: uint8 CUDA tensor, the file from where the previous feed's info.consumed left it (any alignment); final: these are its
        last bytes.  capacity: bytes of text to make room for (default: four times the compressed bytes; the call is repeated once with
        what info asks for when that is too little -- an overflow leaves the state alone).  Returns (text, info): the text this call
        delivered, uint8 [n_bytes], a view laid out as gunzipped_text()'s, and the capi.GunzipInfo.  info.consumed == 0 with no text:
        the chunk holds no whole block, feed a larger one.  A bad member does NOT raise: info.error is its code (see
        engine.lib.faqcs_inflate_error_text; member self.state.members of the file), and text, info.consumed and the state are those of
        the members in front of it within this call, which the caller still has to take -- the state says they were handed on."""
        import torch

        dev = comp.device
        comp = comp.contiguous()
        n_comp = int(comp.numel())
        cap = 4 * n_comp + 4096 if capacity is None else int(capacity)
        front = 64
        info = torch.zeros(5, dtype=torch.int64, device=dev)
        for attempt in range(2):
            o_text = torch.empty(front + cap + capi.ARENA_PAD_AFTER + 16, dtype=torch.uint8, device=dev)
            shift = (-(o_text.data_ptr() + front)) % 16
            out = capi.GunzipOut(o_text.data_ptr() + front + shift, cap, info.data_ptr())
            torch.cuda.current_stream(dev).synchronize()  # the library's compute stream is its own: the input must be complete
            self.engine.gunzip_stream_device(comp.data_ptr() if n_comp else None, n_comp, final, self.state, out, self.piece_bytes, self.max_rounds)
            p = capi.GunzipInfo.from_buffer_copy(info.cpu().numpy().tobytes())
            if not p.overflow:
                break
            if attempt or p.n_bytes >= (1 << 32) - capi.GUNZIP_WINDOW:
                raise FaqcsError(capi.E_INVAL, "faqcs_gunzip_stream_device: the text needs %d bytes, the output holds %d; feed a shorter chunk" % (p.n_bytes, cap))
            cap = int(p.n_bytes)
        a = front + shift
        return o_text[a:a + int(p.n_bytes)], p


def deflated_bgzf(engine, text, member_bytes=0, final=True, capacity=None, mode=capi.DEFLATE_FAST):
    """`text` as BGZF members, compressed on the device (faqcs_deflate_device_mode).

    text: uint8 CUDA tensor (any alignment); member_bytes: text bytes per member (0: 65 280, as bgzip cuts); final: append the EOF member;
    mode: capi.DEFLATE_FAST (the default) or capi.DEFLATE_DENSE, smaller members for more time;
    capacity: bytes to make room for (default: half the text, and the call is repeated once with what info asks for when that is too
    little).  Returns (comp, member_offset): uint8 [n_bytes], a view that starts 16-byte aligned, and int32 [n_members + 1] (bit pattern of
    uint32) -- with n_members = len(member_offset) - 1 the arguments faqcs_inflate_device takes."""
    import torch

    dev = text.device
    text = text.contiguous()
    n_text = int(text.numel())
    mb = int(member_bytes) or 65280
    n = (n_text + mb - 1) // mb + (1 if final else 0)
    cap = n_text // 2 + 31 * n + 64 if capacity is None else int(capacity)
    o_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
    info = torch.zeros(3, dtype=torch.int64, device=dev)
    torch.cuda.current_stream(dev).synchronize()  # the library's compute stream is its own: the input must be complete
    for attempt in range(2):
        o_comp = torch.empty(cap + capi.ARENA_PAD_AFTER + 32, dtype=torch.uint8, device=dev)
        shift = (-o_comp.data_ptr()) % 16
        out = capi.DeflateOut(o_comp.data_ptr() + shift, cap, o_off.data_ptr(), info.data_ptr())
        torch.cuda.current_stream(dev).synchronize()
        engine.deflate_device(text.data_ptr() if n_text else None, n_text, int(member_bytes), final, out, mode=mode)
        engine.sync()
        h = info.cpu().numpy()
        n_bytes, n_mem, overflow = int(h[0]), int(h[1]) & 0xFFFFFFFF, int(h[1]) >> 32
        if not overflow:
            return o_comp[shift:shift + n_bytes], o_off[:n_mem + 1]
        if attempt or n_bytes >= 1 << 32:
            raise FaqcsError(capi.E_INVAL, "faqcs_deflate_device: the members need %d bytes, the output holds %d" % (n_bytes, cap))
        cap = n_bytes
