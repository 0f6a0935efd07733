"""faqcs_inflate_device on the MI355X: the hand-built BGZF files of inflate_cases.py against Python's zlib and against the host statement
faqcs_inflate_host in every info field, the chain inflate -> parse -> submit -> render against the same chain fed with the plain text,
and the condition that the device call beats the 16 CPUs a process is allowed.  The damaged streams that go to the device here are the
ones tests/test_inflate_model.py has put through the same decoder text under the sanitizers on the host: they check a refusal."""
import ctypes as C

import numpy as np
import pytest

import inflate_cases as ic
import parse_cases as pc
from faqcs_amd import _capi as capi
from faqcs_amd.options import parse_args
from test_gpu_parity import SEED, random_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from faqcs_amd.engine import HipEngine

    e = HipEngine(parse_args(["-u", "x", "-d", "y", "--ascii", "33"]), 256, 33, device=0)
    yield e
    e.close()


def inflate_device(eng, comp, moff, capacity=None, with_offsets=True, shift=1, keep=False):
    """One faqcs_inflate_device into canary-filled device buffers; everything comes back as host arrays (the WHOLE buffers), in the form of
    inflate_cases.inflate_host.  shift: the compressed bytes start that many bytes behind a 256-byte aligned address."""
    import torch

    comp = bytes(comp)
    dev = torch.device("cuda:0")
    n = len(moff) - 1
    cap = 65536 * n + 8 if capacity is None else capacity
    d_comp = torch.zeros(shift + len(comp) + 1, dtype=torch.uint8, device=dev)
    if comp:
        d_comp[shift:shift + len(comp)] = torch.from_numpy(np.frombuffer(comp, np.uint8).copy()).to(dev)
    d_moff = torch.from_numpy(np.ascontiguousarray(moff, dtype=np.uint32).view(np.int32).copy()).to(dev)
    text = torch.full((ic.FRONT + cap + 64,), ic.CANARY, dtype=torch.uint8, device=dev)
    mto = torch.full((n + 2,), -0x5A5A5A5B, dtype=torch.int32, device=dev)
    info = torch.full((3,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    assert (text.data_ptr() + ic.FRONT) % 16 == 0 and d_comp.data_ptr() % 256 == 0
    out = capi.InflateOut(text.data_ptr() + ic.FRONT, cap, mto.data_ptr() if with_offsets else None, info.data_ptr())
    eng.inflate_device(d_comp.data_ptr() + shift, len(comp), d_moff.data_ptr(), n, out)
    eng.sync()
    p = capi.InflateInfo.from_buffer_copy(info.cpu().numpy().tobytes())
    o = {"text": text.cpu().numpy(), "member_text_offset": mto.cpu().numpy().view(np.uint32), "with_offsets": with_offsets, "cap": cap,
         "info": {f: int(getattr(p, f)) for f, _ in capi.InflateInfo._fields_ if f != "reserved"}}
    assert p.reserved == 0
    if keep:
        o["d_text"] = text
    return o


def test_seeded_files_equal_zlib_and_the_host_statement(eng):
    """The files of the host test -- every shape, level, strategy, header variant and size, the EOF member --: the text equals zlib's, info
    equals faqcs_inflate_host's in every field, canaries in front of and behind the text beyond the 16-byte rounding; the compressed bytes
    at every alignment."""
    rng = np.random.Generator(np.random.PCG64([121, SEED]))
    edge = ic.edge_members(rng)
    files = [([m for m, _ in edge], [t for _, t in edge]), ([], [])] + [([m], [t]) for m, t in edge[:8]]
    for k in range(60):
        files.append(ic.random_file(rng, int(rng.integers(1, 12)), max_text=65280 if k % 6 == 0 else 6000))
    for k, (ms, ts) in enumerate(files):
        comp, moff = b"".join(ms), ic.offsets_of(ms)
        cap = sum(len(t) for t in ts)
        o = inflate_device(eng, comp, moff, capacity=cap, with_offsets=(k % 3 != 0), shift=k % 5)
        ic.assert_inflate(o, ts, round16=True, what="file %d" % k)
        rc, h = ic.inflate_host(eng.lib, comp, moff, capacity=cap)
        assert rc == 0 and h["info"] == o["info"], k


@pytest.mark.parametrize("kind", ic.DAMAGE)
def test_damaged_members_are_refused(eng, kind):
    """One change to one member in the middle of a file: the stated code, n_members = the member's index, the text in front of it byte-exact,
    nothing outside the scanned total touched; info equals the host statement's."""
    rng = np.random.Generator(np.random.PCG64([123, ic.DAMAGE.index(kind), SEED]))
    for rnd in range(4 if kind == "bitflip" else 2):
        ms, ts = ic.random_file(rng, 9, max_text=5000)
        bad = int(rng.integers(1, 8))
        text = ic.shape_text(rng, "fastq", int(rng.integers(2000, 6000)))
        ms[bad], ts[bad] = ic.damaged(rng, kind, text), text
        comp, moff = b"".join(ms), ic.offsets_of(ms)
        rc, h = ic.inflate_host(eng.lib, comp, moff)
        assert rc == 0
        ic.assert_inflate(h, ts, bad=bad, code=ic.DAMAGE_CODE[kind], what="host %s" % kind)  # (first: the refusal is the host's before it is the device's)
        o = inflate_device(eng, comp, moff)
        ic.assert_inflate(o, ts, bad=bad, code=ic.DAMAGE_CODE[kind], round16=True, what="%s round %d" % (kind, rnd))
        assert o["info"] == h["info"]


def test_a_file_of_100_000_members(eng):
    """>= 100 000 members of mixed shapes and levels (a few hundred distinct ones, drawn at random), the compressed bytes at an odd address."""
    rng = np.random.Generator(np.random.PCG64([127, SEED]))
    pool = [ic.random_member(rng, max_text=2500) for _ in range(300)] + [(ic.EOF_MEMBER, b"")] + ic.edge_members(rng)[:6]
    pick = rng.integers(0, len(pool), 100_500)
    ms, ts = [pool[i][0] for i in pick], [pool[i][1] for i in pick]
    o = inflate_device(eng, b"".join(ms), ic.offsets_of(ms), capacity=sum(len(t) for t in ts), shift=3)
    ic.assert_inflate(o, ts, round16=True, what="100 500 members")


def test_overflow_writes_nothing_but_info(eng):
    rng = np.random.Generator(np.random.PCG64([131, SEED]))
    ms, ts = ic.random_file(rng, 40, max_text=4000)
    nb = sum(len(t) for t in ts)
    o = inflate_device(eng, b"".join(ms), ic.offsets_of(ms), capacity=nb - 1)
    assert o["info"] == {"n_bytes": nb, "n_members": 40, "overflow": 1, "error": 0}
    ic.assert_nothing_written(o)
    o = inflate_device(eng, b"".join(ms), ic.offsets_of(ms), capacity=nb)
    ic.assert_inflate(o, ts, round16=True)
    a, g = eng.inflate_time_ms()
    assert a > 0 and g > 0


def test_argument_checks(eng):
    import torch

    lib = eng.lib
    dev = torch.device("cuda:0")
    buf = torch.zeros(4096, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    base = buf.data_ptr()
    assert base % 16 == 0

    def out(**kw):
        f = dict(text=base + 1024, capacity_bytes=512, member_text_offset=base + 2048, info=base + 3072)
        f.update(kw)
        return capi.InflateOut(**f)

    for bad in (out(text=base + 1028), out(text=None), out(info=None)):
        assert lib.faqcs_inflate_device(eng.ctx, base, 100, base + 512, 1, C.byref(bad)) == capi.E_INVAL
    good = out()
    assert lib.faqcs_inflate_device(eng.ctx, None, 100, base + 512, 1, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_inflate_device(eng.ctx, base, 100, None, 1, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_inflate_device(eng.ctx, base, 1 << 32, base + 512, 1, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_inflate_device(eng.ctx, base, 100, base + 512, 4, C.byref(good)) == capi.E_INVAL
    assert lib.faqcs_inflate_device(eng.ctx, base, 100, base + 512, 1, None) == capi.E_INVAL
    eng.sync()
    assert int(buf.sum()) == 0
    assert lib.faqcs_inflate_device(eng.ctx, None, 0, None, 0, C.byref(good)) == 0  # no members: zeros
    eng.sync()
    h = buf.cpu().numpy()
    assert not h[3072:3096].any() and not h[1024:2048].any() and not h[2048:2052].any()


def _four_files(hip, d_text, n_text, m, final=True):
    """parse -> submit -> render of QC.1, QC.2, unpaired and discard of a paired text (mate 1 then mate 2, m records each) -> the four texts"""
    import torch

    from faqcs_amd.device import rendered_fastq
    from faqcs_amd.engine import _check
    from tools.parse_bench import parse_buffers, read_info

    dev = d_text.device
    n = 2 * m
    pout, t = parse_buffers(dev, n_text, n)
    torch.cuda.synchronize()
    hip.parse_device(d_text.data_ptr(), n_text, final, pout)
    hip.sync()
    pinfo = read_info(t["info"])
    assert (pinfo["n_reads"], pinfo["error"], pinfo["overflow"], pinfo["consumed"]) == (n, 0, 0, n_text)
    seg = np.array([0, m, n], dtype=np.uint32)
    res = torch.zeros((n, 4), dtype=torch.int16, device=dev)
    b = capi.Batch(t["seq"].data_ptr() + 64, t["qual"].data_ptr() + 64, t["offset"].data_ptr(), n, 2, seg.ctypes.data, pinfo["max_read_len"], t["terminal_n"].data_ptr())
    _check(hip.lib, hip.lib.faqcs_submit_device(hip.ctx, C.byref(b), res.data_ptr()))
    hip.sync()
    valid = (res[:, 2] & 1) != 0
    v1, v2 = valid[:m], valid[m:]
    zero = torch.zeros_like(v1)
    inter = torch.stack([torch.arange(m, device=dev), torch.arange(m, device=dev) + m], dim=1).reshape(-1).to(torch.int32)
    nb = pinfo["n_bytes"]
    plans = ((True, torch.cat([v1 & v2, zero]), None), (True, torch.cat([zero, v1 & v2]), None), (True, torch.cat([v1 ^ v2, v1 ^ v2]), inter),
             (False, torch.cat([~v1, ~v2]), inter))
    files = []
    for with_res, sel, order in plans:
        txt, _ = rendered_fastq(hip, d_text, t["def_pos"][:n], t["def_len"][:n], t["seq"][64:64 + nb], t["qual"][64:64 + nb], t["offset"][:n + 1],
                                results=res if with_res else None, select=sel, order=order, terminal_n=t["terminal_n"][:n])
        files.append(txt.cpu().numpy().tobytes())
    return files


@pytest.mark.parametrize("args", [[], ["--adapter", "--polyA"], ["--replace_to_N_q", "15"]], ids=lambda a: " ".join(a) or "default")
def test_round_trip_inflate_parse_submit_render(args):
    """BGZF bytes -> faqcs_inflate_device -> faqcs_parse_device -> faqcs_submit_device -> faqcs_render_device of the four files equals the same
    chain fed with the plain text; and the members fed in three calls -- each call's text laid behind the tail the parse (final = 0) of the
    text so far left over -- give the text, and so the files, of the one call."""
    import torch

    from faqcs_amd.device import inflated_text
    from faqcs_amd.engine import HipEngine
    from tools.parse_bench import parse_buffers, read_info

    rng = np.random.Generator(np.random.PCG64([137, len(args), SEED]))
    m = 350 if "--adapter" in args else 1500
    reads = random_batch(rng, 2 * m, 150, "adv")
    text = b"".join(b"@r%d/%d\n" % (i % m, 1 + i // m) + s + b"\n+\n" + q + b"\n" for i, (d, s, q) in enumerate(reads))
    cuts = [0]
    while cuts[-1] < len(text):  # members end anywhere in a record
        cuts.append(min(len(text), cuts[-1] + int(rng.integers(3000, 45000))))
    ms = [ic.member(text[a:b], ic.LEVELS[int(rng.integers(0, 4))]) for a, b in zip(cuts[:-1], cuts[1:])] + [ic.EOF_MEMBER]
    dev = torch.device("cuda:0")
    hip = HipEngine(parse_args(["-u", "x", "-d", "y", "--ascii", "33"] + args), 256, 33, device=0)
    plain = torch.full((64 + len(text) + 64,), 10, dtype=torch.uint8, device=dev)
    plain[64:64 + len(text)] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(dev)
    want = _four_files(hip, plain[64:64 + len(text)], len(text), m)
    assert sum(len(f) for f in want) > 0
    # one call
    comp = torch.from_numpy(np.frombuffer(b"".join(ms), np.uint8).copy()).to(dev)
    d_text, mto = inflated_text(hip, comp, ic.offsets_of(ms))
    assert int(d_text.numel()) == len(text) and d_text.data_ptr() % 16 == 0 and int(mto[-1]) == len(text)
    assert _four_files(hip, d_text, len(text), m) == want
    # three calls, the tail carried
    bounds = [0, len(ms) // 3, 2 * len(ms) // 3, len(ms)]
    store = torch.full((64 + len(text) + 64,), 10, dtype=torch.uint8, device=dev)
    have, done, n_reads = 0, 0, 0  # text bytes in `store` behind byte 64; text bytes the parse has consumed in all; records so far
    for a, b in zip(bounds[:-1], bounds[1:]):
        part = ms[a:b]
        piece, _ = inflated_text(hip, torch.from_numpy(np.frombuffer(b"".join(part), np.uint8).copy()).to(dev), ic.offsets_of(part))
        store[64 + have:64 + have + piece.numel()] = piece  # (behind the carried tail)
        have += int(piece.numel())
        pout, t = parse_buffers(dev, have, have // 4 + 8)
        torch.cuda.synchronize()
        hip.parse_device(store.data_ptr() + 64, have, b == len(ms), pout)
        hip.sync()
        pinfo = read_info(t["info"])
        assert pinfo["error"] == 0 and pinfo["overflow"] == 0
        c = pinfo["consumed"]
        assert bytes(store[64:64 + c].cpu().numpy()) == text[done:done + c]
        n_reads += pinfo["n_reads"]
        done += c
        tail = store[64 + c:64 + have].clone()
        store[64:64 + tail.numel()] = tail
        have = int(tail.numel())
    assert (done, have, n_reads) == (len(text), 0, 2 * m)
    hip.close()


def test_inflate_is_not_serialised(eng):
    """A condition, not a measurement: 256 MiB of 2x150-shaped text as level-6 members of 65 280 bytes, 64 MiB of it distinct
    (tools/inflate_bench.py builds it).  The median of 5 HIP-event timings of faqcs_inflate_device must be below the time ONE zlib thread
    needs for the same members in the same process, divided by 16 -- the CPUs a process is allowed here (DESIGN.md sections 5 and 9-5):
    below that the device call has no reason to exist beside the host reader."""
    import torch

    from tools.inflate_bench import build_file, inflate_buffers, read_info, upload, zlib_thread_ms

    dev = torch.device("cuda:0")
    distinct, reps, n_distinct, text = build_file(6, 256, 64)
    n_text, n_members = n_distinct * reps, len(distinct) * reps
    assert n_text >= 256 << 20 and n_distinct >= 64 << 20
    store, d_comp, n_comp, d_moff = upload(dev, distinct, reps)
    out, t = inflate_buffers(dev, n_text, n_members)
    torch.cuda.synchronize()
    ms = []
    for rep in range(6):  # the first round warms up
        eng.inflate_device(d_comp, n_comp, d_moff.data_ptr(), n_members, out)
        eng.sync()
        ms.append(sum(eng.inflate_time_ms()))
    assert read_info(t["info"]) == {"n_bytes": n_text, "n_members": n_members, "overflow": 0, "error": 0}
    for r in (0, reps - 1):
        assert (t["text"][64 + r * n_distinct:64 + (r + 1) * n_distinct].cpu().numpy() == text).all()
    z_ms, z_bytes = zlib_thread_ms(distinct)
    z_ms2, _ = zlib_thread_ms(distinct)
    z_ms = min(z_ms, z_ms2) * reps
    assert z_bytes == n_distinct
    dm = float(np.median(ms[1:]))
    print("faqcs_inflate_device %.3f ms (%.2f GB/s of text), one zlib thread %.1f ms (%.3f GB/s), ratio %.1f (needed: > 16)" % (
        dm, n_text / dm / 1e6, z_ms, n_text / z_ms / 1e6, z_ms / dm))
    assert dm < z_ms / 16, "faqcs_inflate_device %.3f ms vs %.1f ms / 16 = %.3f ms for one zlib thread" % (dm, z_ms, z_ms / 16)
