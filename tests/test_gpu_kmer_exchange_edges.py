"""The catalogue of tests/kmer_exchange_edges.py on an MI355X: the owner-partitioned k-mer exchange in ONE process, several HipEngines on device 0,
through the C ABI (kmer_partition, kmer_set_epochs, process, kmer_outbox, kmer_insert_device, kmer_finish_pass, kmer_epoch_counts,
kmer_end_table, kmer_histogram, faqcs_kmer_forward, faqcs_kmer_outbox_host).  No process group: items move between contexts as
device-to-device copies through a torch tensor, as parallel.KmerExchange moves them; the library's outbox memory is handed to another
context only where faqcs_kmer_forward itself does it.  At most 4 engines are alive at once.

Per-read results and counters of every submission go against the oracle first.  Then
    the sender   per submission and destination: counts[d] in occurrences (the sum of the downloaded items' k-mer fields; the items themselves
                 where an item is one k-mer, k <= 15; the pairs in direct mode), every item's bucket maps to d, the key list of
                 faqcs_kmer_outbox_host cut by the items' k-mer fields equals the model's multiset per (destination, epoch); a second
                 kmer_outbox reports nothing
    the owner    every rank the case names gets exactly the items of its destination, twice on fresh engines: on one kmer_epoch_counts is
                 read after every insert (the open group goes through the table) and again behind kmer_finish_pass, on the other only
                 behind kmer_finish_pass; kmer_histogram behind kmer_end_table.  All exact.
Whether an item went through the spill area of the sender staging cannot be read through the ABI: the spill case asserts that the
destination's multiset is complete (the predicate of the catalogue shows that no placement of the items avoids the spill).
Every result-reading call is made twice.  Settings: the default, and small_groups (FAQCS_KMER_GROUP_ITEMS=2^14) for epochs and ring."""
import ctypes as C
import time

import numpy as np
import pytest

import kmer_exchange_edges as kx
from faqcs_amd import _capi as capi
from faqcs_amd import driver

pytestmark = pytest.mark.gpu

ENGINE_ERRORS = []
SLOTS = 1 << 22
SETTINGS = {"default": {}, "small_groups": {"FAQCS_KMER_GROUP_ITEMS": str(kx.SMALL_GROUP)}}
SWITCHES = ("FAQCS_KMER_DEBUG", "FAQCS_KMER_GROUP_ITEMS", "FAQCS_KMER_FINAL", "FAQCS_KMER_DIRECT", "FAQCS_KMER_FORCE_PEER_COPY", "FAQCS_KMER_STATS")
U = np.uint64


@pytest.fixture(scope="module")
def cases():
    return kx.all_cases()


def engine(case, rank):
    from faqcs_amd.engine import HipEngine

    hip = HipEngine(case.opt(), kx.MAX_READ, kx.IN_OFF, device=0, kmer_table_slots=SLOTS)
    hip.kmer_partition(rank, case.world, case.n_epochs)
    return hip


def fetch_outbox(hip, what):
    """(counts per destination, the outbox as a torch tensor of its own: 2 int64 per item); the second call must report nothing"""
    import torch

    from faqcs_amd.parallel import _DevArray

    ptr, counts = hip.kmer_outbox()
    n = int(counts.sum())
    items = torch.empty(2 * n, dtype=torch.int64, device="cuda:0")
    if n:
        items.copy_(torch.as_tensor(_DevArray(ptr, 2 * n), device="cuda:0"))
    torch.cuda.synchronize()
    _, again = hip.kmer_outbox()
    assert not again.any(), "%s: a second kmer_outbox hands out %s again" % (what, again.tolist())
    return counts.astype(np.int64), items


def outbox_keys(hip, what):
    out = []
    for rep in range(2):
        n = C.c_uint64()
        assert hip.lib.faqcs_kmer_outbox_host(hip.ctx, None, 0, C.byref(n)) == 0, what
        keys = np.zeros(n.value + 1, U)
        assert hip.lib.faqcs_kmer_outbox_host(hip.ctx, keys.ctypes.data, n.value, C.byref(n)) == 0, what
        out.append(keys[:n.value])
    assert np.array_equal(out[0], out[1]), "%s: faqcs_kmer_outbox_host differs between two calls" % what
    return out[0]


def check_outbox(case, t, s, i, counts, items, keys):
    """the sender check of one submission"""
    what = "%s: sender %d submission %d" % (case.name, s, i)
    world, want_occ, want_keys = case.world, t.outbox_occurrences(s, i), t.outbox_keys(s, i)
    it = items.cpu().numpy().view(U).reshape(-1, 2)
    dest = np.repeat(np.arange(world), counts)
    if case.direct:  # 16-byte (key, epoch) pairs, counts in occurrences
        assert counts.tolist() == want_occ.tolist(), "%s: pairs per destination %s, the model's %s" % (what, counts.tolist(), want_occ.tolist())
        assert (it[:, 1] < U(case.n_epochs)).all(), "%s: the outbox does not hold (key, epoch) pairs" % what
        assert np.array_equal(keys, it[:, 0]), what
        key_dest, key_epoch, key = dest, it[:, 1].astype(np.int64), it[:, 0]
    else:
        w1 = it[:, 1]
        nk = ((w1 >> U(kx.NK_SHIFT)) & U((1 << kx.NK_BITS) - 1)).astype(np.int64) + 1
        part = ((w1 >> U(kx.PART_SHIFT)) & U((1 << kx.PART_BITS) - 1)).astype(np.int64)
        run = (w1 >> U(kx.RUN_SHIFT)).astype(np.int64)
        assert int(nk.sum()) == len(keys), "%s: faqcs_kmer_outbox_host lists %d keys, the items of the outbox hold %d" % (what, len(keys), int(nk.sum()))
        bad = np.nonzero((((part >> 11) * world) >> 8) != dest)[0]
        assert not len(bad), "%s: destination %d holds an item of bucket %d" % (what, dest[bad[0]] if len(bad) else -1, part[bad[0]] >> 11 if len(bad) else -1)
        got_occ = np.bincount(dest, weights=nk, minlength=world).astype(np.int64)
        print("%s: items per destination %s, occurrences %s" % (what, counts.tolist(), got_occ.tolist()))
        assert got_occ.tolist() == want_occ.tolist(), "%s: occurrences per destination %s, the model's %s" % (what, got_occ.tolist(), want_occ.tolist())
        if kx.ke.skm_geom(case.k)[1] == 1:  # an item is one k-mer: the items themselves are modelled
            assert counts.tolist() == [t.items_to(s, i, d) for d in range(world)], what
        key_dest, key_epoch, key = np.repeat(dest, nk), np.repeat(run, nk), keys
    got = sorted(set(zip(key_dest.tolist(), key_epoch.tolist())))
    assert got == sorted(want_keys), "%s: (destination, epoch) pairs %s, the model's %s" % (what, got, sorted(want_keys))
    for (d, e), want in want_keys.items():
        mine = np.sort(key[(key_dest == d) & (key_epoch == e)])
        assert np.array_equal(mine, want), "%s: destination %d epoch %d: %d keys, the model's %d; the multisets differ" % (what, d, e, len(mine), len(want))


def submit(hip, ora, sub, what):
    """one submission on a sender against the oracle; a refused one must fail with the library's message and leave the context as it was"""
    from faqcs_amd.engine import FaqcsError

    packed = driver.pack_segments(sub.buffers())
    hip.kmer_set_epochs(sub.epochs())
    if sub.error:
        with pytest.raises(FaqcsError) as e:
            hip.process(*packed)
        assert e.value.code == capi.E_INVAL and sub.error in str(e.value), "%s: %s" % (what, e.value)
        assert hip.lib.faqcs_sync(hip.ctx) == 0, what
        for rep in range(2):
            assert (hip.counters() == ora.counters()).all(), "%s: the refused submission has changed the counter block" % what
        return False
    r1, r2 = hip.process(*packed), ora.process(*packed)
    bad = np.nonzero(r1 != r2)[0]
    assert len(bad) == 0, "%s: first differing read %d: hip=%s oracle=%s" % (what, bad[0], r1[bad[0]], r2[bad[0]])
    for rep in range(2):
        assert (hip.counters() == ora.counters()).all(), "%s: the counter blocks differ" % what
    return True


def run_senders(case, t):
    """every sender's submissions -> {(s, i): (counts, items tensor)}, each checked against the oracle and the model's outbox"""
    from oracle_engine import OracleEngine

    out = {}
    for s, subs in enumerate(case.senders):
        hip, ora = engine(case, s % case.world), OracleEngine(case.opt(), kx.MAX_READ, kx.IN_OFF)
        for i, sub in enumerate(subs):
            what = "%s: sender %d submission %d" % (case.name, s, i)
            if submit(hip, ora, sub, what):
                counts, items = fetch_outbox(hip, what)
                check_outbox(case, t, s, i, counts, items, outbox_keys(hip, what))
                out[(s, i)] = (counts, items)
        hip.close()
        ora.close()
    return out


def part_of(box, key, r):
    """(device address, items) of what submission `key` holds for rank r"""
    counts, items = box[key]
    at = int(counts[:r].sum())
    return items.data_ptr() + 16 * at, int(counts[r])


def read_epochs(hip, want, what):
    for rep in range(2):
        d, t = hip.kmer_epoch_counts()
        for e in range(len(want[0])):
            assert (int(d[e]), int(t[e])) == (want[0][e], want[1][e]), "%s: epoch %d: (keys by first epoch, occurrences) = (%d, %d), the model's (%d, %d)" % (
                what, e, d[e], t[e], want[0][e], want[1][e])
    return d.tolist(), t.tolist()


def read_histogram(hip, want, what):
    for rep in range(2):
        c, n = hip.kmer_histogram()
        got = list(zip(c.tolist(), n.tolist()))
        assert got == want[2], "%s: histogram differs first at %s" % (what, next((a, b) for a, b in zip(got + [None], want[2] + [None]) if a != b))
    return got


def finish_owner(hip, want, what, before=True):
    if before:
        read_epochs(hip, want, what + ": before kmer_finish_pass")
    hip.kmer_finish_pass()
    ep = read_epochs(hip, want, what + ": behind kmer_finish_pass")
    hip.kmer_end_table()
    return ep, read_histogram(hip, want, what)


def check_owner(case, t, r, box, setting, capfd):
    """rank r on two fresh engines: asked after every insert, and asked only at the end"""
    what = "%s under %s: owner %d" % (case.name, setting, r)
    arrivals = t.arrivals(r)
    assert [k for k in t.order() if part_of(box, k, r)[1]] == [a[0] for a in arrivals], what
    results = []
    for asked in (True, False):
        capfd.readouterr()
        hip = engine(case, r)
        for step, (key, _, _) in enumerate(arrivals):
            hip.kmer_insert_device(*part_of(box, key, r))
            if asked:
                read_epochs(hip, t.owner_state(r, step + 1), "%s: behind sender %d submission %d" % (what, key[0], key[1]))
        results.append(finish_owner(hip, t.owner_state(r), what, before=asked))
        hip.close()
        err = capfd.readouterr().err
        if not asked and "flushed" in case.expect and setting == "small_groups":
            assert "through the table (a group was flushed before the pass ended)" in err, "%s: %s" % (what, err[-500:])
    assert results[0] == results[1], what


def run_plain(case, setting, capfd):
    t = case.ctx().t
    box = run_senders(case, t)
    for r in case.ranks():
        check_owner(case, t, r, box, setting, capfd)


def run_forward(case, setting, capfd, monkeypatch):
    """faqcs_kmer_forward from one sender to the owner contexts, in place or through the peer copy; then the same items by the
    kmer_outbox -> copy -> kmer_insert_device route on fresh engines"""
    from oracle_engine import OracleEngine

    if case.flow == "forward_peer":
        monkeypatch.setenv("FAQCS_KMER_FORCE_PEER_COPY", "1")
    t, lib = case.ctx().t, capi.load_library()
    owners = [engine(case, r) for r in range(case.world)]
    sender, ora, box = engine(case, 0), OracleEngine(case.opt(), kx.MAX_READ, kx.IN_OFF), {}
    right = (C.c_void_p * case.world)(*[o.ctx.value for o in owners])
    wrong = (C.c_void_p * case.world)(*[o.ctx.value for o in owners[1:] + owners[:1]])
    subs = case.senders[0]
    for i, sub in enumerate(subs):
        what = "%s: submission %d" % (case.name, i)
        assert submit(sender, ora, sub, what)
        counts, items = fetch_outbox(sender, what)
        check_outbox(case, t, 0, i, counts, items, outbox_keys(sender, what))
        box[(0, i)] = (counts, items)
        if "wrong_rank" in case.expect and i == len(subs) - 1:  # refused with nothing enqueued: the owners' results below are the model's
            assert lib.faqcs_kmer_forward(sender.ctx, wrong, case.world) == capi.E_INVAL, what
            assert b"owners[r] must be the context of rank r" in (lib.faqcs_last_error() or b""), what
        assert lib.faqcs_kmer_forward(sender.ctx, right, case.world) == 0, "%s: %s" % (what, lib.faqcs_last_error())
    for r, o in enumerate(owners):
        finish_owner(o, t.owner_state(r), "%s: owner %d behind faqcs_kmer_forward" % (case.name, r))
    for e in owners + [sender, ora]:
        e.close()
    for r in range(case.world):
        check_owner(case, t, r, box, setting, capfd)


def run_ring(case, setting, capfd):
    """four contexts, each sender and owner; submission i + 1 is enqueued on every context before the items of i are inserted"""
    from oracle_engine import OracleEngine

    t = case.ctx().t
    ctxs = [engine(case, r) for r in range(case.world)]
    oras = [OracleEngine(case.opt(), kx.MAX_READ, kx.IN_OFF) for _ in ctxs]
    box, pending = {}, []

    def insert(keys):
        for r, o in enumerate(ctxs):
            for key in keys:
                ptr, n = part_of(box, key, r)
                if n:
                    o.kmer_insert_device(ptr, n)

    for i in range(3):
        for s, hip in enumerate(ctxs):
            assert submit(hip, oras[s], case.senders[s][i], "%s: context %d submission %d" % (case.name, s, i))
        for s, hip in enumerate(ctxs):
            what = "%s: context %d submission %d" % (case.name, s, i)
            counts, items = fetch_outbox(hip, what)
            check_outbox(case, t, s, i, counts, items, outbox_keys(hip, what))
            box[(s, i)] = (counts, items)
        insert(pending)
        pending = [(s, i) for s in range(len(ctxs))]
    insert(pending)
    got = [finish_owner(o, t.owner_state(r), "%s under %s: owner %d" % (case.name, setting, r), before=False) for r, o in enumerate(ctxs)]
    for e in ctxs + oras:
        e.close()
    # the sums over the four owners, taken as points, against the oracle on the whole input in file order
    d, tot = (np.sum([g[0][j] for g in got], axis=0) for j in (0, 1))
    hist = {}
    for g in got:
        for c, n in g[1]:
            hist[c] = hist.get(c, 0) + n
    points, _, ohist = kx.oracle_whole(case)
    assert kx.points_of(case, d, tot) == points, "%s under %s: points %s, the oracle's %s" % (case.name, setting, kx.points_of(case, d, tot), points)
    assert sorted(hist.items()) == ohist, "%s under %s: the histogram summed over the owners differs from the oracle's" % (case.name, setting)


def run_cases(todo, setting, monkeypatch, capfd):
    from faqcs_amd.engine import FaqcsError

    assert not ENGINE_ERRORS, "not run: an engine call failed before (%s); nothing more is started on the device" % ENGINE_ERRORS[0]
    assert todo
    for case in todo:
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)
        monkeypatch.setenv("FAQCS_KMER_STATS", "1")
        for name, v in SETTINGS[setting].items():
            monkeypatch.setenv(name, v)
        if case.direct_env:
            monkeypatch.setenv("FAQCS_KMER_DIRECT", "1")
        t0 = time.perf_counter()
        case.ctx()
        t1 = time.perf_counter()
        try:
            if case.flow == "ring":
                run_ring(case, setting, capfd)
            elif case.flow in ("forward", "forward_peer"):
                run_forward(case, setting, capfd, monkeypatch)
            else:
                run_plain(case, setting, capfd)
        except FaqcsError as e:
            ENGINE_ERRORS.append("%s under %s: %s" % (case.name, setting, e))
            raise
        with capfd.disabled():
            print("%s under %s: model %.2f s, device and checks %.2f s" % (case.name, setting, t1 - t0, time.perf_counter() - t1))


@pytest.mark.parametrize("world", kx.WORLDS)
def test_owners(cases, world, monkeypatch, capfd):
    run_cases([c for c in cases if c.family == "owners" and c.world == world], "default", monkeypatch, capfd)


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_epochs(cases, setting, monkeypatch, capfd):
    run_cases([c for c in cases if c.family == "epochs"], setting, monkeypatch, capfd)


def test_outbox(cases, monkeypatch, capfd):
    run_cases([c for c in cases if c.family == "outbox"], "default", monkeypatch, capfd)


@pytest.mark.parametrize("flow", ["forward", "forward_peer"])
def test_forward(cases, flow, monkeypatch, capfd):
    run_cases([c for c in cases if c.family == "forward" and c.flow == flow], "default", monkeypatch, capfd)


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", ["ring_curve_completes_mid_run", "ring_no_scheduled_point"])
def test_ring(cases, name, setting, monkeypatch, capfd):
    run_cases([c for c in cases if c.name == name], setting, monkeypatch, capfd)


def test_no_case_is_left_out(cases):
    assert {c.family for c in cases} == {"owners", "epochs", "outbox", "forward", "ring"} and all(c.world in kx.WORLDS for c in cases if c.family == "owners")
    assert all(c.flow == "ring" for c in cases if c.family == "ring") and all(c.flow.startswith("forward") for c in cases if c.family == "forward")
    assert all(c.flow == "plain" for c in cases if c.family in ("owners", "epochs", "outbox"))
