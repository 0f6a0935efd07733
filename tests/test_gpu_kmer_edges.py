"""The catalogue of tests/kmer_edges.py on an MI355X: every case through HipEngine on a single device with the case's table size.  Per-read
results and counters must equal the oracle's before any k-mer is compared; then the sampling points, the totals, kmer_active() and the
whole histogram of counts are held, exactly, to the plain model of the catalogue (which tests/test_kmer_edges_model.py ties to the oracle
without a GPU).  Every engine call that reads results is made twice.  The catalogue runs under three path settings, all switches the
library reads per engine, per flush or per pass:
    one_piece     the default: a pass is counted when it ends, without the table (FAQCS_KMER_STATS must say so)
    table         FAQCS_KMER_FINAL=0: every group goes through the table
    small_groups  FAQCS_KMER_GROUP_ITEMS=2^14: groups are flushed in the middle of the pass
Cases of one option list and table size are consecutive passes on one engine (kmer_edges.engine_runs); one test per family and setting,
the failing case's name in the assertion message.  A case that is named after a path asserts the diagnostics of that path."""
import re

import numpy as np
import pytest

import kmer_edges as ke
from faqcs_amd import driver

pytestmark = pytest.mark.gpu

ENGINE_ERRORS = []
SETTINGS = {"one_piece": {}, "table": {"FAQCS_KMER_FINAL": "0"}, "small_groups": {"FAQCS_KMER_GROUP_ITEMS": str(1 << 14)}}


@pytest.fixture(scope="module")
def cases():
    return ke.all_cases()


def stats(err):
    """[(fine partitions through their table slices, inserts into the overflow area, 'in one piece'?)] of the passes FAQCS_KMER_STATS reported"""
    return [(int(a), int(b), "in one piece" in line) for line in err.splitlines() if line.startswith("[kmer stats]")
            for a, b in re.findall(r"; (\d+) of \d+ fine partitions through their table slices; (\d+) inserts", line)]


def points_of(engine):
    return [tuple(int(x) for x in p) for p in engine.kmer_points()]


def run_engine(run, setting, monkeypatch, capfd):
    """The cases of `run` as consecutive passes on one HipEngine, an oracle engine and a model engine side by side"""
    from oracle_engine import OracleEngine

    from faqcs_amd.engine import HipEngine

    monkeypatch.setenv("FAQCS_KMER_STATS", "1")
    for name in ("FAQCS_KMER_DEBUG", "FAQCS_KMER_GROUP_ITEMS", "FAQCS_KMER_FINAL"):
        monkeypatch.delenv(name, raising=False)
    for name, v in [kv for c in run for kv in c.env.items()] + list(SETTINGS[setting].items()):  # (the setting's value holds where both name a switch)
        monkeypatch.setenv(name, v)
    opt = run[0].opt()
    hip, ora, m = HipEngine(opt, ke.MAX_READ, ke.IN_OFF, device=0, kmer_table_slots=run[0].slots), OracleEngine(opt, ke.MAX_READ, ke.IN_OFF), ke.Model(opt)
    for case in run:
        what = "%s under %s" % (case.name, setting)
        assert m.active, what
        capfd.readouterr()
        for sub in case.subs:
            packed = driver.pack_segments(sub)
            r1, r2 = hip.process(*packed), ora.process(*packed)
            bad = np.nonzero(r1 != r2)[0]
            assert len(bad) == 0, "%s: first differing read %d: hip=%s oracle=%s" % (what, bad[0], r1[bad[0]], r2[bad[0]])
            assert (hip.counters() == ora.counters()).all(), "%s: the counter blocks differ" % what
            m.submit(sub, r2)
            for rep in range(2):
                assert hip.kmer_active() == m.active, what
                if case.ask:
                    assert points_of(hip) == m.points and hip.kmer_totals() == m.totals(), what
        hip.kmer_end_table()
        m.end_table()
        for rep in range(2):
            assert points_of(hip) == m.points, "%s: points %s, the model's %s" % (what, points_of(hip), m.points)
            assert hip.kmer_totals() == m.last_totals, "%s: totals %s, the model's %s" % (what, hip.kmer_totals(), m.last_totals)
            assert hip.kmer_active() == m.active, what
            c, n = hip.kmer_histogram()
            got, want = list(zip(c.tolist(), n.tolist())), m.histogram()
            assert got == want, "%s: histogram differs first at %s" % (what, next((a, b) for a, b in zip(got + [None], want + [None]) if a != b))
        err = capfd.readouterr().err
        st = stats(err)
        with capfd.disabled():
            print("%s: (redo, overflow inserts, in one piece) %s" % (what, st))
        assert len(st) == 1, "%s: %s" % (what, err[-2000:])
        redo, overflow, one_piece = st[0]
        n_bytes = sum(len(r[1]) for sub in case.subs for seg in sub for r in seg)
        if setting == "one_piece":
            assert one_piece == (not case.ask and "flushed" not in case.expect), what
            assert redo >= 1 or "redo" not in case.expect, what
        if setting == "table" or "flushed" in case.expect or (setting == "small_groups" and n_bytes > 8 << 14):
            assert not one_piece, what
        if "overflow" in case.expect:
            assert overflow > 0, what
        if "fullest" in case.expect:
            fullest = [int(x) for x in re.findall(r"fullest partition (\d+) keys", err)]
            assert fullest and (max(fullest) > ke.LDS_SLOTS or setting == "small_groups"), "%s: %s" % (what, fullest)
    hip.close()
    ora.close()


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("family", ke.FAMILIES)
def test_catalogue(cases, family, setting, monkeypatch, capfd):
    from faqcs_amd.engine import FaqcsError

    assert not ENGINE_ERRORS, "not run: an engine call failed before (%s); nothing more is started on the device" % ENGINE_ERRORS[0]
    runs = ke.engine_runs(cases, family)
    assert runs
    for run in runs:
        try:
            run_engine(run, setting, monkeypatch, capfd)
        except FaqcsError as e:
            ENGINE_ERRORS.append("%s under %s: %s" % (run[0].name, setting, e))
            raise


def test_no_case_is_left_out(cases):
    assert sorted({c.name for f in ke.FAMILIES for r in ke.engine_runs(cases, f) for c in r}) == sorted(c.name for c in cases)
