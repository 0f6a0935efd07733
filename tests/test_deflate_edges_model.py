"""The catalogue of tests/deflate_edges.py without a GPU: its restated constants against csrc/faqcs_deflate.h, its coverage table (every edge
claimed, every claim of a case true, every case in a family, the unreachable edges by name and counted), the arithmetic of the pay test, and
its plain model against the host statement faqcs_deflate_host_mode on every case in both modes, byte for byte -- a difference names the case,
the member, the first differing bit and the token or header field that bit belongs to -- with every call also through
deflate_cases.assert_deflate, so that zlib, gzip and the library's own index and inflate read what the model predicted.

Restated in deflate_edges.py without a value the library shows (compared with the header's text instead, test_restated_constants): MAX_TEXT,
TILE, SUB, HASH_BITS, MIN_MATCH, MAX_MATCH, MAX_DIST, SURE_LENGTH, MATCH_BASE_BITS, the two hash multipliers; from RFC 1951 and RFC 1952: the
length and distance tables, the order of the code-length code's lengths, the fixed code, the member's header and the 28-byte EOF member."""
import os
import re

import numpy as np
import pytest

import deflate_cases as dc
import deflate_dense_cases as dd
import deflate_edges as de
import inflate_cases as ic
from faqcs_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


@pytest.fixture(scope="module")
def cases():
    return de.all_cases()


def test_restated_constants():
    src = open(os.path.join(ROOT, "faqcs_amd", "csrc", "faqcs_deflate.h")).read()
    for name, rx in de.CONSTANT_SOURCES.items():
        m = re.search(rx, src)
        assert m, "%s: csrc/faqcs_deflate.h no longer states it as %r" % (name, rx)
        assert getattr(de, name) == int(m.group(1), 0), name
    assert (de.FAST, de.DENSE) == (capi.DEFLATE_FAST, capi.DEFLATE_DENSE) == (dd.FAST, dd.DENSE)
    assert de.EOF_MEMBER == ic.EOF_MEMBER and de.GZIP_HEADER == dc.HEADER and de.MAX_TEXT == dc.MAX_TEXT
    assert re.search(r"KIND_STORED = 0, KIND_FIXED = 1, KIND_DYNAMIC = 2", src) and (de.STORED, de.FIXED, de.DYNAMIC) == (0, 1, 2)
    # the RFC's tables against its own rule: a code's range ends where the next begins
    assert all(b + (1 << e) == nb for b, e, nb in zip(de.LENGTH_BASE[:27], de.LENGTH_EXTRA[:27], de.LENGTH_BASE[1:28])) and de.LENGTH_BASE[27] + 31 == 258
    assert all(b + (1 << e) == nb for b, e, nb in zip(de.DIST_BASE, de.DIST_EXTRA, de.DIST_BASE[1:] + (32769,)))
    assert sorted(de.CL_ORDER) == list(range(19))


def test_the_pay_test_never_reaches_sure_length():
    """A literal costs 8 eighths at least, a length under 35 bytes has at most 2 extra bits, a distance at most 13: the longest match the pay
    test can refuse has 27 bytes, at a distance above 16 384 and over one-bit literals.  Every match of 28 .. 31 bytes pays, so SURE_LENGTH =
    32 never decides anything (28 would do the same)."""
    assert de.pay_bound() == (27, [16385, 24577])
    for length in range(28, de.SURE_LENGTH):
        for dist in (1, 4, 5, 1024, 16384, 16385, de.MAX_DIST):
            lits, price = de.pay(bytes(length), {0: 8}, 0, length, dist)
            assert lits > price, (length, dist)
    assert de.pay(bytes(27), {0: 8}, 0, 27, 16385) == (216, 216) and de.pay(bytes(27), {0: 8}, 0, 27, 16384) == (216, 208)
    assert max(de.LENGTH_EXTRA[de.length_symbol(l)[0]] for l in range(3, 35)) == 2 and max(de.DIST_EXTRA) == 13


def test_every_edge_is_claimed_and_every_claim_holds(cases):
    assert len({c.name for c in cases}) == len(cases), "two cases share a name"
    table, lost, more = de.coverage(cases)
    assert not lost, "claims that do not hold: %s" % lost
    missing = sorted(e for e, v in table.items() if not v and e not in de.UNREACHABLE)
    assert not missing, "edges no case reaches: %s" % missing
    assert all(c.family in de.FAMILIES for c in cases), "a case is in no family"
    assert {c.family for c in cases} == set(de.FAMILIES)
    assert len(table) >= 100 and all(e in table for c in cases for e in c.claims)


def test_unreachable_edges_by_name_and_counted(cases):
    """An edge that no input can reach stays in the table with its argument; nothing may reach it, and such edges are at most a tenth."""
    table, lost, more = de.coverage(cases)
    assert sorted(de.UNREACHABLE) == ["codes:code_length_code_of_one_symbol", "header:n_cl_below_12"]
    for e, why in de.UNREACHABLE.items():
        assert why and not table[e] and not more[e], "%s is reached by %s" % (e, table[e] + more[e])
        assert not any(e in c.claims for c in cases), e
    assert 10 * len(de.UNREACHABLE) <= len(table)
    # the smallest n_cl of the catalogue is the smallest there is
    assert min(m.st["n_cl"] for c in cases for mode in de.MODES for m in c.view(mode).members() if m.tr["kind"] == de.DYNAMIC) == 12
    # the longest token of the catalogue is the recorded one
    longest = max(de._longest(m) for c in cases for mode in de.MODES for m in c.view(mode).members())
    assert longest == de.LONGEST_TOKEN and 32 < longest <= 48


def test_the_pay_test_decides_as_its_two_sides_say(cases):
    """Every candidate under SURE_LENGTH bytes that the model put to the pay test, in every member of the catalogue: kept exactly when its
    literals cost more than the match (in the dense mode the lazy step may still take it back), and the price is 8 (12 + le + de)."""
    n = 0
    for case in cases:
        for mode in de.MODES:
            for m in case.view(mode).members():
                for p, (lits, price, (length, dist)) in m.tr["pay"].items():
                    k = m.tr["kept"][p]
                    assert 3 <= length < de.SURE_LENGTH and price == 8 * (12 + de.length_symbol(length)[1] + de.distance_symbol(dist)[1])
                    assert lits == sum(m.tr["cost"][b] for b in m.text[p:p + length])
                    assert (k == "pay") if lits <= price else (k == (length, dist) or (k == "lazy" and mode == de.DENSE)), (case.name, p)
                    n += 1
    assert n > 10000


@pytest.mark.parametrize("family", de.FAMILIES)
def test_host_statement_equals_the_model(lib, cases, family):
    n = 0
    for case in de.cases_of(family, cases):
        for mode in de.MODES:
            v = case.view(mode)
            for k, c in enumerate(v.calls):
                rc, o = dd.deflate_host_mode(lib, c["text"], case.calls[k][1], c["final"], mode=mode, capacity=c["capacity"])
                assert rc == 0
                e = c["out"]
                nb = o["info"]["n_bytes"]
                if e["info"]["overflow"]:
                    assert o["info"] == e["info"], "%s: %s" % (case.name, o["info"])
                    dc.assert_nothing_written(o)
                    continue
                nm = o["info"]["n_members"]
                bad = de.first_difference(case, k, mode, bytes(o["comp"][dc.FRONT:dc.FRONT + nb]), o["info"], o["member_offset"][:nm + 1])
                assert bad is None, bad
                dc.assert_deflate(lib, o, c["text"], case.calls[k][1], c["final"], what="%s call %d" % (case.name, k), per_member=len(c["members"]) <= 600)
                n += 1
    assert n


def test_the_reader_reads_what_the_model_wrote(cases):
    """read_stream() on the model's own members: kind, the three counts, the header tokens, the three length sets, every token with its bit
    offset and bit length, and the end of the stream"""
    for case in cases:
        if case.n_bytes() > 300000:
            continue
        for mode in de.MODES:
            for m in case.view(mode).members():
                st, tr = m.st, m.tr
                assert st["kind"] == tr["kind"], case.name
                if st["kind"] == de.STORED:
                    assert st["text"] == m.text
                    continue
                assert [t for t, _, _ in st["tokens"]] == tr["tokens"] and [(a, b) for _, a, b in st["tokens"]] == tr["where"], case.name
                assert (st["end"] + 7) // 8 == len(m.bytes) - 26 and st["end"] == tr["stream_bits"]
                if st["kind"] == de.DYNAMIC:
                    assert (st["n_lit"], st["n_dist"], st["n_cl"]) == (tr["n_lit"], tr["n_dist"], tr["n_cl"]) and st["header_tokens"] == tr["header_tokens"]
                    assert (st["lit"], st["dist"], st["cl"]) == (tr["lit"], tr["dist"], {s: l for s, l in tr["cl"].items() if de.CL_ORDER.index(s) < tr["n_cl"]})
