"""The BGZF index without a GPU: the catalogue of bgzf_index_cases.py -- its plain-Python restatement of the walk -- against the host
statement faqcs_bgzf_index_host in every field, every offset and the canaries; the coverage table; and the exports and bindings of the
device form, which the GPU test (test_gpu_bgzf_index.py) compares with the same host statement."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import bgzf_index_cases as bc
from faqcs_amd import _capi as capi


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def test_restatement_equals_the_host_statement_on_every_case(lib):
    """info, member_offset[0 .. n_members] and the untouched entries and canaries around them; and every edge a case names that the walk
    or the impostor search can observe is observed in it."""
    for c in bc.cases():
        info, offs, seen = bc.walk(c.comp, c.final, c.capacity)
        rc, h, off = bc.index_host(lib, c.comp, c.final, c.capacity)
        assert rc == 0, c.name
        assert h == dict(info, reserved=0), c.name
        assert (off == bc.expected_offsets(offs, c.capacity)).all(), c.name
        assert c.edges & bc.WALK_EDGES <= seen, (c.name, sorted(c.edges & bc.WALK_EDGES - seen))
        if c.edges & bc.IMPOSTOR_EDGES or any(e.startswith("impostor in") for e in c.edges):
            found, kinds = bc.impostors(c.comp)
            assert found and c.edges & bc.IMPOSTOR_EDGES <= kinds, (c.name, kinds)


def test_constructed_facts():
    """what the catalogue says about its own shapes: the capacities, the dense chain's size, the tile-boundary starts, the residue case"""
    by_edge = {}
    for c in bc.cases():
        for e in c.edges:
            by_edge.setdefault(e, []).append(c)
    for c in by_edge["header at tile boundary"]:
        offs = bc.walk(c.comp, 1, 1 << 30)[1]
        assert any(o % bc.TILE in range(bc.TILE - 18, bc.TILE) or (o % bc.TILE == 0 and o) for o in offs), c.name
    starts = sorted({o % bc.TILE for c in by_edge["header at tile boundary"] for o in bc.walk(c.comp, 1, 1 << 30)[1] if o and (o % bc.TILE == 0 or o % bc.TILE >= bc.TILE - 18)})
    assert starts == [0] + list(range(bc.TILE - 18, bc.TILE))
    for e, d in (("capacity=n-1", -1), ("capacity=n", 0), ("capacity=n+1", 1)):
        for c in by_edge[e]:
            assert c.capacity == bc.walk(c.comp, c.final, 1 << 30)[0]["n_members"] + d, c.name
    assert all(c.capacity == 0 for c in by_edge["capacity=0"]) and all(len(c.comp) == 0 for c in by_edge["n_comp=0"])
    assert any(len(c.comp) == bc.DENSE_MEMBERS * 28 > (bc.SCAN_TILES + 1) * bc.TILE for c in by_edge["dense chain"])
    assert any(65536 in np.diff(bc.walk(c.comp, 1, 1 << 30)[1]) for c in by_edge["member of 65536"])
    for c in by_edge["bc in next tile"]:
        offs = bc.walk(c.comp, 1, 1 << 30)[1]
        assert any(a // bc.TILE != (a + 12 + int.from_bytes(c.comp[a + 10:a + 12], "little") - 6) // bc.TILE for a in offs[:-1]), c.name
    for tag, follows in (("impostor at last 18, data ends", False), ("impostor at last 18, member follows", True)):
        assert len(by_edge[tag]) == 18
        for j, c in enumerate(by_edge[tag], 1):
            end = bc.walk(c.comp, 1, 1 << 30)[1][4 if follows else -1]  # the end of the member that holds the pattern
            assert c.comp[end - j:end] == bc.header(64)[:j] and (end == len(c.comp)) != follows, c.name
    r = bc.residue_case()
    assert bc.walk(r, 0, 64)[0] == {"consumed": len(r) - 13, "n_members": 43, "overflow": 0, "error": 0} and bc.impostors(r)[0]


def test_the_coverage_table_is_complete():
    reached = set().union(*(c.edges for c in bc.cases()))
    assert sorted(set(bc.EDGES) - reached) == []
    assert bc.WALK_EDGES | bc.IMPOSTOR_EDGES <= set(bc.EDGES)


def test_random_inputs_agree_and_are_never_refused(lib):
    """the generator of the GPU test's randomised round: the restatement and the host statement agree on what it draws, and the host
    refuses none of it"""
    rng = np.random.Generator(np.random.PCG64([211, bc.MIN_MEMBER]))
    kinds = set()
    for k in range(300):
        comp, final, cap = bc.random_input(rng)
        info, offs, _ = bc.walk(comp, final, cap)
        rc, h, off = bc.index_host(lib, comp, final, cap)
        assert rc == 0 and h == dict(info, reserved=0) and (off == bc.expected_offsets(offs, cap)).all(), k
        kinds.add((info["error"], info["overflow"], info["consumed"] == len(comp)))
    assert len(kinds) >= 6, kinds


def test_exports_and_bindings(lib):
    """the library exports the device form and its timer, the header declares them and capi binds them"""
    names = {"faqcs_bgzf_index_device", "faqcs_bgzf_index_time_ms"}
    fresh = C.CDLL(capi.lib_path())  # (a symbol the library does not export raises AttributeError)
    for nm in names:
        assert getattr(fresh, nm) is not None
    assert names <= set(capi.declared_symbols()) and names <= set(lib._faqcs_symbols)
    assert lib.faqcs_bgzf_index_device.argtypes[3] is C.c_int and len(lib.faqcs_bgzf_index_device.argtypes) == 7
    from faqcs_amd import device, engine

    assert callable(engine.HipEngine.bgzf_index_device) and callable(engine.HipEngine.bgzf_index_time_ms) and callable(device.bgzf_index)
    assert inspect.signature(device.inflated_text).parameters["index"].default == "host"
    src = os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "csrc", "faqcs_bgzf_index_kernel.hip")
    assert os.path.exists(src)


def test_null_context_is_refused(lib):
    ii = capi.BgzfIndexInfo()
    off = np.zeros(4, np.uint32)
    assert lib.faqcs_bgzf_index_device(None, None, 0, 1, off.ctypes.data, 3, C.addressof(ii)) == capi.E_INVAL
    a = C.c_double()
    assert lib.faqcs_bgzf_index_time_ms(None, C.byref(a), C.byref(a)) == capi.E_INVAL
