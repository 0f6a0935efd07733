"""CPU-side limits of the adapter / contaminant library (no device needed): the counter layout of the C library takes up to 65 534
targets -- faqcs_read_result.adapter holds 1 + index in 16 bits, 0xffff marks a bad base -- agrees there with the python statement,
and refuses one more."""
import ctypes as C

import pytest

from faqcs_amd import _capi as capi


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    return capi.load_library()


@pytest.mark.parametrize("R,na", [(150, 65), (256, 200), (1024, 1000), (32767, 65534)])
def test_layout_of_large_libraries_equals_python(lib, R, na):
    lay = capi.Layout()
    assert lib.faqcs_counters_layout(R, na, C.byref(lay)) == 0
    py = capi.python_layout(R, na)
    assert int(lay.n_adapters) == na
    assert (int(lay.adapter_stats), int(lay.total)) == (py["adapter_stats"][0], py["total"])


def test_layout_refuses_more_than_65534_targets(lib):
    lay = capi.Layout()
    assert lib.faqcs_counters_layout(150, 65535, C.byref(lay)) == capi.E_INVAL
