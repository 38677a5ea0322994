"""CPU tests of the ray-query entry points (include/prt.h prt_query_rays / prt_query_surface): both are exported and
refuse a NULL context without a device.  What they compute is tests/test_gpu_ray_query.py's."""
from prt import _lib
import prt


def test_query_symbols_exported():
    L = prt.load()
    for name in ("prt_query_rays", "prt_query_surface"):
        assert name in _lib.EXPORTS and hasattr(L, name), name


def test_null_context_refused():
    L = prt.load()
    assert L.prt_query_rays(None, 0, None, None, None, None, None, 0) == -1 and L.prt_last_error()
    assert L.prt_query_surface(None, 0, None, None, 0, None, None, None, None, 0) == -1 and L.prt_last_error()
