"""The triangle nuclei's entry points without a device: gm_tri_clique4_local, gm_nucleus34 and gm_nucleus34_decompose exist in the library,
refuse what needs no handle to refuse, and the Python names are exported."""
import ctypes as C


def test_entry_points_refuse_without_a_handle():
    from graphminer_amd import _lib

    lib = _lib.load()
    n, m, rounds, cmax = C.c_uint64(7), C.c_uint64(7), C.c_int32(7), C.c_uint32(7)
    somewhere = C.c_void_p(64)  # (never dereferenced: every call below is refused before it looks at a handle or an array)
    rc = lib.gm_tri_clique4_local(None, None, 0, None, C.byref(n), None)
    print(f"gm_tri_clique4_local(NULL) -> {rc}", flush=True)
    assert rc == _lib.GM_ERR_INVALID
    rc = lib.gm_nucleus34(None, 1, None, 0, None, C.byref(n), C.byref(m), C.byref(rounds), None)
    print(f"gm_nucleus34(NULL) -> {rc}", flush=True)
    assert rc == _lib.GM_ERR_INVALID
    rc = lib.gm_nucleus34_decompose(None, None, 0, somewhere, None, C.byref(cmax), C.byref(rounds), None)
    print(f"gm_nucleus34_decompose(NULL) -> {rc}", flush=True)
    assert rc == _lib.GM_ERR_INVALID
    rc = lib.gm_nucleus34_decompose(None, None, 0, None, None, C.byref(cmax), C.byref(rounds), None)
    print(f"gm_nucleus34_decompose(no theta array) -> {rc}", flush=True)
    assert rc == _lib.GM_ERR_INVALID


def test_python_names():
    import graphminer_amd as gm

    for name in ("tri_clique4_local", "nucleus34", "nucleus34_decompose"):
        assert callable(getattr(gm, name)) and name in gm.__all__, name


def test_constant():
    from common import gm_constant

    assert gm_constant("nuc_whole_wave") == 64
    assert gm_constant("nuc_group") == 8
