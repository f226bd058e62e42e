"""The k-clique trusses' entry points without a device: gm_clique_ktruss and gm_clique_truss_decompose exist in the library, refuse what needs
no handle to refuse, and the Python names are exported."""
import ctypes as C


def test_entry_points_refuse_without_a_handle():
    from graphminer_amd import _lib

    lib = _lib.load()
    n, m, rounds, cmax = C.c_uint64(7), C.c_uint64(7), C.c_int32(7), C.c_uint64(7)
    somewhere = C.c_void_p(64)  # (never dereferenced: every call below is refused before it looks at a handle or an array)
    for k in (3, 2, 13):
        rc = lib.gm_clique_ktruss(None, k, 1, None, None, C.byref(n), C.byref(m), C.byref(rounds), None)
        print(f"gm_clique_ktruss(NULL, k = {k}) -> {rc}", flush=True)
        assert rc == _lib.GM_ERR_INVALID
        rc = lib.gm_clique_truss_decompose(None, k, None, somewhere, None, C.byref(cmax), C.byref(rounds), None)
        print(f"gm_clique_truss_decompose(NULL, k = {k}) -> {rc}", flush=True)
        assert rc == _lib.GM_ERR_INVALID
    rc = lib.gm_clique_truss_decompose(None, 3, None, None, None, C.byref(cmax), C.byref(rounds), None)
    print(f"gm_clique_truss_decompose(no theta array) -> {rc}", flush=True)
    assert rc == _lib.GM_ERR_INVALID


def test_python_names():
    import graphminer_amd as gm

    for name in ("clique_ktruss", "clique_truss_decompose"):
        assert callable(getattr(gm, name)) and name in gm.__all__, name
