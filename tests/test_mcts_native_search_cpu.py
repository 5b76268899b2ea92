"""The device search's ABI without a GPU: the exports against the header and what
acme_mcts_search_create refuses before it touches the device (the refusals that need two live
networks are in tests/test_mcts_native_search_gpu.py)."""

import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_match_the_header():
    from acme_amd import _lib
    text = open(os.path.join(ROOT, "include", "acme_hip.h")).read()
    protos = re.findall(r"^int (acme_mcts_search_\w+)\(([^;]*)\);", text, re.M)
    assert {n for n, _ in protos} == {f"acme_mcts_search_{e}"
                                      for e in ("create", "destroy", "run", "debug_buffer")}
    L = _lib.lib()
    for name, args in protos:
        assert name in _lib.EXPORTED_SYMBOLS
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int32 and len(fn.argtypes) == len(args.split(",")), name
    body = re.search(r"typedef struct acme_mcts_search_config \{(.*?)\}", text, re.S).group(1)
    fields = [d.split()[-1] for d in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";")
              if d.strip()]
    assert fields == [f[0] for f in _lib.MCTSSearchConfig._fields_]  # noqa: SLF001
    for macro in ("MAX_WIDTH", "LDS_BYTES", "FIXED_BYTES", "TREE_BYTES"):
        value = int(re.search(r"#define ACME_MCTS_SEARCH_%s (\d+)" % macro, text).group(1))
        assert value == getattr(_lib, "MCTS_SEARCH_" + macro)


def test_create_rejects_bad_configurations_without_a_gpu():
    from acme_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.acme_mcts_search_create(None, ctypes.byref(h)) == _lib.ACME_ERR_INVALID
    assert "null config" in L.acme_last_error().decode()
    for kw, msg in ((dict(max_simulations=0), "max_simulations"),
                    (dict(stream_weights=2), "stream_weights"), (dict(az=None), "az must"),
                    (dict(model=None), "model must")):
        cfg = _lib.MCTSSearchConfig()
        # Never dereferenced: every case fails before the handles are read.
        cfg.az, cfg.model, cfg.max_simulations, cfg.stream_weights = 1, 1, 50, 0
        for k, v in kw.items():
            setattr(cfg, k, v)
        rc = L.acme_mcts_search_create(ctypes.byref(cfg), ctypes.byref(h))
        assert rc == _lib.ACME_ERR_INVALID and msg in L.acme_last_error().decode(), kw
    with pytest.raises(ValueError, match="max_simulations"):
        _lib.check(rc=L.acme_mcts_search_create(ctypes.byref(_lib.MCTSSearchConfig()),
                                                ctypes.byref(h)))

