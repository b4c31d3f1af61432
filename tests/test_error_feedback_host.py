"""Error feedback for 'top' — the checks that need no GPU: the C ABI surface and its argument
errors (reported before the GPU is touched), the aggregation routing of a stateful codec, and
the config defaults (include/fedcodec.h, openmsftl_amd/compression.py, aggregation.py)."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fedcodec.h")
EF_SYMBOLS = ("fc_topk_encode_ef", "fc_ef_sum", "fc_ef_clear")
FC_ERR_ARG, FC_ERR_WORKSPACE = -1, -3


@pytest.fixture(scope="module")
def lib():
    from openmsftl_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_header_declares_and_library_exports_the_entry_points(lib):
    from openmsftl_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(fc_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\s[TW]\s+(\S+)", out))
    for name in EF_SYMBOLS:
        assert name in declared, name
        assert name in exported, name
        assert name in _lib.SIGNATURES, name
    assert lib.fc_abi_version() == 4          # additions only


def _addr(buf, off=0):
    return ((ctypes.addressof(buf) + 15) & ~15) + off


def test_encode_ef_argument_errors_do_not_touch_gpu(lib):
    n, k, cap, big = 4096, 400, 8192, 1 << 30
    g, e, r = (ctypes.create_string_buffer(4 * n + 32) for _ in range(3))
    pk = ctypes.create_string_buffer(64)
    G, E, R, P = _addr(g), _addr(e), _addr(r), _addr(pk)

    def call(g_=G, e_=E, r_=R, k_=k, ws_bytes=big):
        return lib.fc_topk_encode_ef(g_, e_, r_, n, k_, P, P, cap, P, P, P, P, ws_bytes, None)

    assert call(r_=G) == FC_ERR_ARG and b"alias" in lib.fc_last_error()       # res_out is g
    assert call(r_=E) == FC_ERR_ARG and b"alias" in lib.fc_last_error()       # res_out is res_in
    assert call(r_=G + 16) == FC_ERR_ARG and b"alias" in lib.fc_last_error()  # partial overlap
    assert call(r_=R + 4) == FC_ERR_ARG and b"aligned" in lib.fc_last_error()
    assert call(e_=E + 8) == FC_ERR_ARG and b"aligned" in lib.fc_last_error()
    assert call(g_=G + 4) == FC_ERR_ARG and b"aligned" in lib.fc_last_error()
    assert call(k_=0) == FC_ERR_ARG and b"0 < k < n" in lib.fc_last_error()
    assert call(k_=n) == FC_ERR_ARG and b"0 < k < n" in lib.fc_last_error()
    assert call(e_=None) == FC_ERR_ARG and call(r_=None) == FC_ERR_ARG
    assert call(ws_bytes=16) == FC_ERR_WORKSPACE and b"workspace" in lib.fc_last_error()


def test_ef_sum_and_clear_argument_errors_do_not_touch_gpu(lib):
    from openmsftl_amd import _lib
    n = 4096
    g, e, r = (ctypes.create_string_buffer(4 * n + 32) for _ in range(3))
    G, E, R = _addr(g), _addr(e), _addr(r)
    assert lib.fc_ef_sum(G, E, G, n, None) == FC_ERR_ARG and b"alias" in lib.fc_last_error()
    assert lib.fc_ef_sum(G, E, E, n, None) == FC_ERR_ARG
    assert lib.fc_ef_sum(G, E, R + 4, n, None) == FC_ERR_ARG and b"aligned" in lib.fc_last_error()
    assert lib.fc_ef_sum(None, E, R, n, None) == FC_ERR_ARG
    assert lib.fc_ef_sum(G, E, R, 0, None) == FC_ERR_ARG
    v = _lib.PacketView(idx=0, val=G, bitmap=0, cnt=G, hdr=G, qoff=0, weight=1.0, reserved=0)
    assert lib.fc_ef_clear(ctypes.byref(v), n, R, None) == FC_ERR_ARG      # no idx: not idx/val
    assert b"incomplete" in lib.fc_last_error()
    assert lib.fc_ef_clear(None, n, R, None) == FC_ERR_ARG


def _client(cfg, n=1000):
    from openmsftl_amd import Compression
    return types.SimpleNamespace(C=Compression(cfg), grad=np.zeros(n, np.float32), client_id=0)


def test_streamed_paths_reject_an_error_feedback_client():
    from openmsftl_amd import aggregation as ag
    top = {"compression_function": "top", "fraction_coordinate": 0.1}
    plain, ef = _client(top), _client(dict(top, error_feedback=True))
    assert ag._streamable(plain.C, 1000) and not ag._streamable(ef.C, 1000)
    assert ag.common_top_fraction([plain, plain]) == 0.1
    assert ag.common_top_fraction([plain, ef]) is None
    assert ag.row_plan([plain, plain], 1000) is not None
    assert ag.row_plan([plain, ef], 1000) is None
    # 'full' keeps no state: the key changes nothing for it
    assert ag._streamable(_client({"compression_function": "full", "error_feedback": True}).C, 1000)


def test_config_defaults_are_the_reference():
    from openmsftl_amd import Compression
    ref_cfg = {"compression_function": "top", "num_bits": 2, "fraction_coordinate": 0.25,
               "dropout_p": 0.3}
    C = Compression(dict(ref_cfg))
    assert C.error_feedback is False and C.get_residual() is None
    assert (C.compression_function, C.num_bits, C.fraction_coordinates, C.dropout_p) == \
        ("top", 2, 0.25, 0.3)
    assert Compression({}).error_feedback is False
    E = Compression(dict(ref_cfg, error_feedback=True))
    assert E.error_feedback is True and E.get_residual() is None
    x = np.ones(8, np.float32)
    assert Compression({"compression_function": "full", "error_feedback": True}).compress(x) is x
    with pytest.raises(NotImplementedError):
        E.compress(x, layer_wise=True)                  # still raised first
    for fn in ("rand", "dropout-biased", "dropout-unbiased", "qsgd", "nonsense"):
        with pytest.raises(NotImplementedError):        # never a silent non-EF result
            Compression({"compression_function": fn, "error_feedback": True}).compress(x)
