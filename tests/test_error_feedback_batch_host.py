"""Batched error feedback for 'top' — the checks that need no GPU: the C ABI surface of
fc_topk_encode_ef_batch and its argument errors (reported before the GPU is touched), and the
predicate of the opt-in "ef-batch" aggregation route (include/fedcodec.h, aggregation.py)."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fedcodec.h")
FC_ERR_ARG, FC_ERR_WORKSPACE = -1, -3


@pytest.fixture(scope="module")
def lib():
    from openmsftl_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_header_declares_and_library_exports_the_entry_point(lib):
    from openmsftl_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bfc_topk_encode_ef_batch\s*\(", src)
    assert re.search(r"typedef\s+struct\s+fc_ef_job\s*\{[^}]*res_in[^}]*res_out[^}]*\}\s*fc_ef_job\s*;", src)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    assert "fc_topk_encode_ef_batch" in set(re.findall(r"\s[TW]\s+(\S+)", out))
    assert "fc_topk_encode_ef_batch" in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.EfJob) == 16 and ctypes.sizeof(_lib.EncodeJob) == 64
    assert lib.fc_abi_version() == 4          # additions only


def test_encode_ef_batch_argument_errors_do_not_touch_gpu(lib):
    n, k, cap, big, m = 4096, 400, 8192, 1 << 30, 3
    jobs = ctypes.create_string_buffer(64 * m + 32)       # host buffers stand in for the tables:
    efs = ctypes.create_string_buffer(16 * m + 32)        # a call that got past the checks would
    ws = ctypes.create_string_buffer(64)                  # fault, not return an error code
    J, E, W = (((ctypes.addressof(b) + 15) & ~15) for b in (jobs, efs, ws))

    def call(j_=J, e_=E, m_=m, k_=k, cap_=cap, w_=W, ws_bytes=big):
        return lib.fc_topk_encode_ef_batch(j_, e_, m_, n, k_, cap_, w_, ws_bytes, None)

    assert call(j_=None) == FC_ERR_ARG and b"NULL" in lib.fc_last_error()
    assert call(e_=None) == FC_ERR_ARG and b"NULL" in lib.fc_last_error()
    assert call(m_=0) == FC_ERR_ARG and b"m=0" in lib.fc_last_error()
    assert call(m_=65536) == FC_ERR_ARG and b"m=65536" in lib.fc_last_error()
    assert call(k_=0) == FC_ERR_ARG and b"0 < k < n" in lib.fc_last_error()
    assert call(k_=n) == FC_ERR_ARG and b"0 < k < n" in lib.fc_last_error()
    assert call(cap_=cap - 1) == FC_ERR_ARG and b"capacity" in lib.fc_last_error()
    assert call(w_=None) == FC_ERR_ARG and b"workspace" in lib.fc_last_error()
    assert call(ws_bytes=16) == FC_ERR_WORKSPACE and b"workspace" in lib.fc_last_error()
    need = lib.fc_workspace_bytes_batch(n, m)
    assert call(ws_bytes=need - 1) == FC_ERR_WORKSPACE


# ---- the routing predicate -----------------------------------------------------------------
TOP_EF = {"compression_function": "top", "fraction_coordinate": 0.1, "error_feedback": True}


def _client(cfg, n=1000, dtype=np.float32):
    from openmsftl_amd import Compression
    return types.SimpleNamespace(C=Compression(dict(cfg)), grad=np.zeros(n, dtype), client_id=0)


def _agg(**cfg):
    from openmsftl_amd.aggregation import Aggregator
    return Aggregator(dict({"aggregation_scheme": "fed_avg"}, **cfg))


def test_key_absent_an_all_ef_round_keeps_dense_fold():
    from openmsftl_amd import aggregation as ag
    clients = [_client(TOP_EF) for _ in range(3)]
    for agg in (_agg(), _agg(batched_error_feedback=False)):
        assert ag.ef_batch_k(agg, clients) is None
        # today's routing: no streamed plan, a device GAR and no hierarchies -> "dense-fold"
        assert ag.row_plan(clients, 1000) is None
        assert hasattr(agg.gar, "aggregate_packets") and agg.num_hierarchies == 0


def test_key_set_an_all_ef_round_is_batched():
    from openmsftl_amd import aggregation as ag
    clients = [_client(TOP_EF) for _ in range(3)]
    agg = _agg(batched_error_feedback=True)
    assert ag.ef_batch_k(agg, clients) == 100
    agg.gar.gradient_weights = np.array([0.5, 0.25, 0.25], np.float32)
    assert ag.ef_batch_k(agg, clients) == 100
    # the three predicates of the streamed paths still reject these clients
    assert not ag._streamable(clients[0].C, 1000)
    assert ag.common_top_fraction(clients) is None and ag.row_plan(clients, 1000) is None


def test_key_set_mixed_rounds_keep_todays_route():
    from openmsftl_amd import aggregation as ag
    agg = _agg(batched_error_feedback=True)
    ef = _client(TOP_EF)
    plain_top = _client({"compression_function": "top", "fraction_coordinate": 0.1})
    mixed = {
        "ef + plain top": [ef, plain_top],
        "ef + full": [ef, _client({"compression_function": "full"})],
        "full with the key": [ef, _client({"compression_function": "full", "error_feedback": True})],
        "two fractions": [ef, _client(dict(TOP_EF, fraction_coordinate=0.2))],
        "float64 gradient": [ef, _client(TOP_EF, dtype=np.float64)],
        "k = 0": [_client(dict(TOP_EF, fraction_coordinate=0.0)) for _ in range(2)],
        "k = n": [_client(dict(TOP_EF, fraction_coordinate=1.0)) for _ in range(2)],
        "two lengths": [ef, _client(TOP_EF, n=1001)],
    }
    for name, clients in mixed.items():
        assert ag.ef_batch_k(agg, clients) is None, name
    hier = _agg(batched_error_feedback=True, num_hierarchies=1, cluster_size_list=[2])
    assert ag.ef_batch_k(hier, [ef, ef]) is None
    f64w = _agg(batched_error_feedback=True)
    f64w.gar.gradient_weights = np.array([0.5, 0.5], np.float64)
    assert ag.ef_batch_k(f64w, [ef, ef]) is None
    multi = _agg(batched_error_feedback=True, devices=2)
    assert ag.ef_batch_k(multi, [ef, ef]) is None
    other_gar = _agg(batched_error_feedback=True)
    other_gar.gar = types.SimpleNamespace(gradient_weights=None)      # not the device FedAvg
    assert ag.ef_batch_k(other_gar, [ef, ef]) is None


def test_compression_hooks_validate_like_compress_and_advance_once():
    """_ef_buffers / _ef_commit on host tensors (no kernel runs): the validation raises
    _top_ef's ValueError and stores nothing; the commit swaps the two buffers."""
    import torch
    from openmsftl_amd import Compression
    C = Compression(dict(TOP_EF))
    cpu = torch.device("cpu")
    res, spare = C._ef_buffers(8, cpu)
    assert C.get_residual() is None                         # nothing stored yet
    assert res.dtype == torch.float32 and not res.any() and spare.numel() == 8
    spare.fill_(2.0)
    C._ef_commit(res, spare, True)
    assert C._residual is spare and C._residual_spare is res
    assert C.get_residual().tobytes() == np.full(8, 2.0, np.float32).tobytes()
    res2, spare2 = C._ef_buffers(8, cpu)
    assert res2 is spare and spare2 is res                  # the two buffers swap
    for allocate in (True, False):
        with pytest.raises(ValueError, match="reset_residual"):
            C._ef_buffers(9, cpu, allocate=allocate)
    assert C._residual is spare                             # left where it was
