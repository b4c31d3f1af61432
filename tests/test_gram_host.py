"""The packet Gram matrix and its consumers — the checks that need no GPU: the C ABI surface of
fc_packets_gram and its argument errors (reported before the GPU is touched), the workspace
size, Krum's selection on hand-made Gram matrices, the singular values from a Gram, and the
predicate of the "gram" aggregation route (include/fedcodec.h, gar.py, aggregation.py)."""
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


def test_header_declares_and_library_exports_the_entry_points(lib):
    from openmsftl_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+FC_GRAM_MAX_M\s+128\b", src)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\s[TW]\s+(\S+)", out))
    for name in ("fc_gram_workspace_bytes", "fc_packets_gram"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in exported and name in _lib.SIGNATURES, name
    assert _lib.FC_GRAM_MAX_M == 128
    assert lib.fc_abi_version() == 4          # additions only


def test_packets_gram_argument_errors_do_not_touch_gpu(lib):
    n, m, big = 3 * 8192 + 5, 7, 1 << 40
    views = ctypes.create_string_buffer(56 * m + 32)      # host buffers stand in for the device
    gram = ctypes.create_string_buffer(8 * m * m + 32)    # arrays: a call that got past the
    ws = ctypes.create_string_buffer(64)                  # checks would fault, not return a code
    V, G, W = (((ctypes.addressof(b) + 15) & ~15) for b in (views, gram, ws))

    def call(v_=V, m_=m, n_=n, g_=G, w_=W, ws_bytes=big):
        return lib.fc_packets_gram(v_, m_, n_, g_, w_, ws_bytes, None)

    assert call(v_=None) == FC_ERR_ARG and b"views_dev is NULL" in lib.fc_last_error()
    assert call(g_=None) == FC_ERR_ARG and b"gram is NULL" in lib.fc_last_error()
    assert call(w_=None) == FC_ERR_ARG and b"workspace is NULL" in lib.fc_last_error()
    assert call(m_=0) == FC_ERR_ARG and b"m=0" in lib.fc_last_error()
    assert call(m_=-1) == FC_ERR_ARG and b"m=-1" in lib.fc_last_error()
    assert call(m_=129) == FC_ERR_ARG and b"m=129" in lib.fc_last_error()
    assert call(n_=0) == FC_ERR_ARG and b"n=0" in lib.fc_last_error()
    assert call(g_=G + 8) == FC_ERR_ARG and b"gram must be 16-byte aligned" in lib.fc_last_error()
    assert call(ws_bytes=16) == FC_ERR_WORKSPACE and b"workspace" in lib.fc_last_error()
    need = lib.fc_gram_workspace_bytes(n, m)
    assert need > 0
    assert call(ws_bytes=need - 1) == FC_ERR_WORKSPACE and b"workspace" in lib.fc_last_error()


def test_gram_workspace_bytes_is_monotone_in_n_and_m(lib):
    ns = [1, 3, 2048, 8192, 8193, 6 * 8192 + 2048 + 3, 1 << 20, (1 << 24) + 1, 1 << 27, (1 << 32) - 1]
    table = [[lib.fc_gram_workspace_bytes(n, m) for m in range(1, 129)] for n in ns]
    for row in table:
        assert all(b > 0 for b in row)
        assert all(a <= b for a, b in zip(row, row[1:])), "not monotone in m"
    for lo, hi in zip(table, table[1:]):
        assert all(a <= b for a, b in zip(lo, hi)), "not monotone in n"
    # what a call cannot take has no size
    assert lib.fc_gram_workspace_bytes(0, 4) == 0
    assert lib.fc_gram_workspace_bytes(4096, 0) == 0
    assert lib.fc_gram_workspace_bytes(4096, 129) == 0
    # the bench shape stays far below a gradient's own size (4 n bytes)
    assert lib.fc_gram_workspace_bytes(1 << 27, 128) <= 32 << 20


# ---- Krum.select on hand-made Gram matrices ---------------------------------------------------
def _gram_of(points):
    p = np.asarray(points, dtype=np.float64)
    return p @ p.T


def test_krum_select_clear_winner():
    from openmsftl_amd.gar import Krum
    # four points in a cluster, client 2 at its centre, and two far away
    pts = [[1.0, 0.0], [-1.0, 0.0], [0.0, 0.0], [0.0, 1.5], [40.0, 40.0], [-30.0, 9.0]]
    g = _gram_of(pts)
    assert Krum.select(g, 0.5) == 2           # m = 3: itself and its two nearest
    scores = Krum.krum_scores(g, 0.5)
    d = np.sqrt(((np.asarray(pts)[:, None, :] - np.asarray(pts)[None, :, :]) ** 2).sum(-1))
    want = np.sort(d, axis=1)[:, :3].sum(axis=1)
    assert np.allclose(scores, want, rtol=1e-12, atol=1e-12)
    assert int(np.argmin(want)) == 2


def test_krum_select_exact_tie_takes_the_first_index():
    from openmsftl_amd.gar import Krum
    # a square: every client has the same two distances to its nearest clients
    g = _gram_of([[1.0, 1.0], [1.0, -1.0], [-1.0, -1.0], [-1.0, 1.0]])
    scores = Krum.krum_scores(g, 0.5)         # m = 2: 0 + 2
    assert np.all(scores == scores[0])
    assert Krum.select(g, 0.5) == 0


def test_krum_select_never_takes_a_nan_row():
    from openmsftl_amd.gar import Krum
    g = _gram_of([[0.0, 0.0], [5.0, 0.0], [5.0, 1.0], [9.0, 9.0]])
    g[0, :] = np.nan                          # the poisoned client would otherwise be anywhere
    g[:, 0] = np.nan
    scores = Krum.krum_scores(g, 0.5)
    assert np.isnan(scores[0]) and np.all(np.isfinite(scores[1:]))
    assert Krum.select(g, 0.5) == 1           # 1 and 2 tie (0 + 1): the first
    # the others' scores skip the NaN distance: the row sorts it last
    assert scores[1] == 1.0 and scores[2] == 1.0


def test_krum_select_all_nan_gives_the_last_index():
    from openmsftl_amd.gar import Krum
    assert Krum.select(np.full((5, 5), np.nan), 0.5) == 4


def test_krum_select_m_zero_scores_nothing_and_takes_index_zero():
    from openmsftl_amd.gar import Krum
    g = _gram_of([[3.0, 0.0], [0.0, 1.0], [7.0, 7.0]])
    assert int(0.3 * 3) == 0
    assert np.array_equal(Krum.krum_scores(g, 0.3), np.zeros(3))
    assert Krum.select(g, 0.3) == 0


def test_krum_negative_squared_distance_clamps_to_zero():
    from openmsftl_amd.gar import Krum
    g = np.array([[1.0, 1.0 + 1e-12], [1.0 + 1e-12, 1.0]])    # G_ii + G_jj - 2 G_ij < 0
    assert np.array_equal(Krum.krum_scores(g, 1.0), np.zeros(2))


def test_gram_singular_values():
    from openmsftl_amd.gar import gram_singular_values
    rng = np.random.default_rng(5)
    G = rng.standard_normal((6, 40))
    s = gram_singular_values(G @ G.T)
    assert s.dtype == np.float64 and s.shape == (6,) and np.all(np.diff(s) <= 0)
    assert np.allclose(s, np.linalg.svd(G, compute_uv=False), rtol=1e-10)
    state = np.random.get_state()
    bad = G @ G.T
    bad[2, 3] = np.nan
    assert np.all(np.isnan(gram_singular_values(bad))) and gram_singular_values(bad).shape == (6,)
    assert np.array_equal(np.random.get_state()[1], state[1])     # draws nothing


# ---- the routing predicate -----------------------------------------------------------------
TOP = {"compression_function": "top", "fraction_coordinate": 0.1}


def _client(cfg, n=1000, dtype=np.float32):
    from openmsftl_amd import Compression
    return types.SimpleNamespace(C=Compression(dict(cfg)), grad=np.zeros(n, dtype), client_id=0)


def _agg(**cfg):
    from openmsftl_amd.aggregation import Aggregator
    return Aggregator(dict({"aggregation_scheme": "fed_avg"}, **cfg))


def test_scheme_and_key_select_the_route():
    from openmsftl_amd import aggregation as ag
    from openmsftl_amd.gar import FedAvg, Krum
    krum = _agg(aggregation_scheme="krum", krum_frac=0.5)
    assert type(krum.gar) is Krum and krum.gar.krum_frac == 0.5
    assert type(_agg(aggregation_scheme="krum").gar.krum_frac) is float      # default 0.3
    assert _agg(aggregation_scheme="krum").gar.krum_frac == 0.3
    assert ag.gram_wanted(krum)
    pc = _agg(pc_analysis="gram")
    assert type(pc.gar) is FedAvg and ag.gram_wanted(pc)
    assert not ag.gram_wanted(_agg())
    assert not ag.gram_wanted(_agg(pc_analysis=True))       # keeps raising as before
    assert not ag.gram_wanted(_agg(pc_analysis=False))
    clients = [_client(TOP) for _ in range(3)]
    assert ag.gram_route_k(krum, clients) == 100
    assert ag.gram_route_k(pc, clients) == 100
    with pytest.raises(NotImplementedError, match="pc_analysis"):
        _agg(pc_analysis=True).aggregate_grads(clients)
    with pytest.raises(NotImplementedError):
        _agg(aggregation_scheme="fed_spectral_avg")


def test_each_failing_condition_raises_without_a_gpu():
    from openmsftl_amd import aggregation as ag
    top = _client(TOP)
    rounds = {
        "'top'": [top, _client({"compression_function": "full"})],
        "'top' ": [top, _client({"compression_function": "rand", "fraction_coordinate": 0.1})],
        "without error feedback": [top, _client(dict(TOP, error_feedback=True))],
        "one common fraction": [top, _client(dict(TOP, fraction_coordinate=0.2))],
        "float32 gradients": [top, _client(TOP, dtype=np.float64)],
        "one length": [top, _client(TOP, n=1001)],
        "0 < k < n": [_client(dict(TOP, fraction_coordinate=0.0)) for _ in range(2)],
        "0 < k < n ": [_client(dict(TOP, fraction_coordinate=1.0)) for _ in range(2)],
        "at most 128 clients": [top] * 129,
    }
    for scheme in ({"aggregation_scheme": "krum"}, {"pc_analysis": "gram"}):
        for why, clients in rounds.items():
            agg = _agg(**scheme)
            with pytest.raises(NotImplementedError, match=why.strip()):
                agg.aggregate_grads(clients)
            assert agg.agg_path is None and agg.agg_grad is None, why
        with pytest.raises(NotImplementedError, match="hierarchies"):
            _agg(num_hierarchies=1, cluster_size_list=[2], **scheme).aggregate_grads([top, top])
        with pytest.raises(NotImplementedError, match="one device"):
            _agg(devices=2, **scheme).aggregate_grads([top, top])
        f64w = _agg(**scheme)
        f64w.gar.gradient_weights = np.array([0.5, 0.5], np.float64)
        with pytest.raises(NotImplementedError, match="float32 GAR weights"):
            f64w.aggregate_grads([top, top])
        # the round's packets must fit the configured budget: two 1000-element clients hold
        # far more than 1000 bytes
        small = _agg(device_budget_bytes=1000, **scheme)
        with pytest.raises(NotImplementedError, match="device_budget_bytes"):
            small.aggregate_grads([top, top])
        assert ag.gram_resident_bytes(1000, 2) > 1000
    assert ag.gram_route_k(_agg(aggregation_scheme="krum"), [top] * 128) == 100
