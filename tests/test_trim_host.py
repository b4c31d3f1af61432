"""The coordinate-wise rules (trimmed mean, median) — the checks that need no GPU: the definition
in tests/trim_model.py against NumPy's own median and sorted mean and on hand-written columns,
the config handling of gar.TrimmedMean / gar.CoordinateMedian, the routing of the two schemes
(aggregation.py) and the C ABI surface of fc_packets_trim with its argument errors, which are
reported before the GPU is touched (include/fedcodec.h).
"""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import trim_model as tm
from oracle import packet_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fedcodec.h")
FC_ERR_ARG, FC_ERR_WORKSPACE = -1, -3
F = np.float32
NAN, INF = F(np.nan), F(np.inf)
NEG0 = F(-0.0)


def sparse_matrix(M, N, frac, seed):
    """Random normal values at a fraction of the cells, +0.0 elsewhere; no NaN, no -0.0."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((M, N)).astype(F)
    G[rng.random((M, N)) >= frac] = F(0.0)
    return G


# ---- the model ------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 7, 8])
def test_model_median_equals_numpy_median(M):
    for frac in (0.1, 0.6, 1.0):
        G = sparse_matrix(M, 4000, frac, seed=100 + M)
        got = tm.trimmed_mean_model(G, tm.median_trim(M))
        want = np.median(G, axis=0)
        assert want.dtype == np.float32
        assert po.same_bits(got, want), (M, frac)


@pytest.mark.parametrize("M,b", [(9, 2), (8, 0), (16, 1), (5, 2)])
def test_model_equals_numpy_sorted_mean_on_non_degenerate_columns(M, b):
    for frac in (0.1, 0.6, 1.0):
        G = sparse_matrix(M, 4000, frac, seed=200 + M)
        got = tm.trimmed_mean_model(G, b)
        want = np.mean(np.sort(G, axis=0)[b:M - b], axis=0)
        assert want.dtype == np.float32
        assert po.same_bits(got, want), (M, b, frac)


def test_model_zero_signs_and_non_finite_columns_by_hand():
    def one(col, b):
        return tm.trimmed_mean_model(np.array(col, dtype=F).reshape(-1, 1), b)[0]

    def bits(x):
        return int(np.array(x, F).view(np.uint32))

    # the sum starts from +0.0: zeros of either sign give +0.0, never -0.0
    assert bits(one([NEG0, NEG0, NEG0], 0)) == 0
    assert bits(one([NEG0, NEG0, NEG0], 1)) == 0
    assert bits(one([NEG0, 0.0, NEG0, 0.0], 1)) == 0
    assert bits(one([-1.0, NEG0, 1.0], 1)) == 0
    # plain cases: (2 + 3 + 4) / 3 after trimming 1 and 5
    assert one([5.0, 1.0, 3.0, 2.0, 4.0], 1) == F(3.0)
    assert one([5.0, 1.0, 3.0, 2.0, 4.0], 2) == F(3.0)
    assert one([1.0, 2.0], 0) == F(1.5)
    # ascending order of the adds: (-(2^25) + 1) + 2^25 = 0 in float32, not 1
    big = F(2.0 ** 25)
    assert one([big, 1.0, -big], 0) == F(0.0)
    # a NaN is trimmed like a largest value
    assert one([NAN, 1.0, 2.0, 3.0, 0.0], 1) == F(2.0)            # drops 0 and NaN
    assert np.isnan(one([NAN, NAN, 2.0, 3.0, 0.0], 1))            # b + 1 NaNs
    assert one([NAN, NAN, 2.0, 3.0, 0.0], 2) == F(3.0)
    assert np.isnan(one([NAN], 0))
    # infinities survive or are trimmed by rank
    assert one([INF, -INF, 1.0, 2.0, 3.0], 1) == F(2.0)
    assert np.isnan(one([INF, -INF, 1.0, 2.0, 3.0], 0))           # both survive: inf - inf
    assert one([INF, INF, 1.0, 2.0, 3.0], 1) == INF
    assert one([-INF, -INF, 1.0, 2.0, 3.0], 1) == -INF
    assert one([INF, NAN, 1.0, 2.0, -INF], 1) == INF              # NaN and -inf trimmed, +inf stays
    # denormals add exactly
    d = F(1e-45)
    assert one([d, d, 0.0, 0.0], 0) == F(2e-45) / F(4.0)
    with pytest.raises(ValueError):
        tm.trimmed_mean_model(np.zeros((4, 3), F), 2)
    with pytest.raises(ValueError):
        tm.trimmed_mean_model(np.zeros((4, 3), F), -1)


# ---- gar.TrimmedMean / gar.CoordinateMedian ---------------------------------------------------
class _FakeCodec:
    """Stands in for codec while CoordinateTrim.aggregate_packets runs on the host."""

    def __init__(self):
        self.calls = []

    def trimmed_mean(self, packets, trim, out=None):
        self.calls.append((len(packets), trim, out))
        return "agg"


def test_trim_count_from_the_config(monkeypatch):
    from openmsftl_amd import gar
    fake = _FakeCodec()
    monkeypatch.setattr(gar, "codec", fake)
    r = gar.TrimmedMean({})
    assert r.trim is None and r.trim_frac == 0.1 and r.trim_count is None
    assert r.aggregate_packets([0] * 128) == "agg" and r.trim == 12
    assert r.aggregate_packets([0] * 9) == "agg" and r.trim == 0
    r = gar.TrimmedMean({"trim_frac": 0.25})
    r.aggregate_packets([0] * 9)
    assert r.trim == 2 == int(0.25 * 9)
    r = gar.TrimmedMean({"trim_count": 3})
    r.aggregate_packets([0] * 7, out="o")
    assert r.trim == 3 and fake.calls[-1] == (7, 3, "o")
    r = gar.TrimmedMean({"trim_count": np.int64(0)})
    r.aggregate_packets([0])
    assert r.trim == 0
    med = gar.CoordinateMedian({})
    for m, b in ((1, 0), (2, 0), (3, 1), (8, 3), (9, 4), (128, 63)):
        med.aggregate_packets([0] * m)
        assert med.trim == b and fake.calls[-1][:2] == (m, b)
    for rule in (gar.TrimmedMean({}), med):
        assert isinstance(rule, gar.CoordinateTrim) and isinstance(rule, gar.GAR)
        with pytest.raises(NotImplementedError, match="aggregate_packets"):
            rule.aggregate(np.zeros((3, 8), F))


def test_trim_config_errors_name_the_key(monkeypatch):
    from openmsftl_amd import gar
    monkeypatch.setattr(gar, "codec", _FakeCodec())
    with pytest.raises(ValueError, match="trim_frac.*trim_count|trim_count.*trim_frac"):
        gar.TrimmedMean({"trim_frac": 0.1, "trim_count": 1})
    for bad in (-0.1, float("nan"), "a", True):
        with pytest.raises(ValueError, match="trim_frac"):
            gar.TrimmedMean({"trim_frac": bad})
    for bad in (-1, 1.5, True, "2"):
        with pytest.raises(ValueError, match="trim_count"):
            gar.TrimmedMean({"trim_count": bad})
    with pytest.raises(ValueError, match="trim_frac"):
        gar.TrimmedMean({"trim_frac": 0.5}).aggregate_packets([0] * 8)       # 2 * 4 >= 8
    with pytest.raises(ValueError, match="trim_count"):
        gar.TrimmedMean({"trim_count": 2}).aggregate_packets([0] * 4)
    with pytest.raises(ValueError, match="trim_count"):
        gar.TrimmedMean({"trim_count": 1}).aggregate_packets([0])


def test_weights_are_refused(monkeypatch):
    from openmsftl_amd import gar
    fake = _FakeCodec()
    monkeypatch.setattr(gar, "codec", fake)
    for rule in (gar.TrimmedMean({}), gar.CoordinateMedian({})):
        rule.gradient_weights = np.full(4, 0.25, F)
        with pytest.raises(ValueError, match="gradient_weights"):
            rule.aggregate_packets([0] * 4)
    assert fake.calls == []


def test_codec_trim_checks_need_no_gpu():
    from openmsftl_amd import codec
    with pytest.raises(ValueError, match="no packets"):
        codec.trimmed_mean([], 0)
    assert codec._check_trim(9, 4) == 4 and codec._check_trim(1, 0) == 0
    assert codec._check_trim(128, np.int32(63)) == 63
    for m, b in ((8, 4), (1, 1), (9, 5)):
        with pytest.raises(ValueError, match="2 \\* trim"):
            codec._check_trim(m, b)
    with pytest.raises(ValueError, match="negative"):
        codec._check_trim(8, -1)
    with pytest.raises(ValueError, match="at most 128"):
        codec._check_trim(129, 0)
    with pytest.raises(ValueError, match="integer"):
        codec._check_trim(8, 1.0)


# ---- routing ---------------------------------------------------------------------------------
TOP = {"compression_function": "top", "fraction_coordinate": 0.1}
SCHEMES = [{"aggregation_scheme": "trimmed_mean"},
           {"aggregation_scheme": "trimmed_mean", "trim_count": 1},
           {"aggregation_scheme": "coordinate_median"}]


def _client(cfg, n=1000, dtype=np.float32):
    from openmsftl_amd import Compression
    return types.SimpleNamespace(C=Compression(dict(cfg)), grad=np.zeros(n, dtype), client_id=0)


def _agg(**cfg):
    from openmsftl_amd.aggregation import Aggregator
    return Aggregator(dict({"aggregation_scheme": "fed_avg"}, **cfg))


def test_the_two_schemes_select_the_route():
    from openmsftl_amd import aggregation as ag
    from openmsftl_amd.gar import CoordinateMedian, CoordinateTrim, TrimmedMean
    clients = [_client(TOP) for _ in range(3)]
    for scheme, kind in zip(SCHEMES, (TrimmedMean, TrimmedMean, CoordinateMedian)):
        a = _agg(**scheme)
        assert type(a.gar) is kind and isinstance(a.gar, CoordinateTrim)
        assert ag.gram_wanted(a) and ag.gram_route_k(a, clients) == 100
        assert a.agg_path is None
    assert _agg(aggregation_scheme="trimmed_mean", trim_frac=0.2).gar.trim_frac == 0.2
    with pytest.raises(ValueError, match="trim_count"):
        _agg(aggregation_scheme="trimmed_mean", trim_count=-2)


def test_a_round_outside_the_route_raises_without_a_gpu():
    top = _client(TOP)
    rounds = {
        "'top'": [top, _client({"compression_function": "full"})],
        "without error feedback": [top, _client(dict(TOP, error_feedback=True))],
        "one common fraction": [top, _client(dict(TOP, fraction_coordinate=0.2))],
        "float32 gradients": [top, _client(TOP, dtype=np.float64)],
        "one length": [top, _client(TOP, n=1001)],
        "0 < k < n": [_client(dict(TOP, fraction_coordinate=0.0)) for _ in range(2)],
        "at most 128 clients": [top] * 129,
    }
    for scheme in SCHEMES:
        for why, clients in rounds.items():
            agg = _agg(**scheme)
            with pytest.raises(NotImplementedError, match=why):
                agg.aggregate_grads(clients)
            assert agg.agg_path is None and agg.agg_grad is None, why
        with pytest.raises(NotImplementedError, match="hierarchies"):
            _agg(num_hierarchies=1, cluster_size_list=[2], **scheme).aggregate_grads([top, top])
        with pytest.raises(NotImplementedError, match="one device"):
            _agg(devices=2, **scheme).aggregate_grads([top, top])
        small = _agg(device_budget_bytes=1000, **scheme)
        with pytest.raises(NotImplementedError, match="device_budget_bytes"):
            small.aggregate_grads([top, top])
        weighted = _agg(**scheme)
        weighted.gar.gradient_weights = np.array([0.5, 0.5], np.float32)
        with pytest.raises(ValueError, match="gradient_weights"):
            weighted.aggregate_grads([top, top])
        assert weighted.agg_path is None and weighted.agg_grad is None
        with pytest.raises(ValueError, match="gradient_weights"):
            weighted.aggregate_wire([b""])


@pytest.fixture(scope="module")
def lib():
    from openmsftl_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_gram_resident_bytes_is_unchanged_for_the_existing_schemes(lib):
    """The formula as it stood before the two schemes, restated here."""
    from openmsftl_amd import aggregation as ag
    from openmsftl_amd.pipeline import packet_bytes
    for n, m in ((1000, 2), (3 * 8192 + 37, 16), (1 << 24, 128)):
        want = (m * (4 * n + packet_bytes(n)) + int(lib.fc_workspace_bytes_batch(n, m))
                + int(lib.fc_gram_workspace_bytes(n, m)) + int(lib.fc_dot_workspace_bytes(n, m))
                + 4 * n + 4 * n + 8 * m * m)
        assert ag.gram_resident_bytes(n, m) == want
        for cfg in ({"aggregation_scheme": "fed_avg"}, {"aggregation_scheme": "krum"},
                    {"aggregation_scheme": "geometric_median"},
                    {"aggregation_scheme": "centered_clip", "cclip_tau": 1.0},
                    {"aggregation_scheme": "spectral_gram", "adaptive_rank_th": 0.95}):
            assert ag.gram_resident_bytes(n, m, _agg(**cfg).gar) == want, cfg
        for scheme in SCHEMES:
            assert ag.gram_resident_bytes(n, m, _agg(**scheme).gar) \
                == want + int(lib.fc_trim_workspace_bytes(n, m))


# ---- ABI -------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points(lib):
    from openmsftl_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\s[TW]\s+(\S+)", out))
    for name in ("fc_trim_workspace_bytes", "fc_packets_trim"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in exported and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    assert lib.fc_abi_version() == 4          # additions only


def test_packets_trim_argument_errors_do_not_touch_gpu(lib):
    n, m = 3 * 8192 + 5, 7
    views = ctypes.create_string_buffer(56 * m + 32)      # host buffers stand in for the device
    out = ctypes.create_string_buffer(64)                 # arrays: a call that got past the
    ws = ctypes.create_string_buffer(64)                  # checks would fault, not return a code
    V, O, W = (((ctypes.addressof(b) + 15) & ~15) for b in (views, out, ws))

    def call(v_=V, m_=m, n_=n, b_=1, o_=O, w_=W, ws_bytes=0):
        return lib.fc_packets_trim(v_, m_, n_, b_, o_, w_, ws_bytes, None)

    err = lib.fc_last_error
    assert call(v_=None) == FC_ERR_ARG and b"views_dev is NULL" in err()
    assert call(o_=None) == FC_ERR_ARG and b"out is NULL" in err()
    assert call(m_=0) == FC_ERR_ARG and b"m=0" in err()
    assert call(m_=-1) == FC_ERR_ARG and b"m=-1" in err()
    assert call(m_=129, b_=0) == FC_ERR_ARG and b"m=129" in err()
    assert call(b_=-1) == FC_ERR_ARG and b"trim=-1" in err()
    assert call(b_=4) == FC_ERR_ARG and b"trim=4" in err()              # 2 * 4 >= 7
    assert call(m_=8, b_=4) == FC_ERR_ARG and b"trim=4" in err()        # 2 * 4 >= 8
    assert call(m_=1, b_=1) == FC_ERR_ARG and b"trim=1" in err()
    assert call(b_=(1 << 31) - 1) == FC_ERR_ARG and b"trim=" in err()   # 2 * trim does not wrap
    assert call(n_=0) == FC_ERR_ARG and b"n=0" in err()
    assert call(n_=1 << 32) == FC_ERR_ARG and b"outside [1, 2^32-1]" in err()
    assert call(o_=O + 8) == FC_ERR_ARG and b"out must be 16-byte aligned" in err()
    assert call(w_=W + 8, ws_bytes=64) == FC_ERR_ARG and b"workspace must be 16-byte aligned" in err()
    need = lib.fc_trim_workspace_bytes(n, m)
    if need:
        assert call(w_=None) == FC_ERR_ARG and b"workspace is NULL" in err()
        assert call(ws_bytes=need - 1) == FC_ERR_WORKSPACE and b"workspace" in err()


def test_trim_workspace_bytes_is_small_and_monotone(lib):
    ns = [1, 8192, 8193, 1 << 20, (1 << 24) + 1, 1 << 27, (1 << 32) - 1]
    table = [[lib.fc_trim_workspace_bytes(n, m) for m in range(1, 129)] for n in ns]
    for row in table:
        assert all(a <= b for a, b in zip(row, row[1:])), "not monotone in m"
    for lo, hi in zip(table, table[1:]):
        assert all(a <= b for a, b in zip(lo, hi)), "not monotone in n"
    assert lib.fc_trim_workspace_bytes(1 << 27, 128) <= 4 << 20      # far below a gradient (4 n)
