"""The coordinate-wise rules over scaled-sign packets — the checks that need no GPU: the rank-order
walk (tests/sign_trim_model.py) against the sorted definition, the C ABI of fc_sign_trim and its
argument errors (reported before the GPU is touched), codec.trimmed_mean_sign's own checks, the
dispatch of gar.CoordinateTrim.aggregate_packets by packet kind and the Aggregator's "sign_trim"
routing on stub clients.

Run:  python -m pytest tests/test_sign_trim_host.py -m "not gpu" -q
"""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import sign_geometry_model as gm
import sign_model as sm
import sign_trim_model as stm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fedcodec.h")
FC_ERR_ARG, FC_ERR_WORKSPACE = -1, -3
F = np.float32
NEW = ("fc_sign_trim_workspace_bytes", "fc_sign_trim")


def same_bits(got, want, what=""):
    """Bit for bit; NaN positions compare as NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == F, what
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.argwhere((gn != wn) | (~gn & ~wn & (got.view(np.uint32) != want.view(np.uint32))))
    assert bad.size == 0, f"{what}: {len(bad)} of {got.size} differ, first at {bad[:4].tolist()}"


@pytest.fixture(scope="module")
def lib():
    from openmsftl_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


# ---- the walk is the sorted definition --------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 8, 9, 33])
def test_walk_equals_the_sorted_model(m):
    rng = np.random.default_rng(40 + m)
    n = 3 * (m + 1) + 5
    bit_cases = {"random": rng.random((m, 257)) < 0.5, "all_set": np.ones((m, 40), bool),
                 "all_clear": np.zeros((m, 40), bool), "edges": stm.edge_bits(m, n, rng)}
    for b in stm.trims(m):
        for sname, make in stm.SCALES.items():
            s = make(m, rng, b)
            for bname, B in bit_cases.items():
                same_bits(stm.walk(B, s, b), stm.expected(B, s, b), f"m={m} b={b} {sname} {bname}")


def test_walk_takes_a_scale_with_its_sign_bit_as_it_stands():
    rng = np.random.default_rng(7)
    m = 9
    B = stm.edge_bits(m, 45, rng)
    s = stm.SCALES["tie_groups"](m, rng, 0)
    s[[1, 4, 6]] *= F(-1.0)
    s[2], s[7] = F(-0.0), -np.inf
    for b in stm.trims(m):
        same_bits(stm.walk(B, s, b), stm.expected(B, s, b), f"b={b}")


def test_model_hand_columns():
    def one(bits, scales, b):
        return stm.expected(np.array(bits, bool).reshape(-1, 1), F(scales), b)[0]

    assert one([1, 0, 0], [1.0, 2.0, 4.0], 0) == F(5.0) / F(3.0)              # -1 + 2 + 4
    assert one([1, 0, 0], [1.0, 2.0, 4.0], 1) == F(2.0)
    assert one([1, 1, 0], [1.0, 2.0, 4.0], 1) == F(-1.0)                      # -2 | -1 | 4
    assert one([0, 1, 0], [np.nan, 2.0, 4.0], 1) == F(4.0)                    # -2 | 4 | NaN
    assert np.isnan(one([1, 1, 0], [np.nan, 2.0, 4.0], 0))
    big = F(2.0 ** 25)
    assert one([1, 0, 0], [big, 1.0, big], 0) == F(0.0)                       # (-2^25 + 1) + 2^25
    z = one([1, 1, 0], [0.0, 0.0, 0.0], 0)
    assert z == 0 and not np.signbit(z)                                       # +0.0, never -0.0
    # all scales equal: the median is the majority vote, a tie gives +0.0
    rng = np.random.default_rng(3)
    for m in (1, 2, 5, 8):
        B = rng.random((m, 300)) < 0.5
        same_bits(stm.expected(B, np.full(m, 0.375, F), (m - 1) // 2), sm.vote(B, 0.375), f"m={m}")


# ---- the C ABI ----------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound(lib):
    from openmsftl_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = {name: args.count(",") + 1
            for name, args in re.findall(r"\b(fc_sign_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S)}
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                        text=True, check=True).stdout
    exported = set(re.findall(r"\s[TW]\s+(\S+)", nm))
    for name in NEW:
        assert name in decl and name in exported, name
        assert len(_lib.SIGNATURES[name][1]) == decl[name], name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    assert lib.fc_abi_version() == 4                                          # an addition only
    assert re.search(r"#define FC_ABI_VERSION 4\b", open(HEADER).read())


def test_argument_errors_do_not_touch_gpu(lib):
    buf = ctypes.create_string_buffer(1 << 16)
    a = (ctypes.addressof(buf) + 15) & ~15
    n, m = 4096, 5
    err = lambda: lib.fc_last_error()                                  # noqa: E731
    need = lib.fc_sign_trim_workspace_bytes(n, m)
    assert need % 16 == 0

    def call(v_=a, m_=m, n_=n, t_=1, o_=a + 1024, w_=a + 4096, wsb=max(need, 16)):
        return lib.fc_sign_trim(v_, m_, n_, t_, o_, w_, wsb, None)

    assert call(v_=None) == FC_ERR_ARG and b"views_dev is NULL" in err()
    assert call(o_=None) == FC_ERR_ARG and b"out is NULL" in err()
    for bad in (0, -1, 129):
        assert call(m_=bad) == FC_ERR_ARG and b"m=" in err()
    for bad_m, bad_t in ((5, -1), (5, 3), (4, 2), (1, 1), (128, 64)):
        assert call(m_=bad_m, t_=bad_t) == FC_ERR_ARG and b"trim=" in err()
    assert call(n_=0) == FC_ERR_ARG and b"n=0" in err()
    assert call(n_=1 << 32) == FC_ERR_ARG and b"n=" in err()
    assert call(o_=a + 1024 + 8) == FC_ERR_ARG and b"out must be 16-byte aligned" in err()
    assert call(w_=a + 4096 + 8) == FC_ERR_ARG and b"workspace must be 16-byte aligned" in err()
    if need:                                                           # fc_packets_trim's rule
        assert call(w_=None) == FC_ERR_ARG and b"workspace is NULL" in err()
        assert call(wsb=need - 1) == FC_ERR_WORKSPACE and b"workspace" in err()
    for n_, m_ in ((0, 4), (1 << 32, 4), (4096, 0), (4096, 129)):
        assert lib.fc_sign_trim_workspace_bytes(n_, m_) == 0


# ---- codec and gar --------------------------------------------------------------------------
def test_codec_checks_need_no_gpu(lib):
    import torch
    from openmsftl_amd import codec
    with pytest.raises(ValueError, match="no packets"):
        codec.trimmed_mean_sign([], 0)
    with pytest.raises(TypeError, match="sign packets"):
        codec.trimmed_mean_sign([object()], 0)
    cpu = torch.zeros(4, dtype=torch.int32)                            # 4 = fc_sign_words(100)
    pk = [codec.SignPacket(words=cpu, hdr=None, n=100) for _ in range(4)]
    for bad, why in ((-1, "negative"), (2, r"2 \* trim"), (1.0, "integer"), (True, "integer")):
        with pytest.raises(ValueError, match=why):
            codec.trimmed_mean_sign(pk, bad)
    with pytest.raises(ValueError, match="at most 128"):
        codec.trimmed_mean_sign(pk * 33, 0)
    with pytest.raises(ValueError, match="share n"):
        codec.trimmed_mean_sign(pk + [codec.SignPacket(words=cpu, hdr=None, n=101)], 0)


class _FakeCodec:
    """Stands in for codec while CoordinateTrim.aggregate_packets runs on the host."""

    def __init__(self):
        self.calls = []

    def trimmed_mean(self, packets, trim, out=None):
        self.calls.append(("idxval", len(packets), trim, out))
        return "agg"

    def trimmed_mean_sign(self, packets, trim, out=None):
        self.calls.append(("sign", len(packets), trim, out))
        return "agg-sign"


def test_coordinate_trim_dispatches_by_packet_kind(monkeypatch):
    from openmsftl_amd import codec, gar
    sp = codec.SignPacket(words=None, hdr=None, n=8)
    fake = _FakeCodec()
    monkeypatch.setattr(gar, "codec", fake)
    r = gar.TrimmedMean({"trim_count": 2})
    assert r.aggregate_packets([sp] * 7, out="o") == "agg-sign" and fake.calls[-1] == ("sign", 7, 2, "o")
    assert r.aggregate_packets([object()] * 5) == "agg" and fake.calls[-1] == ("idxval", 5, 2, None)
    med = gar.CoordinateMedian({})
    assert med.aggregate_packets([sp] * 8) == "agg-sign" and fake.calls[-1] == ("sign", 8, 3, None)
    done = len(fake.calls)
    for rule in (r, med):
        with pytest.raises(TypeError, match="one kind"):
            rule.aggregate_packets([sp, object(), sp])
        rule.gradient_weights = np.full(3, 1 / 3, F)
        with pytest.raises(ValueError, match="gradient_weights"):
            rule.aggregate_packets([sp] * 3)
    assert len(fake.calls) == done


# ---- routing on stub clients --------------------------------------------------------------------
def _clients(m=3, n=100, fn="sign", dtype=F, **cfg):
    from openmsftl_amd import Compression
    return [types.SimpleNamespace(C=Compression(dict({"compression_function": fn}, **cfg)),
                                  grad=np.zeros(n, dtype), client_id=i) for i in range(m)]


def _agg(scheme="fed_avg", **cfg):
    from openmsftl_amd.aggregation import Aggregator
    return Aggregator(dict({"aggregation_scheme": scheme}, **cfg))


TRIMS = (("trimmed_mean", {}), ("trimmed_mean", {"trim_count": 1}), ("coordinate_median", {}))


def test_sign_trim_routes_the_two_schemes(lib):
    from openmsftl_amd.aggregation import (sign_gram_route, sign_route, sign_trim_resident_bytes,
                                           sign_trim_route, sign_trim_wanted)
    for scheme, cfg in TRIMS:
        agg = _agg(scheme, sign_trim=True, **cfg)
        assert sign_trim_wanted(agg)
        assert sign_trim_route(agg, _clients()) is True
        assert sign_trim_route(agg, _clients(error_feedback=True)) is True
        assert sign_trim_route(agg, _clients(m=128)) is True
        assert sign_route(agg, _clients()) is False                    # steps aside
        assert sign_gram_route(agg, _clients()) is False
        assert sign_trim_route(_agg(scheme, sign_trim=True, pc_analysis="gram", **cfg), _clients()) is True
        assert agg.agg_path is None
    n, m = 1 << 20, 16
    packets = m * ((4 * lib.fc_sign_words(n) + 96 + 255) & ~255)
    ws = lib.fc_sign_trim_workspace_bytes(n, m)
    assert sign_trim_resident_bytes(n, m) == packets + 8 * n + ws
    assert sign_trim_resident_bytes(n, m, packets_bytes=12345) == 12345 + 4 * n + ws
    assert sign_trim_resident_bytes(n, m, True) == (packets + 8 * n + ws + 8 * m * m
                                                    + lib.fc_sign_gram_workspace_bytes(n, m))


def test_sign_trim_names_each_failed_condition(lib):
    from openmsftl_amd.aggregation import sign_trim_route
    stub = _clients()
    stub[1].C = types.SimpleNamespace(compression_function="sign", error_feedback=False)
    for scheme, cfg in TRIMS:
        def agg(**more):
            return _agg(scheme, sign_trim=True, **cfg, **more)
        for a, cl, why in (
                (agg(), stub, "drop-in Compression"),
                (agg(num_hierarchies=1, cluster_size_list=[2]), _clients(), "no hierarchies"),
                (agg(devices=2), _clients(), "one device"),
                (agg(), _clients(dtype=np.float64), "1-D float32 gradients"),
                (agg(), _clients() + _clients(1, n=101), "gradients of one length"),
                (agg(), _clients(n=0), "n > 0"),
                (agg(), _clients(m=129), r"at most 128 clients \(got 129\)"),
                (agg(device_budget_bytes=1000), _clients(m=8, n=4096),
                 r"device_budget_bytes \(\d+ > 1000 bytes\)")):
            with pytest.raises(NotImplementedError, match=r"the sign-trim route \(sign_trim\) needs .*" + why):
                sign_trim_route(a, cl)
            with pytest.raises(NotImplementedError, match=r"the sign-trim route \(sign_trim\) needs .*" + why):
                a.aggregate_grads(cl)                                  # before a GPU is touched
            assert a.agg_path is None and a.agg_grad is None
        weighted = agg()
        weighted.gar.gradient_weights = np.full(3, 1 / 3, F)
        with pytest.raises(ValueError, match="is unweighted: gradient_weights must be None"):
            sign_trim_route(weighted, _clients())
        with pytest.raises(ValueError, match="is unweighted: gradient_weights must be None"):
            weighted.aggregate_grads(_clients())
        assert weighted.agg_path is None and weighted.agg_grad is None


def test_the_key_does_nothing_for_other_schemes_and_other_rounds(lib):
    from openmsftl_amd import aggregation as ag
    # krum (and every other scheme without a consumer) still refuses a round of sign clients
    for scheme, cfg in (("krum", {}), ("geometric_median", {}), ("centered_clip", {"cclip_tau": 1.0}),
                        ("spectral_gram", {"rank": 2, "adaptive_rank_th": 0}), ("fed_avg", {"pc_analysis": "gram"})):
        a = _agg(scheme, sign_trim=True, **cfg)
        assert not ag.sign_trim_wanted(a) and ag.sign_trim_route(a, _clients()) is False
        with pytest.raises(NotImplementedError, match="no consumer of sign packets"):
            a.aggregate_grads(_clients())
    # fed_avg and sign_majority keep the "sign" route
    for scheme in ("fed_avg", "sign_majority"):
        a = _agg(scheme, sign_trim=True)
        assert ag.sign_trim_route(a, _clients()) is False and ag.sign_route(a, _clients()) is True
    for scheme, cfg in TRIMS:
        # a trim round of 'top' clients still routes to "gram"
        a = _agg(scheme, sign_trim=True, **cfg)
        top = _clients(n=1000, fn="top", fraction_coordinate=0.1)
        assert ag.sign_trim_route(a, top) is False and ag.sign_route(a, top) is False
        assert ag.gram_wanted(a) and ag.gram_route_k(a, top) == 100
        # a round that is not all 'sign' is the "gram" route's to refuse, as without the key
        for key in ({"sign_trim": True}, {}):
            with pytest.raises(NotImplementedError, match="every client to compress with 'top'"):
                _agg(scheme, **cfg, **key).aggregate_grads(_clients() + _clients(1, fn="top"))
        # without the key (or with it False, or with sign_geometry alone) the refusal stands
        for key in ({}, {"sign_trim": False}, {"sign_geometry": True}):
            a = _agg(scheme, **cfg, **key)
            assert ag.sign_trim_route(a, _clients()) is False
            with pytest.raises(NotImplementedError, match="no consumer of sign packets"):
                ag.sign_route(a, _clients())
            with pytest.raises(NotImplementedError, match="no consumer of sign packets"):
                a.aggregate_grads(_clients())


def test_aggregate_wire_refusals_on_host_bytes(lib):
    rng = np.random.default_rng(5)
    B, s = rng.random((3, 129)) < 0.5, F([0.5, 1.0, 2.0])
    raws = gm.packets(B, s)
    for scheme, cfg in TRIMS:
        for key in ({}, {"sign_geometry": True}):
            with pytest.raises(NotImplementedError, match="aggregate_wire needs .*sign packets"):
                _agg(scheme, **cfg, **key).aggregate_wire(raws)
        with pytest.raises(NotImplementedError, match=r"sign-trim route .*at most 128 payloads \(got 129\)"):
            _agg(scheme, sign_trim=True, **cfg).aggregate_wire([raws[0]] * 129)
        with pytest.raises(NotImplementedError, match=r"sign-trim route .*device_budget_bytes \(\d+ > 1000 bytes\)"):
            _agg(scheme, sign_trim=True, device_budget_bytes=1000, **cfg).aggregate_wire(raws)
        with pytest.raises(NotImplementedError, match="one device"):
            _agg(scheme, sign_trim=True, devices=2, **cfg).aggregate_wire(raws)
        with pytest.raises(NotImplementedError, match="no hierarchies"):
            _agg(scheme, sign_trim=True, num_hierarchies=1, cluster_size_list=[2], **cfg).aggregate_wire(raws)
        weighted = _agg(scheme, sign_trim=True, **cfg)
        weighted.gar.gradient_weights = np.full(3, 1 / 3, F)
        with pytest.raises(ValueError, match="is unweighted: gradient_weights must be None"):
            weighted.aggregate_wire(raws)
        bad = bytearray(raws[1])
        bad[-1] = 0x80
        with pytest.raises(ValueError, match="payload 1: sign wire: pad word"):
            _agg(scheme, sign_trim=True, **cfg).aggregate_wire([raws[0], bytes(bad)])
        other = gm.packets(B[:1, :128], s[:1])[0]
        with pytest.raises(NotImplementedError, match="one length n"):
            _agg(scheme, sign_trim=True, **cfg).aggregate_wire([raws[0], other])
    with pytest.raises(NotImplementedError, match="aggregate_wire needs .*sign packets"):
        _agg("krum", sign_trim=True).aggregate_wire(raws)
