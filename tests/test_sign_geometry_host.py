"""The geometry of scaled-sign packets on the host: the C ABI of fc_sign_gram / fc_sign_dot and
their argument errors (reported before the GPU is touched), the workspace sizes, the model's hand
cases, the rules' coefficient functions on model Grams, and the Aggregator's "sign_geometry"
routing on stub clients.

Run:  python -m pytest tests/test_sign_geometry_host.py -m "not gpu" -q

No GPU is needed: the library loads without one (tests/test_lib_abi.py).
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fedcodec.h")
F = np.float32
NEW = ("fc_sign_gram_workspace_bytes", "fc_sign_gram", "fc_sign_dot_workspace_bytes", "fc_sign_dot")


@pytest.fixture(scope="module")
def lib():
    from openmsftl_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


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
        getattr(lib, name)
    assert lib.fc_abi_version() == 4
    assert re.search(r"#define FC_ABI_VERSION 4\b", open(HEADER).read())


def test_argument_errors_do_not_touch_gpu(lib):
    buf = ctypes.create_string_buffer(1 << 16)
    a = (ctypes.addressof(buf) + 15) & ~15
    n, m = 4096, 5
    err = lambda: lib.fc_last_error()                                  # noqa: E731
    gws, dws = lib.fc_sign_gram_workspace_bytes(n, m), lib.fc_sign_dot_workspace_bytes(n, m)
    assert gws > 0 and dws > 0

    def gram(v_=a, m_=m, n_=n, g_=a + 1024, w_=a + 4096, wsb=gws):
        return lib.fc_sign_gram(v_, m_, n_, g_, w_, wsb, None)

    def dot(v_=a, m_=m, n_=n, x_=a + 2048, o_=a + 1024, w_=a + 4096, wsb=dws):
        return lib.fc_sign_dot(v_, m_, n_, x_, o_, w_, wsb, None)

    for call in (gram, dot):
        assert call(v_=None) == -1 and b"views_dev is NULL" in err()
        assert call(w_=None) == -1 and b"workspace is NULL" in err()
        for bad in (0, -1, 129):
            assert call(m_=bad) == -1 and b"m=" in err()
        assert call(n_=0) == -1 and b"n=0" in err()
        assert call(n_=1 << 32) == -1 and b"n=" in err()
        assert call(w_=a + 4096 + 8) == -1 and b"workspace must be 16-byte aligned" in err()
        assert call(wsb=15) == -3 and b"workspace" in err()
    assert gram(g_=None) == -1 and b"gram is NULL" in err()
    assert gram(g_=a + 1024 + 8) == -1 and b"gram must be 16-byte aligned" in err()
    assert gram(wsb=gws - 1) == -3
    assert dot(o_=None) == -1 and b"out is NULL" in err()
    assert dot(o_=a + 1024 + 8) == -1 and b"out must be 16-byte aligned" in err()
    assert dot(x_=a + 2048 + 4) == -1 and b"v must be 16-byte aligned" in err()
    assert dot(wsb=dws - 1) == -3


def test_workspace_sizes_are_monotone(lib):
    ns = [1, 31, 32, 33, 127, 128, 129, 2047, 2048, 2049, 8191, 8193, 65536, 1_000_003, 1 << 24,
          1 << 27, (1 << 32) - 1]
    for fn in (lib.fc_sign_gram_workspace_bytes, lib.fc_sign_dot_workspace_bytes):
        table = np.array([[fn(n, m) for m in range(1, 129)] for n in ns], dtype=np.int64)
        assert (table > 0).all() and (table % 16 == 0).all()
        assert (np.diff(table, axis=0) >= 0).all() and (np.diff(table, axis=1) >= 0).all()
        assert fn(0, 4) == 0 and fn(1 << 32, 4) == 0 and fn(4096, 0) == 0 and fn(4096, 129) == 0
        assert fn(1 << 27, 128) <= 32 << 20                       # far below the packets (m n / 8)


# ---- the model on hand cases --------------------------------------------------------------------
def test_model_identical_rows_and_complements():
    rng = np.random.default_rng(1)
    b = rng.random(77) < 0.4
    B = np.stack([b, b, ~b])
    assert gm.hamming(B).tolist() == [[0, 0, 77], [0, 0, 77], [77, 77, 0]]
    s = F([0.5, 2.0, 3.0])
    K = gm.gram(B, s)
    assert K.tolist() == [[0.25 * 77, 77.0, -1.5 * 77], [77.0, 4.0 * 77, -6.0 * 77],
                          [-1.5 * 77, -6.0 * 77, 9.0 * 77]]
    G = gm.decoded(B, s).astype(np.float64)
    assert (G @ G.T).tolist() == K.tolist()


def test_model_n_1_and_only_bit_32_of_33():
    B = np.array([[True], [False]])
    assert gm.hamming(B).tolist() == [[0, 1], [1, 0]]
    assert gm.gram(B, F([2.0, 3.0])).tolist() == [[4.0, -6.0], [-6.0, 9.0]]
    B = np.zeros((2, 33), bool)
    B[0, 32] = True
    assert int(sm.words_of(B[0])[1]) == 1 and int(sm.words_of(B[0])[0]) == 0
    assert gm.hamming(B).tolist() == [[0, 1], [1, 0]]
    assert gm.gram(B, F([1.0, 1.0])).tolist() == [[33.0, 31.0], [31.0, 33.0]]
    D, bound = gm.dot(B, F([1.0, 1.0]))
    assert D.tolist() == [31.0, 33.0] and bound == 0.0
    v = np.arange(33, dtype=F)
    D, bound = gm.dot(B, F([1.0, 1.0]), v)
    assert D.tolist() == [528.0 - 64.0, 528.0] and bound > 0
    assert gm.dot_out(B, F([0.5, np.inf]), v).tolist()[:1] == [232.0]
    assert np.isnan(gm.dot_out(B, F([0.5, np.inf]), v)[1])


def test_model_gram_is_the_correctly_rounded_product_and_marks_non_finite_scales():
    rng = np.random.default_rng(2)
    B = rng.random((4, 1001)) < 0.5
    s = F([3.3e-19, 7.7e17, np.nan, 1.1])
    K = gm.gram(B, s)
    assert np.isnan(K[2]).all() and np.isnan(K[:, 2]).all()
    keep = [0, 1, 3]
    A = gm.agreement(B)
    for i in keep:
        for j in keep:
            # one IEEE multiply of the exact product of the scales by the exact integer
            assert K[i, j] == (np.float64(s[i]) * np.float64(s[j])) * np.float64(A[i, j])
    assert (K[np.ix_(keep, keep)] == K[np.ix_(keep, keep)].T).all()


# ---- the rules' coefficient functions on model Grams --------------------------------------------
def _round(m=7, n=4099, seed=3):
    rng = np.random.default_rng(seed)
    B = rng.random((m, n)) < rng.uniform(0.3, 0.7, (m, 1))
    # two sign-flipped outliers; not exact complements, which would make the Gram matrix singular
    # (a singular value at 0 is sqrt(rounding error), not comparable at allclose's defaults)
    B[1], B[4] = ~B[0] ^ (rng.random(n) < 0.1), ~B[2] ^ (rng.random(n) < 0.1)
    s = rng.uniform(0.5, 2.0, m).astype(F)
    return B, s


def test_rules_on_model_grams_match_the_dense_product():
    from openmsftl_amd import gar
    B, s = _round()
    K = gm.gram(B, s)
    G = gm.decoded(B, s).astype(np.float64)
    Kd = G @ G.T
    assert np.allclose(K, Kd)
    w = np.full(len(s), 1.0 / len(s))
    assert np.allclose(gar.Krum.krum_scores(K, 0.5), gar.Krum.krum_scores(Kd, 0.5))
    assert gar.Krum.select(K, 0.5) == gar.Krum.select(Kd, 0.5)
    assert np.allclose(gar.gram_singular_values(K), gar.gram_singular_values(Kd))
    for a_, b_ in zip(gar.spectral_coeffs(K, w, B.shape[1], rank=3),
                      gar.spectral_coeffs(Kd, w, B.shape[1], rank=3)):
        assert np.allclose(a_, b_)
    rs = gm.dot_out(B, s)[:-1]
    assert np.allclose(rs, G.sum(axis=1))
    for a_, b_ in zip(gar.spectral_coeffs(K, w, B.shape[1], adaptive_rank_th=0.9, row_sums=rs),
                      gar.spectral_coeffs(Kd, w, B.shape[1], adaptive_rank_th=0.9, row_sums=G.sum(axis=1))):
        assert np.allclose(a_, b_)
    assert np.allclose(gar.geometric_median_coeffs(K, w)[0], gar.geometric_median_coeffs(Kd, w)[0])
    v = np.random.default_rng(4).standard_normal(B.shape[1]).astype(F)
    r = gm.dot_out(B, s, v)
    assert np.allclose(r[:-1], G @ v.astype(np.float64))
    for a_, b_ in zip(gar.centered_clip_coeffs(K, r[:-1], r[-1], 5.0),
                      gar.centered_clip_coeffs(Kd, G @ v.astype(np.float64), float(v.astype(np.float64) @ v), 5.0)):
        assert np.allclose(a_, b_)


def test_gar_refuses_a_round_of_mixed_packet_kinds():
    from openmsftl_amd import codec, gar
    sp = codec.SignPacket(words=None, hdr=None, n=8)
    for rule in (gar.Krum({}), gar.GeometricMedian({})):
        with pytest.raises(TypeError, match="one kind"):
            rule.aggregate_packets([sp, object()])


# ---- routing on stub clients --------------------------------------------------------------------
def _clients(m=3, n=100, fn="sign", dtype=F, **cfg):
    from openmsftl_amd import Compression
    return [types.SimpleNamespace(C=Compression(dict({"compression_function": fn}, **cfg)),
                                  grad=np.zeros(n, dtype), client_id=i) for i in range(m)]


def _agg(scheme="fed_avg", **cfg):
    from openmsftl_amd.aggregation import Aggregator
    return Aggregator(dict({"aggregation_scheme": scheme}, **cfg))


SCHEMES = (("krum", {}), ("spectral_gram", {"rank": 2, "adaptive_rank_th": 0}), ("geometric_median", {}),
           ("centered_clip", {"cclip_tau": 1.0}), ("fed_avg", {"pc_analysis": "gram"}))


def test_sign_geometry_routes_each_scheme(lib):
    from openmsftl_amd.aggregation import sign_gram_route, sign_route, sign_gram_resident_bytes
    for scheme, cfg in SCHEMES:
        agg = _agg(scheme, sign_geometry=True, **cfg)
        assert sign_gram_route(agg, _clients()) is True
        assert sign_gram_route(agg, _clients(error_feedback=True)) is True
        assert sign_route(agg, _clients()) is False                    # not the "sign" route's
        assert sign_gram_route(agg, _clients(fn="top")) is False       # the "gram" route's business
        assert sign_gram_route(agg, _clients(m=128)) is True
        agg.gar.gradient_weights = np.full(3, 1 / 3, F)
        assert sign_gram_route(agg, _clients()) is True
    # a plain fed_avg round keeps the "sign" route whatever the key says
    agg = _agg(sign_geometry=True)
    assert sign_gram_route(agg, _clients()) is False and sign_route(agg, _clients()) is True
    assert sign_gram_route(_agg("sign_majority", sign_geometry=True), _clients()) is False
    n, m = 1 << 20, 16
    assert sign_gram_resident_bytes(n, m) >= m * n // 8 + 8 * n + 8 * m * m
    assert sign_gram_resident_bytes(n, m) == (
        m * ((4 * lib.fc_sign_words(n) + 96 + 255) & ~255) + 8 * n + 8 * m * m
        + lib.fc_sign_gram_workspace_bytes(n, m) + lib.fc_sign_dot_workspace_bytes(n, m))


def test_sign_geometry_names_each_failed_condition(lib):
    from openmsftl_amd.aggregation import sign_gram_route
    stub = _clients()
    stub[1].C = types.SimpleNamespace(compression_function="sign", error_feedback=False)
    K = "krum"
    for agg, cl, why in (
            (_agg(K, sign_geometry=True), stub, "drop-in Compression"),
            (_agg(K, sign_geometry=True), _clients(dtype=np.float64), "1-D float32 gradients"),
            (_agg(K, sign_geometry=True), _clients() + _clients(1, n=101), "gradients of one length"),
            (_agg(K, sign_geometry=True), _clients(n=0), "n > 0"),
            (_agg(K, sign_geometry=True, num_hierarchies=1, cluster_size_list=[2]), _clients(), "no hierarchies"),
            (_agg(K, sign_geometry=True, devices=2), _clients(), "one device"),
            (_agg(K, sign_geometry=True), _clients(m=129), r"at most 128 clients \(got 129\)"),
            (_agg(K, sign_geometry=True, device_budget_bytes=1000), _clients(m=8, n=4096),
             r"device_budget_bytes \(\d+ > 1000 bytes\)")):
        with pytest.raises(NotImplementedError, match="sign-gram route.*" + why):
            sign_gram_route(agg, cl)
        with pytest.raises(NotImplementedError, match="sign-gram route.*" + why):
            agg.aggregate_grads(cl)                                    # before a GPU is touched
    a = _agg("geometric_median", sign_geometry=True)
    a.gar.gradient_weights = np.full(3, 1 / 3, np.float64)
    with pytest.raises(NotImplementedError, match="float32 GAR weights"):
        sign_gram_route(a, _clients())
    # a round that mixes 'sign' and 'top' clients is no sign round: the "gram" route refuses it
    with pytest.raises(NotImplementedError, match="every client to compress with 'top'"):
        _agg(K, sign_geometry=True).aggregate_grads(_clients() + _clients(1, fn="top"))


def test_trim_rules_and_rounds_without_the_key_still_raise(lib):
    from openmsftl_amd.aggregation import sign_gram_route, sign_route
    for scheme in ("trimmed_mean", "coordinate_median"):
        agg = _agg(scheme, sign_geometry=True)
        assert sign_gram_route(agg, _clients()) is False
        with pytest.raises(NotImplementedError, match="no consumer of sign packets"):
            sign_route(agg, _clients())
        with pytest.raises(NotImplementedError, match="no consumer of sign packets"):
            agg.aggregate_grads(_clients())
    for scheme, cfg in SCHEMES:
        for key in ({}, {"sign_geometry": False}):
            agg = _agg(scheme, **cfg, **key)
            assert sign_gram_route(agg, _clients()) is False
            with pytest.raises(NotImplementedError, match="no consumer of sign packets"):
                agg.aggregate_grads(_clients())


def test_aggregate_wire_refusals_on_host_bytes(lib):
    B, s = _round(m=7, n=129)
    raws = gm.packets(B[:3], s[:3])
    for scheme in ("krum", "geometric_median"):
        with pytest.raises(NotImplementedError, match="sign packets"):
            _agg(scheme).aggregate_wire(raws)                          # without the key
    for scheme in ("trimmed_mean", "coordinate_median"):
        with pytest.raises(NotImplementedError, match="sign packets"):
            _agg(scheme, sign_geometry=True).aggregate_wire(raws)
    with pytest.raises(NotImplementedError, match=r"at most 128 payloads for the sign-gram route \(got 129\)"):
        _agg("krum", sign_geometry=True).aggregate_wire([raws[0]] * 129)
    with pytest.raises(NotImplementedError, match=r"device_budget_bytes \(\d+ > 1000 bytes\)"):
        _agg("krum", sign_geometry=True, device_budget_bytes=1000).aggregate_wire(raws)
    with pytest.raises(NotImplementedError, match="one device"):
        _agg("krum", sign_geometry=True, devices=2).aggregate_wire(raws)
    bad = bytearray(raws[1])
    bad[-1] = 0x80
    with pytest.raises(ValueError, match="payload 1: sign wire: pad word"):
        _agg("krum", sign_geometry=True).aggregate_wire([raws[0], bytes(bad)])
    other = gm.packets(B[:1, :128], s[:1])[0]
    with pytest.raises(NotImplementedError, match="one length n"):
        _agg("krum", sign_geometry=True).aggregate_wire([raws[0], other])
