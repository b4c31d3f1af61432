"""The CPU packet builder and consumer of oracle/packet_oracle.py (no GPU).

The builder states the wire format of include/fedcodec.h, the consumer the decode and fold
rules of csrc/fc_decode.hip; tests/test_packet_consumers_gpu.py feeds the GPU decoders what the
builder makes and compares with the consumer, so both are checked here against hand-written
expectations and against the reference's own goldens.
"""
import struct

import numpy as np
import pytest

from conftest import golden
from oracle import compression_oracle as co
from oracle import gar_oracle as go
from oracle import packet_oracle as po
from oracle import philox as ph

G = golden()
NEG0 = np.float32(-0.0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.dtype(f"<u{a.dtype.itemsize}"))


# ---- the format, on a hand-written example -----------------------------------------------
def test_qoff_packing_three_chunks():
    n = 2 * 8192 + 100                                  # chunk 2 holds 100 elements
    idx = [0, 2047, 2048, 4096, 8191, 16384 + 5, 16384 + 99]
    val = np.arange(1, 8, dtype=np.float32)
    f = po.build_idxval(n, idx, val, thresh=0, codec=po.CODEC_TOP, k=7)
    assert f["idx"].dtype == np.uint16 and f["val"].dtype == np.float32
    assert f["cnt"].dtype == np.uint32 and f["qoff"].dtype == np.uint64
    assert f["idx"].shape == f["val"].shape == (3 * 8192,)
    assert f["cnt"].tolist() == [5, 0, 2]
    # quarter starts 1, 2, 3 in bits 0-15 / 16-31 / 32-47, cnt in bits 48-63
    assert f["qoff"].tolist() == [2 | 3 << 16 | 4 << 32 | 5 << 48, 0,
                                  2 | 2 << 16 | 2 << 32 | 2 << 48]
    assert f["idx"][:5].tolist() == [0, 2047, 2048, 4096, 8191]
    assert f["val"][:5].tolist() == [1, 2, 3, 4, 5]
    assert f["idx"][16384:16386].tolist() == [5, 99]
    assert f["val"][16384:16386].tolist() == [6, 7]
    unlisted = np.ones(3 * 8192, dtype=bool)
    unlisted[:5] = False
    unlisted[16384:16386] = False
    assert np.all(f["idx"][unlisted] == 0xFFFF) and np.all(np.isnan(f["val"][unlisted]))
    gidx, gval = po.listed_entries(f)
    assert gidx.tolist() == idx and gval.tolist() == val.tolist()


def test_header_layout_is_fc_packet_hdr():
    f = po.build_idxval(20_011, [3, 9000], [1.0, 2.0], thresh=0x1234_5678_9ABC, lower=0x1111,
                        codec=po.CODEC_RAND, key_mode=po.KEY_PHILOX, k=2, seed=(7 << 32) | 5,
                        offset=11, p=0.25, n_definite=1, n_cand=1)
    raw = f["hdr"].tobytes()
    assert len(raw) == 96
    (thresh, lower, n, k, n_ent, ib, codec, status, n_def, n_cand, seed, offset, p, chunk, fmt,
     key_mode, r0, r1, r2) = struct.unpack("<QQIIIIIIIIQQdIIIIII", raw)
    assert (thresh, lower, n, k, n_ent, ib) == (0x1234_5678_9ABC, 0x1111, 20_011, 2, 2, 15)
    assert (codec, status, n_def, n_cand) == (2, 0, 1, 1)
    assert (seed, offset, p, chunk, fmt, key_mode) == ((7 << 32) | 5, 11, 0.25, 8192, 0, 1)
    assert (r0, r1, r2) == (0, 0, 0)
    # fc_mask_encode's static header: no entry count, no key mode, no threshold
    m = po.build_idxval(20_011, [3], [1.0], thresh=0, codec=po.CODEC_DROPOUT_UNBIASED, p=0.3)
    assert int(m["hdr"]["n_entries"]) == 0 and int(m["hdr"]["key_mode"]) == 0
    assert po.index_bits(1) == 1 and po.index_bits(2) == 1 and po.index_bits(3) == 2
    assert po.index_bits(8192) == 13 and po.index_bits(8193) == 14


def test_builder_rejects_malformed_entries():
    for idx in ([2, 1], [1, 1], [-1], [10]):
        with pytest.raises(ValueError):
            po.build_idxval(10, idx, np.zeros(len(idx)), thresh=0, codec=po.CODEC_TOP)


def test_without_qoff_and_bitmap_layout():
    n = 8192 + 40
    idx = [1, 31, 32, 8191, 8192, 8192 + 39]
    val = np.array([1, -2, 3, -4, 5, -6], dtype=np.float32)
    f = po.build_idxval(n, idx, val, thresh=0, codec=po.CODEC_TOP, with_qoff=False)
    assert f["qoff"] is None
    b = po.build_bitmap(n, idx, val, codec=po.CODEC_DROPOUT_BIASED, p=0.5)
    assert b["bitmap"].shape == (2 * 256,) and b["bitmap"].dtype == np.uint32
    assert int(b["bitmap"][0]) == (1 << 1) | (1 << 31) and int(b["bitmap"][1]) == 1
    assert int(b["bitmap"][255]) == 1 << 31
    assert int(b["bitmap"][256]) == 1 and int(b["bitmap"][257]) == 1 << 7
    assert b["cnt"].tolist() == [4, 2]
    assert b["val"][:4].tolist() == [1, -2, 3, -4] and b["val"][8192:8194].tolist() == [5, -6]
    assert np.all(np.isnan(b["val"][4:8192]))
    assert int(b["hdr"]["format"]) == 1
    want = np.zeros(n, dtype=np.float32)
    want[idx] = val
    assert po.decode_packet(f).tobytes() == want.tobytes()
    assert po.decode_packet(b).tobytes() == want.tobytes()


# ---- the consumer's rules ----------------------------------------------------------------
def test_threshold_drops_slack_and_cuts_ties_by_index():
    n = 100
    ib = po.index_bits(n)
    one = 0x3F800000                                    # bits of 1.0f
    idx = [10, 20, 30, 40, 50]
    val = np.array([0.5, 1.0, -1.0, NEG0, 2.0], dtype=np.float32)
    # T64 = (key(1.0), index 30): of the two |v| = 1 entries the higher index stays
    f = po.build_idxval(n, idx, val, thresh=(one << ib) | 30, codec=po.CODEC_TOP, k=2)
    out = po.decode_packet(f)
    want = np.zeros(n, dtype=np.float32)
    want[30], want[50] = -1.0, 2.0
    assert out.tobytes() == want.tobytes()
    # thresh == 0 keeps everything listed, -0.0 included
    f0 = po.build_idxval(n, idx, val, thresh=0, codec=po.CODEC_TOP, k=n)
    out0 = po.decode_packet(f0)
    assert _bits(out0)[40] == 0x80000000 and out0[10] == 0.5
    # the select-nothing threshold of k = 0 keeps nothing, not even a NaN
    val2 = val.copy()
    val2[0] = np.nan
    fn = po.build_idxval(n, idx, val2, thresh=po.NOTHING, codec=po.CODEC_TOP, k=0)
    assert po.decode_packet(fn).tobytes() == np.zeros(n, dtype=np.float32).tobytes()
    # a NaN's key is above +inf's
    inf_key = 0x7F800000
    fi = po.build_idxval(n, idx, np.array([np.nan, np.inf, -np.inf, 1.0, 3e38], np.float32),
                         thresh=(inf_key << ib) | 25, codec=po.CODEC_TOP, k=2)
    oi = po.decode_packet(fi)
    assert np.isnan(oi[10]) and oi[20] == 0 and oi[30] == -np.inf and oi[50] == 0


def test_philox_keys_select_by_the_elements_word():
    n, seed, offset = 20_011, 0xABCDEF0123, 3
    words = ph.element_words(n, seed, offset)
    idx = np.array([0, 63, 64, 255, 256, 8191, 8192, 20_010])
    np.testing.assert_array_equal(po.philox_keys_at(idx, seed, offset), words[idx] >> 1)
    keys = (words >> 1).astype(np.uint32)
    k = 2000
    t = po.threshold(keys, k)
    c = po.comps(keys)
    lower = np.partition(c, n - k - 300)[n - k - 300]          # 300 entries of slack
    listed = np.nonzero(c >= lower)[0]
    g = np.random.default_rng(1).standard_normal(n).astype(np.float32)
    f = po.build_idxval(n, listed, g[listed], thresh=t, lower=lower, codec=po.CODEC_RAND,
                        key_mode=po.KEY_PHILOX, k=k, seed=seed, offset=offset)
    want = np.zeros(n, dtype=np.float32)
    sel = po.selected_indices(keys, k)
    want[sel] = g[sel]
    assert listed.size == k + 300 and po.kept_entries(f)[0].size == k
    assert po.decode_packet(f).tobytes() == want.tobytes()


@pytest.mark.parametrize("fmt", ["idxval", "bitmap"])
def test_dropout_unbiased_scaling_and_p_zero(fmt):
    n = 9000
    idx = [0, 5, 8191, 8999]
    val = np.array([1.0, -3.0, NEG0, 1e-45], dtype=np.float32)
    for p in (0.3, 0.0):
        if fmt == "idxval":
            f = po.build_idxval(n, idx, val, thresh=0, codec=po.CODEC_DROPOUT_UNBIASED, p=p)
        else:
            f = po.build_bitmap(n, idx, val, codec=po.CODEC_DROPOUT_UNBIASED, p=p)
        o32, o64 = po.decode_packet(f, np.float32), po.decode_packet(f, np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            w64 = val.astype(np.float64) / np.float64(p)
        assert po.same_bits(o64[idx], w64)
        assert po.same_bits(o32[idx], w64.astype(np.float32))
        rest = np.ones(n, dtype=bool)
        rest[idx] = False
        if p == 0.0:
            assert np.all(np.isnan(o32[rest])) and np.all(np.isnan(o64[rest]))
            assert o32[0] == np.inf and o32[5] == -np.inf and np.isnan(o32[8191])
        else:
            assert not _bits(o32)[rest].any() and not _bits(o64)[rest].any()
            assert _bits(o32)[8191] == 0x80000000          # -0.0 / p stays -0.0
    # the biased codec stores the value itself
    fb = po.build_idxval(n, idx, val, thresh=0, codec=po.CODEC_DROPOUT_BIASED, p=0.3)
    assert po.decode_packet(fb)[idx].tobytes() == val.tobytes()


def test_fold_is_the_row_order_sum():
    n, M = 9000, 5
    rng = np.random.default_rng(3)
    pk, rows = [], []
    for m in range(M):
        idx = np.sort(rng.choice(n, 700, replace=False))
        val = rng.standard_normal(700).astype(np.float32)
        val[::50] = NEG0
        pk.append(po.build_idxval(n, idx, val, thresh=0, codec=po.CODEC_TOP, k=700))
        r = np.zeros(n, dtype=np.float32)
        r[idx] = val
        rows.append(r)
    w = np.array([0.5, -1.25, 0.0, -0.0, 3.0], dtype=np.float32)
    want = go.sequential_weighted_sum(rows, w)
    got = po.fold_packets(pk, w)
    assert got.tobytes() == want.tobytes()
    assert not (_bits(got) == 0x80000000).any()            # a +0-started sum is never -0
    # splitting the rows across two calls gives the same bits
    part = po.fold_packets(pk[:2], w[:2])
    assert po.fold_packets(pk[2:], w[2:], acc=part).tobytes() == want.tobytes()
    # a partial sum without -0.0 is the same as one more row of weight 1
    acc = rng.standard_normal(n).astype(np.float32)
    acc[::7] = 1e-42
    cont = po.fold_packets(pk, w, acc=acc)
    assert cont.tobytes() == go.sequential_weighted_sum([acc] + rows, [np.float32(1)] + list(w)).tobytes()
    # -0.0 in the partial sum stays -0.0 only under terms that are all -0.0
    accz = np.full(n, NEG0)
    neg = po.fold_packets(pk[:1], [np.float32(-1.0)], acc=accz)   # dropped: fl(+0 * -1) = -0
    pos = po.fold_packets(pk[:1], [np.float32(1.0)], acc=accz)    # dropped: +0 -> -0 + +0 = +0
    dropped = rows[0] == 0
    dropped[po.listed_entries(pk[0])[0]] = False
    assert np.all(_bits(neg)[dropped] == 0x80000000) and not _bits(pos)[dropped].any()
    # an inf weight poisons every coordinate its packet drops (fl(+0 * inf) = NaN)
    inf = po.fold_packets(pk[:2], [np.float32(1), np.float32(np.inf)])
    np.testing.assert_array_equal(np.isnan(inf), rows[1] == 0)
    assert np.all(np.isnan(po.fold_packets(pk[:2], [np.float32(1), np.float32(np.nan)])))


# ---- against the reference's goldens -------------------------------------------------------
@pytest.mark.parametrize("name", [c for c in G.cases("top__") if G.meta(c)["n"] <= 70_000])
def test_topk_packet_decodes_to_the_reference(name):
    m = G.meta(name)
    g = np.ascontiguousarray(G.input(name), dtype=np.float32)
    n = g.shape[0]
    k = co.effective_k(co.num_kept(m["fraction"], n), n)
    idx, val = po.topk_packet(g, k)
    t = po.threshold(po.mag_key(g), k)
    f = po.build_idxval(n, idx, val, thresh=t, lower=t, codec=po.CODEC_TOP, k=k)
    want = co.compress({"compression_function": "top", "fraction_coordinate": m["fraction"]}, g)
    assert po.decode_packet(f).tobytes() == want.tobytes()
    assert int(f["hdr"]["n_entries"]) == k == int(f["cnt"].sum())
    # with slack listed below T64 the decoder still keeps exactly the top k
    if 0 < k < n:
        c = po.comps(po.mag_key(g))
        extra = min(n - k, 5)
        lower = np.partition(c, n - k - extra)[n - k - extra]
        li = np.nonzero(c >= lower)[0]
        fs = po.build_idxval(n, li, g[li], thresh=t, lower=lower, codec=po.CODEC_TOP, k=k)
        assert po.decode_packet(fs).tobytes() == want.tobytes()
