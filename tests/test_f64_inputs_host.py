"""CPU proofs that the crafted float64 inputs of tests/f64_inputs.py have the properties the GPU
tests of tests/test_f64_gpu.py rely on: each test fails if its builder loses the property
(candidates over the slot, group <= 2048, cut inside the group, sample reads only zeros), so a
GPU test cannot pass by missing its branch of csrc/fc_f64.hip."""
import functools

import numpy as np
import pytest

import f64_inputs as fi
from oracle import compression_oracle as co
from test_f64_boundary import tie_at_cut64


@functools.lru_cache(maxsize=None)
def _overflow(edge):
    return fi.chunk_overflow(edge=edge)


@pytest.mark.parametrize("edge", [False, True])
def test_chunk_overflow_has_more_candidates_than_the_slot(edge):
    g, k = _overflow(edge)
    n = g.shape[0]
    assert n == (fi.N_FULL if edge else fi.N_STRAT) and k == co.num_kept(0.1, n)
    assert fi.plan_of(n, k)["full"] == edge
    t = fi.kth_key64(g, k)                                   # threshold, after the insertion
    thw = np.uint32(t >> np.uint64(32))
    same = fi.hi_word(g) == thw
    big = slice(fi.OVER_BIG * fi.CHUNK, (fi.OVER_BIG + 1) * fi.CHUNK)
    small = slice(fi.OVER_SMALL * fi.CHUNK, (fi.OVER_SMALL + 1) * fi.CHUNK)
    # every element with the threshold's high word has its key32: a candidate of any bracket
    assert thw <= fi.CLAMP_HW
    assert np.count_nonzero(same[big]) > fi.SLOT             # the slot overflows: rescanned from g
    assert 0 < np.count_nonzero(same[small]) <= fi.SLOT      # a second chunk that does not
    assert np.count_nonzero(same) < fi.SMALL_CAP             # bin beta can be sorted: no RETRY
    assert not tie_at_cut64(g, k)
    # the cut is inside the cluster: members on both sides, in the overflowed chunk too
    above = fi.key64(g) >= t
    assert 0 < np.count_nonzero(same[big] & above[big]) < np.count_nonzero(same[big])
    # every two members within a relative 2^-21
    mags = np.abs(g[same])
    assert mags.max() / mags.min() - 1.0 <= 2.0 ** -21
    if edge:
        assert thw == 0x3FEFFFFF and (int(thw) + 1) % (1 << 19) == 0


@functools.lru_cache(maxsize=None)
def _tie(kept):
    return fi.tie_group(kept)


@pytest.mark.parametrize("kept", [1, 750, 1499])
def test_tie_group_straddles_the_cut(kept):
    g, k, grp = _tie(kept)
    n = g.shape[0]
    assert n == fi.N_STRAT and not fi.plan_of(n, k)["full"]
    v = np.abs(g[grp[0]])
    members = np.nonzero(np.abs(g) == v)[0]
    np.testing.assert_array_equal(members, grp)
    assert grp.shape[0] == fi.TIE_COUNT <= fi.SMALL_CAP
    assert (g[grp] > 0).any() and (g[grp] < 0).any()         # mixed signs
    per = np.bincount(grp // fi.CHUNK, minlength=n // fi.CHUNK + 1)
    assert per[fi.TIE_BIG] == 200 > fi.SLOT and np.delete(per, fi.TIE_BIG).max() <= 100
    above = int(np.count_nonzero(np.abs(g) > v))
    assert above < k < above + fi.TIE_COUNT and k - above == kept     # the cut is inside the group
    assert tie_at_cut64(g, k)
    # the oracle keeps the group's highest indices, bit copies of g
    q = fi.oracle_top(g, k)
    keep = np.zeros(n, bool)
    keep[np.abs(g) > v] = True
    keep[grp[fi.TIE_COUNT - kept:]] = True
    assert np.count_nonzero(keep) == k
    assert q.tobytes() == np.where(keep, g, 0.0).tobytes()


@functools.lru_cache(maxsize=None)
def _clamped(n):
    return fi.clamped(n)


@pytest.mark.parametrize("n", [100_003, (1 << 20) + 3])
def test_clamped_group_and_the_oracles_kept_sets(n):
    g, i_nan, i_inf, i_big = _clamped(n)
    group = np.concatenate([i_nan, i_inf, i_big])
    k32 = fi.key32(g)
    assert (k32[group] == fi.NAN_KEY32).all()                # one key32 for all 1500
    assert np.count_nonzero(k32 >= fi.CLAMP_HW) == 3 * fi.CLAMP_EACH <= fi.SMALL_CAP
    assert np.isnan(g[i_nan]).all() and np.isinf(g[i_inf]).all() and np.isfinite(g[i_big]).all()
    assert (np.abs(g[i_big]) >= 2.0 ** 1017).all() and np.unique(np.abs(g[i_big])).shape[0] == fi.CLAMP_EACH
    nb = fi.bits(g[i_nan])
    assert np.uint64(fi.NAN_INF_HW) in nb and np.uint64(fi.NAN_INF_HW | (1 << 63)) in nb
    assert np.uint32(0x7FF00000) in fi.hi_word(g[i_nan])     # a NaN with inf's high word
    assert (nb >> np.uint64(63)).min() == 0 and (nb >> np.uint64(63)).max() == 1
    assert (g[i_inf] > 0).any() and (g[i_inf] < 0).any()
    k64 = fi.key64(g)
    assert k64[i_nan].min() > k64[i_inf].max() == k64[i_inf].min() > k64[i_big].max()
    full = n <= fi.FULL_SAMPLE_MAX
    for k in fi.CLAMP_KS:
        P = fi.plan_of(n, k)
        assert P["full"] == full
        if not full:                        # make_plan's r_hi = floor(rho - m) < 1 up to k = 700
            assert P["hi_none"] == (k <= 700) and not P["lo_all"]
        kept = fi.clamped_expected_kept(g, k, i_nan, i_inf, i_big)
        assert kept.shape[0] == k
        keep = np.zeros(n, bool)
        keep[kept] = True
        q = fi.oracle_top(g, k)
        assert q.tobytes() == np.where(keep, g, 0.0).tobytes(), k
        t = fi.kth_key64(g, k)
        if k <= 3 * fi.CLAMP_EACH:          # the cut lands in the clamped key group
            assert np.uint32(t >> np.uint64(32)) > fi.CLAMP_HW
        else:                               # ... or just below all of it
            assert np.uint32(t >> np.uint64(32)) < fi.CLAMP_HW
    # where the cut falls among the members: NaN ties, inf ties, distinct giants
    assert tie_at_cut64(g, 250) and tie_at_cut64(g, 700)
    assert not tie_at_cut64(g, 1200) and not tie_at_cut64(g, 1499) and not tie_at_cut64(g, 1501)


def test_bracket_miss_sample_reads_only_zeros():
    g, k = fi.bracket_miss()
    n = g.shape[0]
    assert n == 4 << 20 and k == n // 10
    # the lone float64 encode plans with single = true: n / 32 / 1024 segments (the float32 test
    # test_top_bracket_miss_falls_back_to_exact restates the batched divisor 64)
    P = fi.plan_of(n, k)
    assert not P["full"] and P["nseg"] == 128 == n // 32 // 1024
    assert not P["hi_none"] and not P["lo_all"]
    m = fi.sampled_mask(n, k)
    assert np.count_nonzero(m) == 128 * 1024                 # disjoint segments
    assert m[:1024].all() and m[n - 1024:].all()             # the first and the last segment
    assert not g[m].any()                                    # the sample reads only zeros
    assert np.count_nonzero(g) == n // 8 > k                 # more than k above the bracket
    assert not tie_at_cut64(g, k)


@pytest.mark.parametrize("n", fi.SWEEP_N)
def test_sweep_inputs_and_plans(n):
    g = fi.sweep(n)
    assert g.shape == (n,) and g.dtype == np.float64 and np.isfinite(g).all()
    if n >= 8191:
        assert (np.signbit(g) & (g == 0)).any()              # -0.0
        tiny = np.abs(g[g != 0]).min()
        assert tiny < 2.3e-308 and tiny / 5e-324 == round(tiny / 5e-324)   # denormals
    ks = fi.sweep_ks(n)
    assert all(0 <= k <= n for k in ks)
    if n >= 3:
        assert 1 in ks and n - 1 in ks
    if n > fi.FULL_SAMPLE_MAX:              # the stratified plan's two one-sided brackets
        assert fi.plan_of(n, 1)["hi_none"] and not fi.plan_of(n, 1)["lo_all"]
        assert fi.plan_of(n, n - 1)["lo_all"] and not fi.plan_of(n, n - 1)["hi_none"]
        assert not fi.plan_of(n, co.num_kept(0.1, n))["hi_none"]
