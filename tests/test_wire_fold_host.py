"""fc_wire_fold's argument checks, aggregation.wire_fold_groups and codec.fold_wire's argument
errors: everything of the wire fold that needs no GPU.

Run:  python -m pytest tests/test_wire_fold_host.py -m "not gpu" -q

The library loads without a GPU (tests/test_lib_abi.py); every call below must return before any
device work starts.
"""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from openmsftl_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


# ---- the C entry point ------------------------------------------------------------------------
def test_argument_errors_do_not_touch_gpu(lib):
    buf = ctypes.create_string_buffer(256)
    addr = (ctypes.addressof(buf) + 15) & ~15

    def call(jobs=addr, weights=addr, m=1, n=10, acc=addr, cont=0):
        rc = lib.fc_wire_fold(jobs, weights, m, n, acc, cont, None)
        return rc, lib.fc_last_error() or b""

    for kw, want in (({"jobs": None}, b"jobs_dev is NULL"), ({"weights": None}, b"weights_dev is NULL"),
                     ({"acc": None}, b"acc is NULL"),
                     ({"m": 0}, b"m=0 outside"), ({"m": 65536}, b"m=65536 outside"),
                     ({"n": 0}, b"n=0 outside"), ({"n": 2 ** 32}, b"n=4294967296 outside"),
                     ({"acc": addr + 4}, b"16-byte aligned")):
        for cont in (0, 1):
            rc, msg = call(cont=cont, **kw)
            assert rc == -1 and want in msg, (kw, rc, msg)


def test_the_header_declares_it_and_the_abi_version_stays(lib):
    from openmsftl_amd import _lib
    assert "fc_wire_fold" in _lib.SIGNATURES
    assert lib.fc_abi_version() == 4


# ---- wire_fold_groups -------------------------------------------------------------------------
def groups(sizes, n, budget):
    from openmsftl_amd.aggregation import wire_fold_groups
    return wire_fold_groups(sizes, n, budget)


def check_cover(gs, count):
    assert all(isinstance(g, range) and g.step == 1 and len(g) >= 1 for g in gs)
    assert [i for g in gs for i in g] == list(range(count))          # consecutive, each once


def test_one_group_when_everything_fits():
    n = 1000
    sizes = [256, 512, 768]
    gs = groups(sizes, n, 4 * n + 1536)
    assert gs == [range(0, 3)]
    assert groups(sizes, n, 1 << 40) == [range(0, 3)]
    assert groups([], n, 1 << 20) == []


def test_a_cut_exactly_at_the_budget_and_one_byte_under_it():
    n = 1000
    sizes = [512, 512, 512, 512]
    assert groups(sizes, n, 4 * n + 1024) == [range(0, 2), range(2, 4)]      # two fit exactly
    assert groups(sizes, n, 4 * n + 1023) == [range(0, 1), range(1, 2), range(2, 3), range(3, 4)]
    assert groups(sizes, n, 4 * n + 2048) == [range(0, 4)]
    assert groups(sizes, n, 4 * n + 2047) == [range(0, 3), range(3, 4)]


def test_each_size_is_rounded_up_to_256_bytes():
    n = 8
    # 257 bytes take 512 of the slab: two of them need 1024, not 514
    assert groups([257, 257], n, 4 * n + 1023) == [range(0, 1), range(1, 2)]
    assert groups([257, 257], n, 4 * n + 1024) == [range(0, 2)]
    assert groups([1, 256, 255], n, 4 * n + 768) == [range(0, 3)]
    assert groups([1, 256, 255], n, 4 * n + 767) == [range(0, 2), range(2, 3)]


def test_a_lone_oversized_payload_raises_naming_both_numbers():
    n = 1000
    with pytest.raises(NotImplementedError, match=r"payload 1 .*\(5024 > 5023 bytes\)"):
        groups([256, 1024, 256], n, 4 * n + 1023)
    with pytest.raises(NotImplementedError, match="aggregate_wire needs payload 0"):
        groups([256], n, 4 * n)                                      # no room beside the aggregate
    assert groups([256, 1024, 256], n, 4 * n + 1024) == [range(0, 1), range(1, 2), range(2, 3)]


def test_groups_are_consecutive_and_cover_every_payload_once():
    rng = np.random.default_rng(5)
    n = 4096
    for trial in range(20):
        sizes = rng.integers(128, 5000, size=int(rng.integers(1, 40))).tolist()
        room = int(rng.integers(5120, 30000))
        gs = groups(sizes, n, 4 * n + room)
        check_cover(gs, len(sizes))
        rounded = [(s + 255) & ~255 for s in sizes]
        for j, g in enumerate(gs):
            assert sum(rounded[i] for i in g) <= room
            if j + 1 < len(gs):                                      # greedy: the next one did not fit
                assert sum(rounded[i] for i in g) + rounded[g.stop] > room


def test_a_group_holds_at_most_65535_payloads():
    gs = groups([128] * 65537, 16, 1 << 40)
    assert gs == [range(0, 65535), range(65535, 65537)]


# ---- codec.fold_wire's argument errors that need no device ------------------------------------
def test_fold_wire_argument_errors_without_a_device(lib, monkeypatch):
    import torch
    from openmsftl_amd import codec

    def no_device(*a, **k):
        raise AssertionError("device work started")
    monkeypatch.setattr(lib, "fc_wire_fold", no_device, raising=False)
    monkeypatch.setattr(codec, "_wire_jobs", no_device)

    def wire(n):
        return codec.WirePacket(n=n, buf=torch.zeros(256, dtype=torch.uint8), nbytes=256)
    with pytest.raises(ValueError, match="no packets"):
        codec.fold_wire([], [])
    with pytest.raises(ValueError, match="share n"):
        codec.fold_wire([wire(100), wire(101)], [1.0, 1.0])
    with pytest.raises(ValueError, match="one weight per packet"):
        codec.fold_wire([wire(100), wire(100)], [1.0])
    with pytest.raises(ValueError, match="continue_sum needs the partial sum"):
        codec.fold_wire([wire(100)], [1.0], continue_sum=True)
    with pytest.raises(TypeError, match="out must be a CUDA"):
        codec.fold_wire([wire(100)], [1.0], out=torch.zeros(100))
    short = codec.WirePacket(n=100, buf=torch.zeros(256, dtype=torch.uint8), nbytes=257)
    with pytest.raises(ValueError, match="nbytes lies outside"):
        codec.fold_wire([short], [1.0], out=torch.zeros(100))
