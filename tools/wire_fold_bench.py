"""The FedAVG fold straight from wire packets against the route there was before it, and a whole
round from host payloads with and without ``"wire_fold"``.  HIP-event timed.

    python tools/wire_fold_bench.py [--shapes 128x16777216,32x134217728] [--f 0.1] [--out FILE]
                                    [--round 32x25500000] [--rounds 7]

Per shape (top-k packets of normal gradients from codec.encode_top_batch, packed with codec.pack),
after first checking that all three forms give the same bits:
(a) wire_fold      fc_wire_fold on prebuilt tables: one launch, each packet's bytes read once
(b) unpack+fold    fc_wire_unpack_batch into slotted packets, then fc_decode_accumulate on them:
                   the only route before (a)
(c) slotted_fold   fc_decode_accumulate alone on the already-unpacked packets: the slotted fold's
                   own rate
Bytes are algorithmic: (a) reads m (6E + 12 nch + 128) and writes 4n; (b) additionally writes and
re-reads m (6E + 12 nch + 96).
One process; after a warm-up the forms alternate over the rounds; median and min-max.

A round (--round MxN): Aggregator.aggregate_wire on M host payloads (Compression.compress_wire's
bytes), fed_avg, with and without ``"wire_fold": True``: host wall time to the host aggregate, the
number of groups each run used under the default budget, then the stages one by one: validation
(host clock), H2D, the device part of each route (events), the aggregate's D2H (host clock).
One JSON line.  Needs a GPU: no fallback.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128x16777216,32x134217728")
    ap.add_argument("--round", default="32x25500000")
    ap.add_argument("--f", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("wire_fold_bench needs a GPU")
    from openmsftl_amd import _lib as L
    from openmsftl_amd import aggregation, codec
    from openmsftl_amd.compression import Compression, kept_count
    lib = L.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    FMT = L.FC_FMT_IDXVAL

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3, out

    def stats(x):
        return {"us": round(statistics.median(x), 1), "minmax": [round(min(x), 1), round(max(x), 1)]}

    def encode(n, m, k):
        packets = codec.Packet.alloc_batch(n, m, FMT, dev, k=k)
        gen = torch.Generator(device=dev).manual_seed(n % 1000 + 7)
        for s in range(0, m, 8):                         # encode a group at a time: 8 gradients live
            gs = [torch.randn(n, device=dev, generator=gen) for _ in range(min(8, m - s))]
            codec.encode_top_batch(gs, k, packets=packets[s:s + len(gs)])
            for p in packets[s:s + len(gs)]:
                p.release()
            del gs
        codec.BatchWorkspace._cache.clear()
        torch.cuda.empty_cache()
        return packets

    def same(x, y):
        return bool(torch.equal(x.view(torch.int32), y.view(torch.int32)))

    res = {"bench": "wire_fold_bench", "f": a.f, "rounds": a.rounds, "shapes": []}
    for shape in [s for s in a.shapes.split(",") if s]:
        m, n = (int(x) for x in shape.split("x"))
        k = kept_count(a.f, n)
        nch = int(lib.fc_num_chunks(n))
        packets = encode(n, m, k)
        wires = codec.pack(packets)
        del packets                                      # one slotted set at a time
        codec.WireWorkspace._cache.clear()
        torch.cuda.empty_cache()
        w = [float(np.float32(1.0 / m))] * m
        wts = torch.from_numpy(np.asarray(w, dtype=np.float32)).to(dev)
        jobs = codec._wire_jobs([x.buf for x in wires], [x.nbytes for x in wires], dev)
        dst = codec.Packet.alloc_batch(n, m, FMT, dev)
        dviews = codec.views_tensor(dst, w, dev)
        outs = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3)]
        stream = codec._stream(dev)

        def wire_fold():
            L.check(lib.fc_wire_fold(codec._vp(jobs), codec._vp(wts), m, n, codec._vp(outs[0]), 0, stream),
                    "fc_wire_fold")

        def unpack_fold():
            L.check(lib.fc_wire_unpack_batch(codec._vp(jobs), codec._vp(dviews), m, n, stream),
                    "fc_wire_unpack_batch")
            L.check(lib.fc_decode_accumulate(codec._vp(dviews), m, FMT, n, codec._vp(outs[1]), stream),
                    "fc_decode_accumulate")

        def slotted_fold():
            L.check(lib.fc_decode_accumulate(codec._vp(dviews), m, FMT, n, codec._vp(outs[2]), stream),
                    "fc_decode_accumulate")

        forms = (wire_fold, unpack_fold, slotted_fold)
        for fn in forms:                                 # the check, and the warm-up
            fn()
        torch.cuda.synchronize()
        equal = same(outs[0], outs[1]) and same(outs[0], outs[2])
        if not equal:
            raise SystemExit(f"{shape}: the three forms do not give the same bits")
        t = [[] for _ in forms]
        for _ in range(a.rounds):                        # alternate: all see the same neighbours
            for i, fn in enumerate(forms):
                us, _ = timed(fn)
                t[i].append(us)
        first = outs[0].clone()
        wire_fold()
        torch.cuda.synchronize()
        wire_total = sum(x.nbytes for x in wires)
        a_bytes = wire_total + 4 * n
        b_bytes = a_bytes + 2 * (6 * m * k + 12 * nch * m + 96 * m)
        med = [statistics.median(x) for x in t]
        res["shapes"].append({
            "m": m, "n": n, "k": k, "wire_bytes_total": wire_total,
            "slotted_bytes_per_packet": 6 * nch * L.FC_CHUNK + 12 * nch + 96,
            "wire_fold": stats(t[0]), "unpack_then_fold": stats(t[1]), "slotted_fold": stats(t[2]),
            "ratio_unpack_then_fold_over_wire_fold": round(med[1] / med[0], 2),
            "ratio_wire_fold_over_slotted_fold": round(med[0] / med[2], 3),
            "wire_fold_algorithmic_bytes": a_bytes, "wire_fold_TBps": round(a_bytes / med[0] / 1e6, 3),
            "unpack_then_fold_algorithmic_bytes": b_bytes,
            "same_bits_three_forms": equal, "same_bits_twice": same(first, outs[0]),
        })
        del wires, dst, dviews, jobs, outs, first
        torch.cuda.empty_cache()

    if a.round:
        from openmsftl_amd.aggregation import Aggregator
        m, n = (int(x) for x in a.round.split("x"))
        k = kept_count(a.f, n)
        rng = np.random.default_rng(5)
        cfg = {"compression_function": "top", "fraction_coordinate": a.f}
        payloads = []                                    # the clients' side: not timed
        for i in range(m):
            payloads.append(Compression(dict(cfg)).compress_wire(rng.standard_normal(n, dtype=np.float32)))
        agg_u = Aggregator({"aggregation_scheme": "fed_avg"})
        agg_f = Aggregator({"aggregation_scheme": "fed_avg", "wire_fold": True})

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        forms = (lambda: agg_f.aggregate_wire(payloads), lambda: agg_u.aggregate_wire(payloads))
        for fn in forms:
            fn()
        equal = agg_f.agg_grad.tobytes() == agg_u.agg_grad.tobytes()
        paths = [agg_f.agg_path, agg_u.agg_path]
        budget = aggregation._budget(agg_f, dev)
        sizes = [len(p) for p in payloads]
        groups_f = len(aggregation.wire_fold_groups(sizes, n, budget))
        per = aggregation.wire_group(agg_u, n, m, dev)
        groups_u = (m + per - 1) // per
        tw = [[], []]
        for _ in range(a.rounds):
            for i, fn in enumerate(forms):
                tw[i].append(wall(fn))
        # the stages, one by one
        tv, th, tf, tu, td = [], [], [], [], []
        arrs = [np.frombuffer(p, dtype=np.uint8) for p in payloads]
        offs = np.concatenate([[0], np.cumsum([(x.size + 255) & ~255 for x in arrs])])
        slab = torch.empty(int(offs[-1]), dtype=torch.uint8, device=dev)
        pk = codec.Packet.alloc_batch(n, m, FMT, dev)
        out = torch.empty(n, dtype=torch.float32, device=dev)
        w = [float(np.float32(1.0 / m))] * m
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            for x in arrs:
                assert lib.fc_wire_validate(ctypes.c_void_p(x.ctypes.data), x.size, n) == 0
            tv.append((time.perf_counter() - t0) * 1e3)
            us, wires = timed(lambda: [codec.TOP.upload(x, L.WireHdr.from_buffer_copy(x[:128].tobytes()), dev,
                                                          out=slab[int(o): int(o) + x.size])
                                       for x, o in zip(arrs, offs)])
            th.append(us / 1e3)
            us, _ = timed(lambda: codec.fold_wire(wires, w, out=out))
            tf.append(us / 1e3)
            us, _ = timed(lambda: codec.decode_accumulate(codec.unpack(wires, pk), w, out=out))
            tu.append(us / 1e3)
            td.append(wall(lambda: out.cpu().numpy()))
            del wires

        def ms(x):
            return {"ms": round(statistics.median(x), 2), "minmax": [round(min(x), 2), round(max(x), 2)]}

        mf, mu = statistics.median(tw[0]), statistics.median(tw[1])
        res["round"] = {
            "m": m, "n": n, "k": k, "payload_bytes": sum(sizes), "budget_bytes": int(budget),
            "aggregate_wire_fold": ms(tw[0]), "aggregate_wire_unpack": ms(tw[1]),
            "ratio_unpack_over_fold": round(mu / mf, 3), "agg_paths": paths,
            "groups_wire_fold": groups_f, "groups_unpack": groups_u, "same_aggregate_bits": bool(equal),
            "stages": {"validate_host": ms(tv), "h2d_pageable": ms(th), "device_wire_fold": ms(tf),
                       "device_unpack_then_fold": ms(tu), "d2h_aggregate": ms(td)},
            "device_fraction_of_round_wire_fold": round(statistics.median(tf) / mf, 4),
            "device_fraction_of_round_unpack": round(statistics.median(tu) / mu, 4),
        }
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
