"""fc_packets_trim against the only route there was before it and against the FedAVG fold, and
one Aggregator round of each coordinate-wise scheme beside the pc_analysis "gram" round.

    python tools/trim_bench.py [--shapes 128x16777216,32x134217728] [--f 0.1] [--out FILE]

Kernel part, per shape (HIP events, one process, the forms alternating over the rounds after a
warm-up, the figure the median round, min-max beside it):
(a) trim    codec.trimmed_mean(packets, int(0.1 * M))             (fc_packets_trim)
(a') median codec.trimmed_mean(packets, (M - 1) // 2)
(b) dense   what a caller could do without the kernel: codec.decode of every packet into a row of
            an (M, N) float32 slab, torch.sort(dim=0), the slice and its sum, the division.  The
            slab and the sort's values and indices are what it holds: their bytes are reported
(c) fold    codec.decode_accumulate on the same packets: the floor, the same gather of the
            entries and the same 4N-byte write
M is cut to what fits beside (b)'s slab and sort (``m_cut``).  Checked once per shape: (a) equals,
bit for bit, the trimmed mean made of (b)'s sorted slab in the definition's order (rows b .. M-b-1
added one by one in float32 from +0.0, then a float32 division by a tensor, which torch does not
turn into a multiplication).  model_bytes: 8 bytes per kept entry and 4N for the aggregate, as a
fraction of 8 TB/s.
Aggregator part (--agg-shapes, default 32x25500000): wall time of aggregate_grads, host
gradients in, host aggregate out, for fed_avg + pc_analysis "gram", trimmed_mean and
coordinate_median; the upload and the batched encode are the same in every form.
One JSON line per shape.  Needs a GPU: no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128x16777216,32x134217728")
    ap.add_argument("--agg-shapes", default="32x25500000")
    ap.add_argument("--f", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--dense-rounds", type=int, default=3)
    ap.add_argument("--agg-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("trim_bench needs a GPU")
    from openmsftl_amd import _lib as L
    from openmsftl_amd import Compression, codec
    from openmsftl_amd.aggregation import Aggregator
    from openmsftl_amd.compression import kept_count
    from openmsftl_amd.pipeline import packet_bytes
    dev = torch.device("cuda", torch.cuda.current_device())

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3, out

    res = {"bench": "trim_bench", "f": a.f, "shapes": [], "aggregator": []}
    for shape in [s for s in a.shapes.split(",") if s]:
        m_asked, n = (int(x) for x in shape.split("x"))
        k = kept_count(a.f, n)
        # (b) holds the slab, the sorted slab and the sort's int64 indices, plus a transient
        per_client = packet_bytes(n) + 4 * n * 2 + 8 * n + 4 * n
        free = int(torch.cuda.mem_get_info(dev)[0] * 0.85) - 16 * n - 8 * 4 * n
        m = max(1, min(m_asked, free // per_client))
        packets = codec.Packet.alloc_batch(n, m, L.FC_FMT_IDXVAL, dev, k=k)
        gen = torch.Generator(device=dev).manual_seed(n % 1000 + 7)
        for s in range(0, m, 8):                         # encode a group at a time: 8 gradients live
            gs = [torch.randn(n, device=dev, generator=gen) for _ in range(min(8, m - s))]
            codec.encode_top_batch(gs, k, packets=packets[s:s + len(gs)])
            for p in packets[s:s + len(gs)]:
                p.release()
            del gs
        codec.BatchWorkspace._cache.clear()
        torch.cuda.empty_cache()
        b_trim, b_med = int(0.1 * m), (m - 1) // 2
        out_t = torch.empty(n, dtype=torch.float32, device=dev)
        out_m = torch.empty(n, dtype=torch.float32, device=dev)
        out_f = torch.empty(n, dtype=torch.float32, device=dev)
        slab = torch.empty((m, n), dtype=torch.float32, device=dev)
        weights = [1.0 / m] * m
        kept = {}

        def trim():
            return codec.trimmed_mean(packets, b_trim, out=out_t)

        def median():
            return codec.trimmed_mean(packets, b_med, out=out_m)

        def fold():
            return codec.decode_accumulate(packets, weights, out=out_f)

        def dense():
            for i, p in enumerate(packets):
                codec.decode(p, out=slab[i])
            srt = torch.sort(slab, dim=0).values
            kept["sorted"] = srt
            return srt[b_trim:m - b_trim].sum(dim=0) / float(m - 2 * b_trim)

        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        dense()                                          # warm-up, and the check's sorted slab
        torch.cuda.synchronize()
        dense_peak = torch.cuda.max_memory_allocated(dev) - before + slab.numel() * 4
        srt = kept.pop("sorted")
        same = {}
        for name, fn, b in (("trim", trim, b_trim), ("median", median, b_med)):
            acc = torch.zeros(n, dtype=torch.float32, device=dev)
            for r in range(b, m - b):
                acc = acc + srt[r]
            want = acc / torch.tensor([float(m - 2 * b)], dtype=torch.float32, device=dev)
            got = fn()
            same[name] = bool(torch.equal(got.view(torch.int32), want.view(torch.int32)))
            del acc, want
        del srt
        torch.cuda.empty_cache()
        forms = (trim, median, fold, dense)
        for fn in forms[:3]:                             # warm-up: code objects, workspaces
            fn()
        torch.cuda.synchronize()
        t = [[] for _ in forms]
        for r in range(a.rounds):                        # alternate: all see the same neighbours
            for i, fn in enumerate(forms):
                if fn is dense and r >= a.dense_rounds:
                    continue
                us, _ = timed(fn)
                kept.clear()
                t[i].append(us)
        again = trim().clone()
        med = [statistics.median(x) for x in t]
        mm = [[round(min(x), 1), round(max(x), 1)] for x in t]
        entries = sum(int(h.k) for h in codec.headers(packets))
        model = 8 * entries + 4 * n
        res["shapes"].append({
            "m_asked": m_asked, "m": m, "m_cut": m != m_asked, "n": n, "k": k,
            "trim": b_trim, "median_trim": b_med, "kept_entries_total": entries,
            "trim_us": round(med[0], 1), "trim_us_minmax": mm[0],
            "median_us": round(med[1], 1), "median_us_minmax": mm[1],
            "fold_us": round(med[2], 1), "fold_us_minmax": mm[2],
            "dense_us": round(med[3], 1), "dense_us_minmax": mm[3], "dense_rounds": len(t[3]),
            "ratio_dense_over_trim": round(med[3] / med[0], 2),
            "ratio_trim_over_fold": round(med[0] / med[2], 2),
            "ratio_median_over_fold": round(med[1] / med[2], 2),
            "model_bytes": model,
            "model_fraction_of_8TBps": round(model / (med[0] * 1e-6) / 8e12, 4),
            "dense_slab_bytes": 4 * m * n, "dense_peak_bytes": int(dense_peak),
            "trim_equals_sorted_slab": same["trim"], "median_equals_sorted_slab": same["median"],
            "same_bits_twice": bool(torch.equal(again.view(torch.int32), out_t.view(torch.int32))),
            "trim_workspace_bytes": int(L.load().fc_trim_workspace_bytes(n, m)),
        })
        del packets, slab, out_t, out_m, out_f, again
        torch.cuda.empty_cache()

    top = {"compression_function": "top", "fraction_coordinate": a.f}
    forms = [("fed_avg+gram", {"aggregation_scheme": "fed_avg", "pc_analysis": "gram"}),
             ("trimmed_mean", {"aggregation_scheme": "trimmed_mean"}),
             ("coordinate_median", {"aggregation_scheme": "coordinate_median"})]
    for shape in [s for s in (a.agg_shapes or "").split(",") if s]:
        m, n = (int(x) for x in shape.split("x"))
        rng = np.random.default_rng(n % 1000 + 11)
        bases = [rng.standard_normal(n, dtype=np.float32) for _ in range(min(8, m))]
        clients = [types.SimpleNamespace(C=Compression(dict(top)), client_id=i,
                                         grad=np.roll(bases[i % 8], 1000003 * (i // 8)))
                   for i in range(m)]
        aggs = []
        for name, cfg in forms:
            cfg = dict(cfg, device_budget_bytes=int(torch.cuda.mem_get_info(dev)[0] * 0.8))
            aggs.append((name, Aggregator(cfg, device=dev)))
        t = {name: [] for name, _ in forms}
        for r in range(a.agg_rounds + 1):                # round 0 warms up
            for name, ag in aggs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ag.aggregate_grads(clients)
                torch.cuda.synchronize()
                ag.__dict__.pop("_gram_packets", None)   # one form's packets resident at a time
                if r:
                    t[name].append((time.perf_counter() - t0) * 1e3)
        base = statistics.median(t["fed_avg+gram"])
        entry = {"m": m, "n": n, "rounds": a.agg_rounds}
        for name, ag in aggs:
            entry[name + "_ms"] = round(statistics.median(t[name]), 2)
            entry[name + "_ms_minmax"] = [round(min(t[name]), 2), round(max(t[name]), 2)]
            entry[name + "_minus_gram_ms"] = round(statistics.median(t[name]) - base, 2)
            entry[name + "_path"] = ag.agg_path
        res["aggregator"].append(entry)
        del aggs, clients, bases
        torch.cuda.empty_cache()
    lines = [json.dumps(dict({"bench": "trim_bench", "part": "kernel", "f": a.f}, **e)) for e in res["shapes"]]
    lines += [json.dumps(dict({"bench": "trim_bench", "part": "aggregator", "f": a.f}, **e))
              for e in res["aggregator"]]
    for line in lines:
        print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
