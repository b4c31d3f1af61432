"""fc_packets_dot against the only route there was before it, and one Aggregator round of each
linear rule against the pc_analysis "gram" round, HIP-event / wall timed.

    python tools/dot_bench.py [--shapes 128x16777216,32x134217728] [--f 0.1] [--out FILE]

Kernel part, per shape (HIP events, one process, the forms alternating over the rounds after a
warm-up, the figure the median round):
(a) dot     codec.dot_dense(packets, v)                           (fc_packets_dot, v dense)
(b) ones    codec.dot_dense(packets, None)                        (row sums, no image)
(a') call   fc_packets_dot alone, the views table already on the device (codec.dot_dense builds
            and uploads it on every call, as codec.gram does), with v and with NULL
(c) dense   codec.decode of every packet into one dense float32 row, then torch.dot(row.double(),
            v.double()) — what a caller could do without the kernel (v.double() made once,
            outside the timing)
max_rel_diff: the largest |a_i - c_i| / (|d_i| |v|) between the two results.
Aggregator part, per shape (wall time of aggregate_grads, host gradients in, host aggregate out;
the upload, the batched encode, the Gram and the fold are the same in every form, so the
difference to the "gram" FedAvg round is the rule's own cost; the forms alternate, and every
round allocates its packets anew so that only one form's are resident): fed_avg + pc_analysis "gram",
spectral_gram (adaptive_rank_th 0.95), geometric_median, centered_clip (second round: a carried
vector).  One JSON line.  Needs a GPU: no fallback.
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
    ap.add_argument("--agg-shapes", default=None, help="default: the kernel shapes")
    ap.add_argument("--f", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--agg-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dot_bench needs a GPU")
    from openmsftl_amd import _lib as L
    from openmsftl_amd import Compression, codec
    from openmsftl_amd.aggregation import Aggregator
    from openmsftl_amd.compression import kept_count
    dev = torch.device("cuda", torch.cuda.current_device())

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3, out

    res = {"bench": "dot_bench", "f": a.f, "shapes": [], "aggregator": []}
    for shape in a.shapes.split(","):
        m, n = (int(x) for x in shape.split("x"))
        k = kept_count(a.f, n)
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
        v = torch.randn(n, device=dev, generator=gen)
        v64 = v.double()
        out_a = torch.empty(m + 1, dtype=torch.float64, device=dev)
        out_b = torch.empty(m + 1, dtype=torch.float64, device=dev)
        row = torch.empty(n, dtype=torch.float32, device=dev)

        def dot():
            return codec.dot_dense(packets, v, out=out_a)

        def ones():
            return codec.dot_dense(packets, None, out=out_b)

        def dense():
            out = torch.empty(m + 1, dtype=torch.float64, device=dev)
            for i, p in enumerate(packets):
                codec.decode(p, out=row)
                out[i] = torch.dot(row.double(), v64)
            out[m] = torch.dot(v64, v64)
            return out

        views = codec.views_tensor(packets, [1.0] * m, dev)
        ws = codec.DotWorkspace.get(n, m, dev)
        lib, out_c = L.load(), torch.empty(m + 1, dtype=torch.float64, device=dev)

        def call(vec):
            L.check(lib.fc_packets_dot(codec._vp(views), m, n, codec._vp(vec), codec._vp(out_c),
                                       codec._vp(ws.buf), ws.nbytes, codec._stream(dev)), "fc_packets_dot")
            return out_c

        forms = (dot, ones, dense, lambda: call(v), lambda: call(None))
        for fn in forms:                                 # warm-up: code objects, workspaces
            fn()
        torch.cuda.synchronize()
        t = [[] for _ in forms]
        outs = [None] * len(forms)
        for _ in range(a.rounds):                        # alternate: all see the same neighbours
            for i, fn in enumerate(forms):
                us, o = timed(fn)
                outs[i] = o.clone()
                t[i].append(us)
        again = dot().clone()
        norms = torch.sqrt(codec.gram(packets).diagonal()) * torch.sqrt(outs[0][m])
        rel = float(((outs[0][:m] - outs[2][:m]).abs() / norms).max())
        med = [statistics.median(x) for x in t]
        entries = sum(int(h.n_entries) for h in codec.headers(packets))
        res["shapes"].append({
            "m": m, "n": n, "k": k, "n_entries_total": entries,
            "dot_us": round(med[0], 1), "ones_us": round(med[1], 1), "dense_us": round(med[2], 1),
            "dot_call_us": round(med[3], 1), "ones_call_us": round(med[4], 1),
            "dot_call_us_minmax": [round(min(t[3]), 1), round(max(t[3]), 1)],
            "ones_call_us_minmax": [round(min(t[4]), 1), round(max(t[4]), 1)],
            "dot_us_minmax": [round(min(t[0]), 1), round(max(t[0]), 1)],
            "ones_us_minmax": [round(min(t[1]), 1), round(max(t[1]), 1)],
            "dense_us_minmax": [round(min(t[2]), 1), round(max(t[2]), 1)],
            "ratio_dense_over_dot": round(med[2] / med[0], 3),
            "model_bytes": 6 * entries + 4 * n * ((m + 63) // 64),
            "model_GBps_dot_call": round((6 * entries + 4 * n * ((m + 63) // 64)) / (med[3] * 1e-6) / 1e9, 1),
            "model_GBps_ones_call": round(6 * entries / (med[4] * 1e-6) / 1e9, 1),
            "max_rel_diff": rel,
            "v_sq_rel_diff": float((outs[0][m] - outs[2][m]).abs() / outs[2][m]),
            "same_bits_twice": bool(torch.equal(again.view(torch.int64), outs[0].view(torch.int64))),
            "dot_workspace_bytes": int(L.load().fc_dot_workspace_bytes(n, m)),
        })
        del packets, row, v, v64, outs, views, ws
        codec.GramWorkspace._cache.clear()
        codec.DotWorkspace._cache.clear()
        torch.cuda.empty_cache()

    top = {"compression_function": "top", "fraction_coordinate": a.f}
    forms = [("fed_avg+gram", {"aggregation_scheme": "fed_avg", "pc_analysis": "gram"}),
             ("spectral_gram", {"aggregation_scheme": "spectral_gram", "adaptive_rank_th": 0.95}),
             ("geometric_median", {"aggregation_scheme": "geometric_median"}),
             ("centered_clip", {"aggregation_scheme": "centered_clip", "cclip_tau": 1.0})]
    for shape in (a.agg_shapes or a.shapes).split(","):
        m, n = (int(x) for x in shape.split("x"))
        rng = np.random.default_rng(n % 1000 + 11)
        bases = [rng.standard_normal(n, dtype=np.float32) for _ in range(min(8, m))]
        clients = [types.SimpleNamespace(C=Compression(dict(top)), client_id=i,
                                         grad=np.roll(bases[i % 8], 1000003 * (i // 8)))
                   for i in range(m)]
        tau = 0.5 * float(np.sqrt(a.f * n))              # about half a row's norm: clients are clipped
        aggs = []
        for name, cfg in forms:
            cfg = dict(cfg, device_budget_bytes=int(torch.cuda.mem_get_info(dev)[0] * 0.8))
            if "cclip_tau" in cfg:
                cfg["cclip_tau"] = tau
            aggs.append((name, Aggregator(cfg, device=dev)))
        t = {name: [] for name, _ in forms}
        for r in range(a.agg_rounds + 1):                # round 0 warms up (and gives clip its v)
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
        entry["geometric_median_iterations"] = int(aggs[2][1].gar.iterations)
        entry["centered_clip_carry"] = float(aggs[3][1].gar.carry)
        res["aggregator"].append(entry)
        del aggs, clients, bases
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
