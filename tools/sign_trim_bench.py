"""The coordinate-wise trimmed mean and median of scaled-sign packets (codec.trimmed_mean_sign)
against the only route there was before it, in one process.

    python tools/sign_trim_bench.py [--shapes 128x16777216:12,32x134217728:3]
                                    [--agg-shapes 32x25500000] [--f 0.1] [--out FILE]

Per shape M x N : b, once with trim = b and once with the median's (M - 1) // 2 (HIP events around
a whole call, the forms alternating over the rounds after a warm-up, the figure the median round
with min-max beside it), one JSON line:
(a) trim_sign   codec.trimmed_mean_sign(packets, trim)                (fc_sign_trim)
    trim_sign_entry   the entry point alone, the device view table already there (a call of 128
                packets through codec also pays the host's view table and its copy)
(b) dense_trim  the route it replaces: codec.decode_sign of every client into an (M, N) float32
                slab, torch.sort(dim=0), the slice [trim, M - trim), a sequential float32 sum in
                ascending order from +0.0 and one float32 division
(c) vote_sign / fold_sign   the other two consumers on the same packets, for context
(d) top_trim    codec.trimmed_mean on the same clients' 'top' packets at f, for context
Checked once per line: (a) and (b) give the same bits (NaN positions as NaN).  Bytes: (a) reads
the words twice but for the last b clients of its second pass, (2 M - b) N / 8, and writes 4 N; it
walks 2 M - 2 b full steps and b counting steps per coordinate.  The dense route writes and
re-reads its 4 M N-byte slab, which alone takes 8 M N / 8 TB/s.
Aggregator part (--agg-shapes), one JSON line per shape:
(e) wall time of one round, host gradients in, host aggregate out, through "sign-trim"
    (trimmed_mean with trim_count = M // 10 and coordinate_median, "sign_trim": True) beside
    "sign" (fed_avg)
Needs a GPU: no fallback.
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

PEAK = 8e12                                           # bytes per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128x16777216:12,32x134217728:3")
    ap.add_argument("--agg-shapes", default="32x25500000")
    ap.add_argument("--f", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--agg-rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sign_trim_bench needs a GPU")
    from openmsftl_amd import _lib as L
    from openmsftl_amd import Compression, codec
    from openmsftl_amd.aggregation import Aggregator
    from openmsftl_amd.compression import kept_count
    lib = L.load()
    dev = torch.device("cuda", torch.cuda.current_device())

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def alternate(forms, rounds):
        """{name: (median us, [min, max])}: every form once per round, in turn."""
        for fn in forms.values():
            fn()
        torch.cuda.synchronize()
        t = {k: [] for k in forms}
        for _ in range(rounds):
            for k, fn in forms.items():
                t[k].append(timed(fn))
        return {k: (round(statistics.median(v), 1), [round(min(v), 1), round(max(v), 1)])
                for k, v in t.items()}

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")

    def same_bits(x, y):
        x, y = x.cpu().numpy(), y.cpu().numpy()
        xn, yn = np.isnan(x), np.isnan(y)
        return bool(np.array_equal(xn, yn) and np.array_equal(x.view(np.uint32)[~xn], y.view(np.uint32)[~yn]))

    for shape in [s for s in a.shapes.split(",") if s]:
        dims, b0 = shape.split(":")
        m, n = (int(x) for x in dims.split("x"))
        k = kept_count(a.f, n)
        gen = torch.Generator(device=dev).manual_seed(n % 1000 + 19)
        signs = [codec.SignPacket.alloc(n, dev) for _ in range(m)]
        tops = codec.Packet.alloc_batch(n, m, L.FC_FMT_IDXVAL, dev, k=k)
        base = torch.randn(n, device=dev, generator=gen)
        for s in range(0, m, 8):                         # a group at a time: 8 gradients live
            gs = [(base + torch.randn(n, device=dev, generator=gen)) * (1.0 + (s + i) / m)
                  for i in range(min(8, m - s))]
            for i, g in enumerate(gs):
                codec.encode_sign(g, packet=signs[s + i])
            codec.encode_top_batch(gs, k, packets=tops[s:s + len(gs)])
            for p in tops[s:s + len(gs)]:
                p.release()
            del gs
        codec.BatchWorkspace._cache.clear()
        del base
        torch.cuda.empty_cache()
        eta = float(np.median([h.p for h in codec.headers(signs)]))
        w = [1.0 / m] * m
        views = codec._sign_views(signs, [1.0] * m, dev)
        ws = codec.SignTrimWorkspace.get(n, m, dev) if lib.fc_sign_trim_workspace_bytes(n, m) else None
        slab = torch.empty((m, n), dtype=torch.float32, device=dev)
        out_s = torch.empty(n, dtype=torch.float32, device=dev)
        out_t = torch.empty(n, dtype=torch.float32, device=dev)
        out_v = torch.empty(n, dtype=torch.float32, device=dev)
        out_f = torch.empty(n, dtype=torch.float32, device=dev)

        for trim in (int(b0), (m - 1) // 2):
            def dense_trim():
                for i, p in enumerate(signs):
                    codec.decode_sign(p, out=slab[i])
                kept = torch.sort(slab, dim=0).values[trim:m - trim]
                acc = torch.zeros(n, dtype=torch.float32, device=dev)
                for row in kept:                             # ascending, one float32 add per row
                    acc.add_(row)
                return codec.div_scalar(acc, float(m - 2 * trim))

            def entry():                                     # fc_sign_trim alone: the views are there
                L.check(lib.fc_sign_trim(codec._vp(views), m, n, trim, codec._vp(out_s),
                                         codec._vp(ws.buf if ws else None), ws.nbytes if ws else 0,
                                         codec._stream(dev)), "fc_sign_trim")

            codec.trimmed_mean_sign(signs, trim, out=out_s)
            same = same_bits(out_s, dense_trim())
            t = alternate({"trim_sign": lambda: codec.trimmed_mean_sign(signs, trim, out=out_s),
                           "trim_sign_entry": entry,
                           "dense_trim": dense_trim,
                           "vote_sign": lambda: codec.vote_sign(signs, eta, out=out_v),
                           "fold_sign": lambda: codec.fold_sign(signs, w, out=out_f),
                           "top_trim": lambda: codec.trimmed_mean(tops, trim, out=out_t)}, a.rounds)
            torch.cuda.empty_cache()
            emit({"bench": "sign_trim_bench", "M": m, "N": n, "trim": trim,
                  "median": trim == (m - 1) // 2, "f": a.f, "rounds": a.rounds,
                  "us": {k_: x[0] for k_, x in t.items()},
                  "minmax": {k_: x[1] for k_, x in t.items()},
                  "trim_sign_equals_dense_bits": same,
                  "speedup": {"trim_sign_vs_dense": round(t["dense_trim"][0] / t["trim_sign"][0], 1),
                              "trim_sign_vs_top_trim": round(t["top_trim"][0] / t["trim_sign"][0], 2)},
                  "ratio": {"trim_sign_over_fold_sign": round(t["trim_sign"][0] / t["fold_sign"][0], 2),
                            "trim_sign_over_vote_sign": round(t["trim_sign"][0] / t["vote_sign"][0], 2)},
                  "trim_sign_bytes": (2 * m - trim) * n // 8 + 4 * n,
                  "entry_model_frac_of_8TBs": round(((2 * m - trim) * n / 8 + 4 * n) / PEAK * 1e6
                                                    / t["trim_sign_entry"][0], 3),
                  "entry_full_steps_per_us": round((2 * m - 2 * trim) * n / t["trim_sign_entry"][0]),
                  "dense_slab_floor_us": round(8 * m * n / PEAK * 1e6, 1),
                  "trim_sign_below_dense_slab_floor": bool(t["trim_sign"][0] < 8 * m * n / PEAK * 1e6)})
        del signs, tops, slab
        torch.cuda.empty_cache()

    # ---- (e) one Aggregator round ----
    for shape in [s for s in a.agg_shapes.split(",") if s]:
        m, n = (int(x) for x in shape.split("x"))
        base = np.random.default_rng(3).standard_normal(n).astype(np.float32)
        grads = [np.roll(base, 1009 * i) * np.float32(1.0 + i / m) for i in range(m)]

        def clients():
            return [types.SimpleNamespace(C=Compression({"compression_function": "sign"}), grad=x, client_id=i)
                    for i, x in enumerate(grads)]

        res = {}
        for name, path, cfg in (("fed_avg", "sign", {}),
                                ("trimmed_mean", "sign-trim", {"sign_trim": True, "trim_count": m // 10}),
                                ("coordinate_median", "sign-trim", {"sign_trim": True})):
            ag = Aggregator(dict({"aggregation_scheme": name}, **cfg))
            ts = []
            for _ in range(a.agg_rounds + 1):            # the first round warms up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ag.aggregate_grads(clients())
                ts.append(time.perf_counter() - t0)
            assert ag.agg_path == path, ag.agg_path
            res[name] = {"agg_path": path, "ms": round(statistics.median(ts[1:]) * 1e3, 1),
                         "minmax_ms": [round(min(ts[1:]) * 1e3, 1), round(max(ts[1:]) * 1e3, 1)]}
        emit({"bench": "sign_trim_bench_aggregator", "M": m, "N": n, "rounds": a.agg_rounds, "routes": res})


if __name__ == "__main__":
    main()
