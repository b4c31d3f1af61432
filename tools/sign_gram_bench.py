"""The geometry of scaled-sign packets (codec.gram_sign, codec.dot_sign) against the only routes
there were before them, in one process.

    python tools/sign_gram_bench.py [--shapes 128x16777216,32x134217728] [--agg-shapes 32x25500000]
                                    [--f 0.1] [--out FILE]

Per shape M x N (HIP events around a whole call, the forms alternating over the rounds after a
warm-up, the figure the median round with min-max beside it), one JSON line:
(a) gram        codec.gram_sign(packets)                              (fc_sign_gram)
(b) dense_gram  the route it replaces: codec.decode_sign of every client into an (M, N) float32
                slab, then G.double() @ G.double().T as gar.Krum.aggregate does, on the same packets
(c) top_gram    codec.gram on the same clients' 'top' packets at f, for context
(d) dot / dot_ones   codec.dot_sign with a dense vector and with v=None  (fc_sign_dot)
(e) dense_dot   the route it replaces: per packet codec.decode_sign into one row, then the float64
                dot of the row with v
Checked once per shape: gram_sign is symmetric bit for bit, equals the dense product within the
dense sum's rounding bound (rtol N 2^-52 of |s_i| |s_j| N), and dot_sign equals the dense dots
within the bound of a float64 sum.  Bytes: M N / 8 for the Gram, M N / 8 + 4 N for the dot; the
dense route writes and re-reads its 4 M N-byte slab, which alone takes 8 M N / 8 TB/s.
Aggregator part (--agg-shapes), one JSON line per shape:
(f) wall time of one round, host gradients in, host aggregate out, through "sign-gram" (krum and
    geometric_median with "sign_geometry": True) beside "sign" (fed_avg)
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
    ap.add_argument("--shapes", default="128x16777216,32x134217728")
    ap.add_argument("--agg-shapes", default="32x25500000")
    ap.add_argument("--f", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--agg-rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sign_gram_bench needs a GPU")
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

    for shape in [s for s in a.shapes.split(",") if s]:
        m, n = (int(x) for x in shape.split("x"))
        k = kept_count(a.f, n)
        gen = torch.Generator(device=dev).manual_seed(n % 1000 + 17)
        signs = [codec.SignPacket.alloc(n, dev) for _ in range(m)]
        tops = codec.Packet.alloc_batch(n, m, L.FC_FMT_IDXVAL, dev, k=k)
        base = torch.randn(n, device=dev, generator=gen)
        for s in range(0, m, 8):                         # a group at a time: 8 gradients live
            gs = [base + torch.randn(n, device=dev, generator=gen) for _ in range(min(8, m - s))]
            for i, g in enumerate(gs):
                codec.encode_sign(g, packet=signs[s + i])
            codec.encode_top_batch(gs, k, packets=tops[s:s + len(gs)])
            for p in tops[s:s + len(gs)]:
                p.release()
            del gs
        codec.BatchWorkspace._cache.clear()
        v = torch.randn(n, device=dev, generator=gen)
        del base
        torch.cuda.empty_cache()
        slab = torch.empty((m, n), dtype=torch.float32, device=dev)
        row = torch.empty(n, dtype=torch.float32, device=dev)
        out_g = torch.empty((m, m), dtype=torch.float64, device=dev)
        out_t = torch.empty((m, m), dtype=torch.float64, device=dev)
        out_d = torch.empty(m + 1, dtype=torch.float64, device=dev)
        dense_d = torch.empty(m, dtype=torch.float64, device=dev)

        def dense_gram():
            for i, p in enumerate(signs):
                codec.decode_sign(p, out=slab[i])
            G64 = slab.double()
            return G64 @ G64.T

        def dense_dot():
            v64 = v.double()
            for i, p in enumerate(signs):
                codec.decode_sign(p, out=row)
                dense_d[i] = torch.dot(row.double(), v64)
            return dense_d

        # ---- checked once: the new values against the dense routes ----
        codec.gram_sign(signs, out=out_g)
        K, Kd = out_g.cpu().numpy(), dense_gram().cpu().numpy()
        sc = np.array([h.p for h in codec.headers(signs)], dtype=np.float64)
        gram_ok = bool(np.all(np.abs(K - Kd) <= n * 2.0 ** -52 * np.outer(sc, sc) * n))
        sym = bool(np.array_equal(K.view(np.uint64), K.T.copy().view(np.uint64)))
        d = codec.dot_sign(signs, v, out=out_d).cpu().numpy()
        dd = dense_dot().cpu().numpy()
        l1 = float(v.double().abs().sum())
        dot_ok = bool(np.all(np.abs(d[:m] - dd) <= 2 * n * 2.0 ** -53 * sc * l1))
        ones = codec.dot_sign(signs, None).cpu().numpy()
        ones_ok = bool(np.all(np.abs(ones[:m] - slab.double().sum(dim=1).cpu().numpy())
                              <= n * 2.0 ** -53 * sc * n) and ones[m] == float(n))
        t = alternate({"gram": lambda: codec.gram_sign(signs, out=out_g),
                       "dense_gram": dense_gram,
                       "top_gram": lambda: codec.gram(tops, out=out_t),
                       "dot": lambda: codec.dot_sign(signs, v, out=out_d),
                       "dot_ones": lambda: codec.dot_sign(signs, None, out=out_d),
                       "dense_dot": dense_dot}, a.rounds)
        gram_bytes, dot_bytes = m * n / 8, m * n / 8 + 4 * n
        rec = {"bench": "sign_gram_bench", "M": m, "N": n, "f": a.f, "rounds": a.rounds,
               "us": {k_: x[0] for k_, x in t.items()},
               "minmax": {k_: x[1] for k_, x in t.items()},
               "gram_symmetric_bits": sym, "gram_within_dense_bound": gram_ok,
               "dot_within_dense_bound": dot_ok, "dot_ones_within_dense_bound": ones_ok,
               "speedup": {"gram_vs_dense": round(t["dense_gram"][0] / t["gram"][0], 1),
                           "gram_vs_top_gram": round(t["top_gram"][0] / t["gram"][0], 2),
                           "dot_vs_dense": round(t["dense_dot"][0] / t["dot"][0], 1),
                           "dot_ones_vs_dense": round(t["dense_dot"][0] / t["dot_ones"][0], 1)},
               "model_frac_of_8TBs": {"gram": round(gram_bytes / PEAK * 1e6 / t["gram"][0], 3),
                                      "dot": round(dot_bytes / PEAK * 1e6 / t["dot"][0], 3),
                                      "dot_ones": round(gram_bytes / PEAK * 1e6 / t["dot_ones"][0], 3)},
               "dense_slab_floor_us": round(8 * m * n / PEAK * 1e6, 1),
               "gram_below_dense_slab_floor": bool(t["gram"][0] < 8 * m * n / PEAK * 1e6),
               "workspace_bytes": {"gram": int(lib.fc_sign_gram_workspace_bytes(n, m)),
                                   "dot": int(lib.fc_sign_dot_workspace_bytes(n, m))}}
        emit(rec)
        del signs, tops, slab, row, v
        torch.cuda.empty_cache()

    # ---- (f) one Aggregator round ----
    for shape in [s for s in a.agg_shapes.split(",") if s]:
        m, n = (int(x) for x in shape.split("x"))
        base = np.random.default_rng(3).standard_normal(n).astype(np.float32)
        grads = [np.roll(base, 1009 * i) * np.float32(1.0 + i / m) for i in range(m)]

        def clients():
            return [types.SimpleNamespace(C=Compression({"compression_function": "sign"}), grad=x, client_id=i)
                    for i, x in enumerate(grads)]

        res = {}
        for name, path, cfg in (("fed_avg", "sign", {}),
                                ("krum", "sign-gram", {"sign_geometry": True}),
                                ("geometric_median", "sign-gram", {"sign_geometry": True})):
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
        emit({"bench": "sign_gram_bench_aggregator", "M": m, "N": n, "rounds": a.agg_rounds, "routes": res})


if __name__ == "__main__":
    main()
