"""QSGD with error feedback against what there was before it, in one process.

    python tools/qsgd_ef_bench.py [--shapes 16777216,134217728] [--bits 2,8]
                                  [--agg-shapes 32x25500000] [--out FILE]

(a) Per N and bits, one JSON line: the lone error-feedback encode, fused (codec.encode_qsgd with a
    residual: fc_qsgd_encode_ef, two launches) against the chain of the entry points there were
    before it on the same tensors (fc_ef_sum, codec.encode_qsgd, codec.decode_qsgd, a torch
    subtract; its three N-float temporaries allocated beforehand).  The two alternate over the rounds
    after a warm-up; whole-call times from HIP events, the median with min-max beside it, each as a
    fraction of 8 TB/s on its byte model (fused 20N + N W / 8, chain 36N + 2 N W / 8), and whether
    the min-max ranges overlap.  The header, codes and new residual of the two are compared once.
(b) Per M x N (--agg-shapes), one JSON line: wall time of one Aggregator round, host gradients (or
    payloads) in, host aggregate out, through "qsgd", "dense-fold" (the key off) and "wire-qsgd"
    (the payloads made beforehand), half of the clients with error feedback; equal bits checked.
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
    ap.add_argument("--shapes", default="16777216,134217728")
    ap.add_argument("--bits", default="2,8")
    ap.add_argument("--agg-shapes", default="32x25500000")
    ap.add_argument("--agg-bits", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--agg-rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("qsgd_ef_bench needs a GPU")
    from openmsftl_amd import _lib as L
    from openmsftl_amd import Compression, codec
    from openmsftl_amd.aggregation import Aggregator
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
        for _ in range(2):
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

    # ---- (a) the lone error-feedback encode ----
    for n in [int(s) for s in a.shapes.split(",") if s]:
        gen = torch.Generator(device=dev).manual_seed(n % 1000 + 23)
        g = torch.randn(n, device=dev, generator=gen)
        e = torch.randn(n, device=dev, generator=gen) * 0.5
        out_f, out_c = torch.empty(n, device=dev), torch.empty(n, device=dev)
        summed, q = torch.empty(n, device=dev), torch.empty(n, device=dev)     # the chain's temporaries
        for bits in [int(b) for b in a.bits.split(",") if b]:
            pk_f, pk_c = codec.QsgdPacket.alloc(n, bits, dev), codec.QsgdPacket.alloc(n, bits, dev)
            W = 4 if bits <= 2 else 8 if bits <= 6 else 16

            def fused():
                codec.encode_qsgd(g, bits, seed=5, offset=1, packet=pk_f, residual=e, residual_out=out_f)

            def chain():
                L.check(lib.fc_ef_sum(codec._vp(g), codec._vp(e), codec._vp(summed), n, codec._stream(dev)),
                        "fc_ef_sum")
                codec.encode_qsgd(summed, bits, seed=5, offset=1, packet=pk_c)
                codec.decode_qsgd(pk_c, out=q)
                torch.sub(summed, q, out=out_c)

            fused(), chain()
            same = {"header": bool(torch.equal(pk_f.hdr, pk_c.hdr)), "codes": bool(torch.equal(pk_f.codes, pk_c.codes)),
                    "residual": bool(torch.equal(out_f.view(torch.int32), out_c.view(torch.int32)))}
            t = alternate({"fused": fused, "chain": chain}, a.rounds)
            model = {"fused": 20 * n + n * W / 8, "chain": 36 * n + 2 * n * W / 8}
            emit({"bench": "qsgd_ef_bench", "N": n, "bits": bits, "W": W, "rounds": a.rounds,
                  "us": {k: v[0] for k, v in t.items()}, "minmax": {k: v[1] for k, v in t.items()},
                  "fused_over_chain": round(t["fused"][0] / t["chain"][0], 3),
                  "ranges_overlap": bool(t["fused"][1][1] >= t["chain"][1][0]),
                  "model_bytes": model, "model_ratio": round(model["fused"] / model["chain"], 3),
                  "model_frac_of_8TBs": {k: round(b / PEAK * 1e6 / t[k][0], 3) for k, b in model.items()},
                  "fused_equals_chain_bytes": same})
            del pk_f, pk_c
        del g, e, out_f, out_c, summed, q
        torch.cuda.empty_cache()

    # ---- (b) one Aggregator round ----
    for shape in [s for s in a.agg_shapes.split(",") if s]:
        m, n = (int(x) for x in shape.split("x"))
        base = np.random.default_rng(3).standard_normal(n).astype(np.float32)
        grads = [np.roll(base, 1009 * i) * np.float32(1.0 + i / m) for i in range(m)]

        def clients():
            return [types.SimpleNamespace(
                C=Compression({"compression_function": "qsgd", "qsgd": "native", "num_bits": a.agg_bits,
                               "seed": i, "error_feedback": i % 2 == 0}), grad=x, client_id=i)
                for i, x in enumerate(grads)]

        payloads = [c.C.compress_wire(c.grad) for c in clients()]
        res, ref = {}, None
        for name, cfg, call in (("qsgd", {"qsgd_packets": True}, lambda ag: ag.aggregate_grads(clients())),
                                ("dense-fold", {}, lambda ag: ag.aggregate_grads(clients())),
                                ("wire-qsgd", {}, lambda ag: ag.aggregate_wire(payloads))):
            ag = Aggregator(dict({"aggregation_scheme": "fed_avg"}, **cfg))
            ts = []
            for _ in range(a.agg_rounds + 1):            # the first round warms up; fresh clients each
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(ag)
                ts.append(time.perf_counter() - t0)
            assert ag.agg_path == name, ag.agg_path
            ref = ag.agg_grad if ref is None else ref
            res[name] = {"ms": round(statistics.median(ts[1:]) * 1e3, 1),
                         "minmax_ms": [round(min(ts[1:]) * 1e3, 1), round(max(ts[1:]) * 1e3, 1)],
                         "equals_qsgd_route_bits": bool(ag.agg_grad.tobytes() == ref.tobytes())}
        emit({"bench": "qsgd_ef_bench_aggregator", "M": m, "N": n, "bits": a.agg_bits, "rounds": a.agg_rounds,
              "payload_bytes": len(payloads[0]), "gradient_bytes": 4 * n, "routes": res})


if __name__ == "__main__":
    main()
