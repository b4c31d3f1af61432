"""The scaled-sign codec against what there was before it, in one process.

    python tools/sign_bench.py [--shapes 128x16777216,32x134217728] [--agg-shapes 32x25500000]
                               [--f 0.1] [--out FILE]
    python tools/sign_bench.py --batch [--batch-shapes 128x16777216,32x134217728] [--out FILE]

Per shape M x N (HIP events, the forms alternating over the rounds after a warm-up, the figure the
median round with min-max beside it), one JSON line:
(a) the lone encode, codec.encode_sign without and with a residual, against what a caller could
    do before from torch ops on the same tensors (the add, abs().sum() in float64, the sign
    select, the subtract), and against the encode's byte model (8N + N/8, with a residual
    16N + N/8 + 4N) as a fraction of 8 TB/s
(b) codec.fold_sign, in every word-loading form (fc_sign_fold_form: scalar loads / vector loads
    and v_readlane / a word per lane; the A/B of that choice), against codec.weighted_sum_dense on the decoded rows
    and against codec.decode_accumulate on the same clients' 'top' f = 0.1 packets; checked once
    per shape for equal bits with the dense fold.  Byte model M N/8 + 4N.  The figure is what a
    call costs: it includes the host's making and uploading of the M-entry view table
(c) codec.vote_sign (every form) against codec.trimmed_mean at the median on the 'top' packets (at
    most FC_GRAM_MAX_M clients)
(d) payload bytes per client: the sign wire form and the 'top' wire form at f
Aggregator part (--agg-shapes), one JSON line per shape:
(e) wall time of one round, host gradients (or payloads) in, host aggregate out, through "sign",
    "dense-fold" ("sign_packets": False) and "wire-sign" (the payloads made beforehand)
Batched encode (--batch: this part alone), one JSON line per shape M x N:
(f) M lone encodes against ONE codec.encode_sign_batch with a prebuilt job table, device-resident
    gradients, in three forms: without residuals, with res_in only (the lone side calls
    fc_sign_encode with a NULL res_out: codec.encode_sign always writes e'), with res_in and
    res_out.  Whole-call times, the six alternating in one process; each form's byte model (lone
    8N / 16N / 20N + N/8, batched 4N / 8N / 20N + N/8 per client) as a fraction of 8 TB/s, and the
    lone two-pass time per client; the first and last client's bytes are compared once per form.
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
    ap.add_argument("--batch", action="store_true", help="the batched-encode part alone")
    ap.add_argument("--batch-shapes", default="128x16777216,32x134217728")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sign_bench needs a GPU")
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

    def with_form(form, fn):
        def run():
            lib.fc_sign_fold_form(form)
            try:
                return fn()
            finally:
                lib.fc_sign_fold_form(-1)
        return run

    # ---- (f) the batched encode ----
    for shape in [s for s in a.batch_shapes.split(",") if s and a.batch]:
        m, n = (int(x) for x in shape.split("x"))
        gen = torch.Generator(device=dev).manual_seed(n % 1000 + 17)
        gs = [torch.randn(n, device=dev, generator=gen) for _ in range(m)]
        es = [torch.randn(n, device=dev, generator=gen) * 0.5 for _ in range(m)]
        outs = [torch.empty(n, device=dev) for _ in range(m)]
        lone_pk = [codec.SignPacket.alloc(n, dev) for _ in range(m)]
        bat_pk = [codec.SignPacket.alloc(n, dev) for _ in range(m)]
        jobs = {"plain": codec.sign_jobs(gs, bat_pk), "res_in": codec.sign_jobs(gs, bat_pk, es),
                "ef": codec.sign_jobs(gs, bat_pk, es, outs)}
        codec.encode_sign(gs[0], packet=lone_pk[0])                      # makes the lone workspace
        ws = codec._SIGN_WS[(dev.index, torch.cuda.current_stream(dev).cuda_stream)]

        def lone_plain():
            for g, p in zip(gs, lone_pk):
                codec.encode_sign(g, packet=p)

        def lone_res_in():
            st = codec._stream(dev)
            for g, e, p in zip(gs, es, lone_pk):
                L.check(lib.fc_sign_encode(codec._vp(g), codec._vp(e), None, n, codec._vp(p.words),
                                           p.words.numel(), codec._vp(p.hdr), codec._vp(ws), ws.numel(), st),
                        "fc_sign_encode")

        def lone_ef():
            for g, e, o, p in zip(gs, es, outs, lone_pk):
                codec.encode_sign(g, e, residual_out=o, packet=p)

        forms = {"lone_plain": lone_plain,
                 "batch_plain": lambda: codec.encode_sign_batch(gs, packets=bat_pk, jobs=jobs["plain"]),
                 "lone_res_in": lone_res_in,
                 "batch_res_in": lambda: codec.encode_sign_batch(gs, es, want_residuals=False, packets=bat_pk,
                                                                 jobs=jobs["res_in"]),
                 "lone_ef": lone_ef,
                 "batch_ef": lambda: codec.encode_sign_batch(gs, es, outs, packets=bat_pk, jobs=jobs["ef"])}
        same = {}
        for form in ("plain", "res_in", "ef"):
            keep = []
            for side in ("lone", "batch"):
                for p in lone_pk + bat_pk:
                    p.words.fill_(-1)
                outs[0].fill_(0), outs[-1].fill_(0)
                forms[f"{side}_{form}"]()
                pk = lone_pk if side == "lone" else bat_pk
                keep.append([t.cpu().numpy().tobytes() for i in (0, m - 1)
                             for t in (pk[i].hdr, pk[i].words, outs[i])])
            same[form] = keep[0] == keep[1]
        t = alternate(forms, max(a.rounds, 5))
        lone_b = {"plain": 8 * n + n / 8, "res_in": 16 * n + n / 8, "ef": 20 * n + n / 8}
        bat_b = {"plain": 4 * n + n / 8, "res_in": 8 * n + n / 8, "ef": 20 * n + n / 8}
        emit({"bench": "sign_batch_bench", "M": m, "N": n, "rounds": max(a.rounds, 5),
              "us": {k_: v[0] for k_, v in t.items()}, "minmax": {k_: v[1] for k_, v in t.items()},
              "batch_over_lone": {f: round(t[f"batch_{f}"][0] / t[f"lone_{f}"][0], 3) for f in lone_b},
              "lone_us_per_client": {f: round(t[f"lone_{f}"][0] / m, 1) for f in lone_b},
              "batch_us_per_client": {f: round(t[f"batch_{f}"][0] / m, 1) for f in lone_b},
              "lone_model_frac_of_8TBs": {f: round(m * b / PEAK * 1e6 / t[f"lone_{f}"][0], 3)
                                          for f, b in lone_b.items()},
              "batch_model_frac_of_8TBs": {f: round(m * b / PEAK * 1e6 / t[f"batch_{f}"][0], 3)
                                           for f, b in bat_b.items()},
              "batch_equals_lone_bytes": same})
        del gs, es, outs, lone_pk, bat_pk, jobs
        torch.cuda.empty_cache()
    if a.batch:
        return

    for shape in [s for s in a.shapes.split(",") if s]:
        m, n = (int(x) for x in shape.split("x"))
        k = kept_count(a.f, n)
        gen = torch.Generator(device=dev).manual_seed(n % 1000 + 11)
        signs = [codec.SignPacket.alloc(n, dev) for _ in range(m)]
        tops = codec.Packet.alloc_batch(n, m, L.FC_FMT_IDXVAL, dev, k=k)
        rows = torch.empty((m, n), dtype=torch.float32, device=dev)
        for s in range(0, m, 8):                         # a group at a time: 8 gradients live
            gs = [torch.randn(n, device=dev, generator=gen) for _ in range(min(8, m - s))]
            for i, g in enumerate(gs):
                codec.encode_sign(g, packet=signs[s + i])
                codec.decode_sign(signs[s + i], out=rows[s + i])
            codec.encode_top_batch(gs, k, packets=tops[s:s + len(gs)])
            for p in tops[s:s + len(gs)]:
                p.release()
            del gs
        codec.BatchWorkspace._cache.clear()
        torch.cuda.empty_cache()
        w = [1.0 / m] * m
        wt = torch.full((m,), 1.0 / m, dtype=torch.float32)
        # ---- (a) the lone encode ----
        g = torch.randn(n, device=dev, generator=gen)
        e = torch.randn(n, device=dev, generator=gen) * 0.5
        pkt, e_out = codec.SignPacket.alloc(n, dev), torch.empty(n, device=dev)

        def torch_plain():
            s = (g.abs().sum(dtype=torch.float64) / n).to(torch.float32)
            return torch.where(torch.signbit(g), -s, s)

        def torch_ef():
            x = g + e
            s = (x.abs().sum(dtype=torch.float64) / n).to(torch.float32)
            q = torch.where(torch.signbit(x), -s, s)
            return q, x - q

        enc = alternate({"encode": lambda: codec.encode_sign(g, packet=pkt),
                         "encode_ef": lambda: codec.encode_sign(g, e, residual_out=e_out, packet=pkt),
                         "torch": torch_plain, "torch_ef": torch_ef}, a.rounds)
        model = {"encode": 8 * n + n / 8, "encode_ef": 16 * n + n / 8 + 4 * n}
        # ---- (b) the fold ----
        out_s, out_d, out_t = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))
        dense = lambda: codec.weighted_sum_dense(rows, wt, out=out_d)         # noqa: E731
        fold0 = with_form(0, lambda: codec.fold_sign(signs, w, out=out_s))
        fold1 = with_form(1, lambda: codec.fold_sign(signs, w, out=out_s))
        fold2 = with_form(2, lambda: codec.fold_sign(signs, w, out=out_s))
        dense()
        same = {}
        for name, fn in (("scalar", fold0), ("vector", fold1), ("lane", fold2)):
            out_s.fill_(float("nan"))
            fn()
            same[name] = bool(torch.equal(out_s.view(torch.int32), out_d.view(torch.int32)))
        fold = alternate({"fold_sign_scalar": fold0, "fold_sign_vector": fold1, "fold_sign_lane": fold2,
                          "dense_rows": dense,
                          "top_packets": lambda: codec.decode_accumulate(tops, w, out=out_t)}, a.rounds)
        # ---- (c) the vote ----
        mt = min(m, L.FC_GRAM_MAX_M)
        vote = alternate({"vote_sign_scalar": with_form(0, lambda: codec.vote_sign(signs, 0.01, out=out_s)),
                          "vote_sign_vector": with_form(1, lambda: codec.vote_sign(signs, 0.01, out=out_s)),
                          "vote_sign_lane": with_form(2, lambda: codec.vote_sign(signs, 0.01, out=out_s)),
                          "median_top": lambda: codec.trimmed_mean(tops[:mt], (mt - 1) // 2, out=out_t)},
                         a.rounds)
        fold_bytes = m * n / 8 + 4 * n
        rec = {"bench": "sign_bench", "M": m, "N": n, "f": a.f, "rounds": a.rounds,
               "encode_us": {k_: v[0] for k_, v in enc.items()},
               "encode_minmax": {k_: v[1] for k_, v in enc.items()},
               "encode_model_frac_of_8TBs": {k_: round(b / PEAK * 1e6 / enc[k_][0], 3) for k_, b in model.items()},
               "fold_us": {k_: v[0] for k_, v in fold.items()},
               "fold_minmax": {k_: v[1] for k_, v in fold.items()},
               "fold_equals_dense_bits": same,
               "fold_model_frac_of_8TBs": {k_: round(fold_bytes / PEAK * 1e6 / fold[k_][0], 3)
                                           for k_ in ("fold_sign_scalar", "fold_sign_vector", "fold_sign_lane")},
               "vote_us": {k_: v[0] for k_, v in vote.items()},
               "vote_minmax": {k_: v[1] for k_, v in vote.items()}, "vote_median_clients": mt,
               "payload_bytes": {"sign": codec.sign_wire_bytes(n), "top": codec.wire_bytes(n, k),
                                 "gradient": 4 * n}}
        emit(rec)
        del signs, tops, rows, g, e, pkt, e_out, out_s, out_d, out_t
        torch.cuda.empty_cache()

    # ---- (e) one Aggregator round ----
    for shape in [s for s in a.agg_shapes.split(",") if s]:
        m, n = (int(x) for x in shape.split("x"))
        base = np.random.default_rng(3).standard_normal(n).astype(np.float32)
        grads = [np.roll(base, 1009 * i) * np.float32(1.0 + i / m) for i in range(m)]

        def clients():
            return [types.SimpleNamespace(C=Compression({"compression_function": "sign"}), grad=x, client_id=i)
                    for i, x in enumerate(grads)]

        payloads = [c.C.compress_wire(c.grad) for c in clients()]
        res, ref = {}, None
        for name, cfg, call in (("sign", {}, lambda ag: ag.aggregate_grads(clients())),
                                ("dense-fold", {"sign_packets": False}, lambda ag: ag.aggregate_grads(clients())),
                                ("wire-sign", {}, lambda ag: ag.aggregate_wire(payloads))):
            ag = Aggregator(dict({"aggregation_scheme": "fed_avg"}, **cfg))
            ts = []
            for _ in range(a.agg_rounds + 1):            # the first round warms up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(ag)
                ts.append(time.perf_counter() - t0)
            assert ag.agg_path == name, ag.agg_path
            ref = ag.agg_grad if ref is None else ref
            res[name] = {"ms": round(statistics.median(ts[1:]) * 1e3, 1),
                         "minmax_ms": [round(min(ts[1:]) * 1e3, 1), round(max(ts[1:]) * 1e3, 1)],
                         "equals_sign_route_bits": bool(ag.agg_grad.tobytes() == ref.tobytes())}
        emit({"bench": "sign_bench_aggregator", "M": m, "N": n, "rounds": a.agg_rounds, "routes": res})


if __name__ == "__main__":
    main()
