"""Batched error-feedback top-k against M lone calls and the no-residual floor, HIP-event timed.

    python tools/ef_batch_bench.py [--shapes 128x16777216,32x134217728] [--f 0.1] [--out FILE]

(a) batch   codec.encode_top_ef_batch(grads, residuals, k, check=False)   (fc_topk_encode_ef_batch)
(b) lone    M x codec.encode_top_ef(g_c, e_c, k, check=False) on the same buffers (the code path
            that predates the batched call: the yardstick)
(c) floor   codec.encode_top_batch on the pre-summed a_c = g_c + e_c: no residual read or written
One process; after a warm-up the three forms alternate over the rounds and the figure per shape
is the median round.  M of a shape is cut to what fits the free device memory beside the
residuals.  hbm_frac: M x (12 N + 6.7 B x n_entries) over the batched time, against the HBM peak.
meets: (a) is faster than (b) by more than (b)'s own min-max spread over the rounds.
One JSON line.  Needs a GPU: no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0          # MI355X: HBM3E 8.0 TB/s (spec), as bench.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128x16777216,32x134217728")
    ap.add_argument("--f", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ef_batch_bench needs a GPU")
    from openmsftl_amd import _lib as L
    from openmsftl_amd import codec
    from openmsftl_amd.compression import kept_count
    from openmsftl_amd.pipeline import packet_bytes
    dev = torch.device("cuda", torch.cuda.current_device())

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    def listed_equal(p, q):
        """The listed entries, counts, quarter offsets and header of two packets, on the device."""
        pos = torch.arange(p.capacity, device=dev)
        listed = (pos % L.FC_CHUNK) < p.cnt[pos // L.FC_CHUNK]
        return bool(torch.equal(p.cnt, q.cnt) and torch.equal(p.qoff, q.qoff)
                    and torch.equal(p.hdr, q.hdr)
                    and torch.equal(p.idx[listed], q.idx[listed])
                    and torch.equal(p.val.view(torch.int32)[listed], q.val.view(torch.int32)[listed]))

    res = {"bench": "ef_batch_bench", "f": a.f, "hbm_peak_GBps": HBM_PEAK_GBPS, "shapes": []}
    for shape in a.shapes.split(","):
        m_want, n = (int(x) for x in shape.split("x"))
        k = kept_count(a.f, n)
        # per client: g, e, two outputs, a (4N each), two packets, a batch workspace
        per = 5 * 4 * n + 2 * packet_bytes(n) + int(L.load().fc_workspace_bytes(n))
        free, _ = torch.cuda.mem_get_info(dev)
        m = int(max(1, min(m_want, int(free * 0.85) // per)))
        gen = torch.Generator(device=dev).manual_seed(n % 1000 + 3)
        gs = [torch.randn(n, device=dev, generator=gen) * (10.0 ** (c % 5 - 2)) for c in range(m)]
        es = [torch.randn(n, device=dev, generator=gen) * (0.5 * 10.0 ** (c % 5 - 2)) for c in range(m)]
        out_a = [torch.empty(n, device=dev) for _ in range(m)]
        out_b = [torch.empty(n, device=dev) for _ in range(m)]
        sums = [torch.add(g, e) for g, e in zip(gs, es)]
        pa = codec.Packet.alloc_batch(n, m, L.FC_FMT_IDXVAL, dev, k=k)
        pb = codec.Packet.alloc_batch(n, m, L.FC_FMT_IDXVAL, dev, k=k)   # (b), then (c)
        jobs_a, efj = codec.encode_jobs(gs, pa), codec.ef_jobs(es, out_a)
        jobs_c = codec.encode_jobs(sums, pb)

        def batch():
            codec.encode_top_ef_batch(gs, es, k, residuals_out=out_a, packets=pa, jobs=jobs_a,
                                      ef_jobs=efj, check=False)

        def lone():
            for g, e, o, p in zip(gs, es, out_b, pb):
                codec.encode_top_ef(g, e, k, residual_out=o, packet=p, check=False)

        def floor():
            codec.encode_top_batch(sums, k, packets=pb, jobs=jobs_c, check=False)

        forms = (batch, lone, floor)
        retries = 0
        for fn, pk in zip(forms, (pa, pb, pb)):        # warm-up: code objects, workspaces
            for _ in range(2):
                fn()
            retries += codec.resolve(pk)
        iters = 3
        t = [[], [], []]
        for _ in range(a.rounds):                      # alternate: all see the same neighbours
            for i, fn in enumerate(forms):
                t[i].append(timed(fn, iters))
        batch()
        lone()
        torch.cuda.synchronize()
        retries += codec.resolve(pa) + codec.resolve(pb)
        same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(out_a, out_b)) \
            and all(listed_equal(p, q) for p, q in zip(pa, pb))
        with L.KernelTimer(0xF) as kt:                 # per-kernel-class times of the batched call
            for _ in range(3):
                batch()
        entries = sum(int(h.n_entries) for h in codec.headers(pa))
        med = [statistics.median(x) for x in t]
        model = 12.0 * n * m + 6.7 * entries
        spread_b = max(t[1]) - min(t[1])
        res["shapes"].append({
            "m": m, "m_wanted": m_want, "n": n, "k": k, "n_entries_total": entries,
            "retries": retries, "same_bits": bool(same),
            "batch_us": round(med[0], 1), "lone_us": round(med[1], 1), "floor_us": round(med[2], 1),
            "batch_us_minmax": [round(min(t[0]), 1), round(max(t[0]), 1)],
            "lone_us_minmax": [round(min(t[1]), 1), round(max(t[1]), 1)],
            "floor_us_minmax": [round(min(t[2]), 1), round(max(t[2]), 1)],
            "per_client_us": {"batch": round(med[0] / m, 2), "lone": round(med[1] / m, 2),
                              "floor": round(med[2] / m, 2)},
            "ratio_lone_over_batch": round(med[1] / med[0], 3),
            "gain_us": round(med[1] - med[0], 1), "lone_spread_us": round(spread_b, 1),
            "meets": bool(med[1] - med[0] > spread_b),
            "model_bytes": int(model),
            "hbm_frac": round(model / med[0] / 1e3 / HBM_PEAK_GBPS, 4),
            "batch_kernel_us": {"pilot_and_sample": round(1e3 * kt.ms["sample"] / 3, 1),
                                "compact": round(1e3 * kt.ms["compact"] / 3, 1),
                                "resolve_2_launches": round(1e3 * kt.ms["engine"] / 3, 1)},
        })
        del gs, es, out_a, out_b, sums, pa, pb, jobs_a, jobs_c, efj
        codec.BatchWorkspace._cache.clear()
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
