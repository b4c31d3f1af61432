"""Error-feedback top-k: the fused call against the composition it replaces, HIP-event timed.

    python tools/ef_bench.py [--sizes 16777216,134217728] [--f 0.1] [--out FILE]

fused        codec.encode_top_ef(g, e, k, residual_out=e2, check=False)     (fc_topk_encode_ef)
composition  a = torch.add(g, e); encode_top(a, k); q = decode(packet); e2 = torch.sub(a, q)
             (entry points that predate the fused call)
Both run in the same process on the same tensors, alternating in rounds after a warm-up; the
figure per size is the median round.  hbm_frac: the byte model 12 N + 6.7 B x n_entries (g and
e read, e' written, 6 B per listed entry written plus the small per-chunk words) over the
fused time, against the HBM peak.  One JSON line.  Needs a GPU: no fallback.
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
    ap.add_argument("--sizes", default="16777216,134217728")
    ap.add_argument("--f", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ef_bench needs a GPU")
    from openmsftl_amd import _lib as L
    from openmsftl_amd import codec
    from openmsftl_amd.compression import kept_count

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    res = {"bench": "ef_bench", "f": a.f, "hbm_peak_GBps": HBM_PEAK_GBPS, "sizes": []}
    for n in [int(x) for x in a.sizes.split(",")]:
        k = kept_count(a.f, n)
        gen = torch.Generator(device="cuda").manual_seed(n % 1000 + 3)
        g = torch.randn(n, device="cuda", generator=gen)
        e = torch.randn(n, device="cuda", generator=gen) * 0.5
        e2, acc, q = torch.empty_like(g), torch.empty_like(g), torch.empty_like(g)
        pf = codec.Packet.alloc(n, L.FC_FMT_IDXVAL, g.device, k=k)
        pc = codec.Packet.alloc(n, L.FC_FMT_IDXVAL, g.device, k=k)
        e2c = torch.empty_like(g)

        def fused():
            codec.encode_top_ef(g, e, k, residual_out=e2, packet=pf, check=False)

        def composed():
            torch.add(g, e, out=acc)
            codec.encode_top(acc, k, packet=pc, check=False)
            codec.decode(pc, out=q)
            torch.sub(acc, q, out=e2c)

        iters = 20 if n > (64 << 20) else 100
        for fn in (fused, composed):                   # warm-up: code objects, workspaces
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        retries = codec.resolve([pf]) + codec.resolve([pc])
        tf, tc = [], []
        for _ in range(a.rounds):                      # alternate: both see the same neighbours
            tf.append(timed(fused, iters))
            tc.append(timed(composed, iters))
        # same result (finite inputs: a - q is the residual rule)
        same = bool(torch.equal(e2.view(torch.int32), e2c.view(torch.int32))
                    and torch.equal(codec.decode(pf), q))
        with L.KernelTimer(0xF) as kt:                 # per-kernel-class times of the fused call
            for _ in range(10):
                fused()
        n_entries = int(pf.header().n_entries)
        us_f, us_c = statistics.median(tf), statistics.median(tc)
        model = 12.0 * n + 6.7 * n_entries
        res["sizes"].append({
            "n": n, "k": k, "n_entries": n_entries, "retries": retries, "same_bits": same,
            "fused_us": round(us_f, 1), "composition_us": round(us_c, 1),
            "fused_us_minmax": [round(min(tf), 1), round(max(tf), 1)],
            "composition_us_minmax": [round(min(tc), 1), round(max(tc), 1)],
            "ratio": round(us_c / us_f, 3),
            "model_bytes": int(model),
            "hbm_frac": round(model / us_f / 1e3 / HBM_PEAK_GBPS, 4),
            "fused_kernel_us": {"sample": round(kt.avg_us("sample"), 1),
                                "compact": round(kt.avg_us("compact"), 1),
                                "resolve_2_launches": round(1e3 * kt.ms["engine"] / 10, 1)},
        })
        del g, e, e2, acc, q, e2c, pf, pc
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
