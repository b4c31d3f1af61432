"""The packet Gram matrix against the only route there was before it, HIP-event timed.

    python tools/gram_bench.py [--shapes 128x16777216,32x134217728] [--f 0.1] [--out FILE]

(a) gram    codec.gram(packets)                                   (fc_packets_gram)
(b) dense   codec.decode of every packet into the rows of a dense float32 (M, N) matrix, then
            the float64 torch product blockwise over N (G[:, b].double() @ G[:, b].double().T
            summed over column blocks) — what a caller could do without the kernel, at a shape
            whose rows fit the device
One process; after a warm-up the two forms alternate over the rounds and the figure per shape is
the median round.  The packets are top-k packets of normal gradients (codec.encode_top_batch, one
group at a time).  max_rel_diff: the largest |a - b| / sqrt(a_ii a_jj) between the two results.
One JSON line.  Needs a GPU: no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128x16777216,32x134217728")
    ap.add_argument("--f", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--block", type=int, default=1 << 20, help="columns per float64 product")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gram_bench needs a GPU")
    from openmsftl_amd import _lib as L
    from openmsftl_amd import codec
    from openmsftl_amd.compression import kept_count
    dev = torch.device("cuda", torch.cuda.current_device())

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3, out

    res = {"bench": "gram_bench", "f": a.f, "block": a.block, "shapes": []}
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
        out_a = torch.empty((m, m), dtype=torch.float64, device=dev)
        G = torch.empty((m, n), dtype=torch.float32, device=dev)

        def gram():
            return codec.gram(packets, out=out_a)

        def dense():
            for i, p in enumerate(packets):
                codec.decode(p, out=G[i])
            acc = torch.zeros((m, m), dtype=torch.float64, device=dev)
            for b0 in range(0, n, a.block):
                blk = G[:, b0:b0 + a.block].double()
                acc.addmm_(blk, blk.T)
            return acc

        forms = (gram, dense)
        for fn in forms:                                 # warm-up: code objects, workspaces
            fn()
        torch.cuda.synchronize()
        t = [[], []]
        outs = [None, None]
        for _ in range(a.rounds):                        # alternate: both see the same neighbours
            for i, fn in enumerate(forms):
                us, outs[i] = timed(fn)
                t[i].append(us)
        d = torch.sqrt(torch.diagonal(outs[1]))
        rel = float(((outs[0] - outs[1]).abs() / (d[:, None] * d[None, :])).max())
        first = outs[0].clone()
        again = gram()
        med = [statistics.median(x) for x in t]
        entries = sum(int(h.n_entries) for h in codec.headers(packets))
        res["shapes"].append({
            "m": m, "n": n, "k": k, "n_entries_total": entries,
            "gram_us": round(med[0], 1), "dense_us": round(med[1], 1),
            "gram_us_minmax": [round(min(t[0]), 1), round(max(t[0]), 1)],
            "dense_us_minmax": [round(min(t[1]), 1), round(max(t[1]), 1)],
            "ratio_dense_over_gram": round(med[1] / med[0], 3),
            "model_fma_per_s": round(0.5 * m * (m + 1) * k / (med[0] * 1e-6), 0),
            "max_rel_diff": rel,
            "same_bits_twice": bool(torch.equal(again.view(torch.int64), first.view(torch.int64))),
            "gram_workspace_bytes": int(L.load().fc_gram_workspace_bytes(n, m)),
            "dense_G_bytes": 4 * m * n,
        })
        del packets, G, out_a, outs
        codec.GramWorkspace._cache.clear()
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
