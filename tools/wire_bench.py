"""The wire format's kernels against the only route there was before them, and a whole round from
host payloads against the round from host gradients.  HIP-event timed.

    python tools/wire_bench.py [--shapes 128x16777216,32x134217728] [--f 0.1] [--out FILE]
                               [--round 32x25500000] [--rounds 7]

Pack / unpack, per shape (top-k packets of normal gradients, codec.encode_top_batch, as
tools/gram_bench.py makes them: the sampled bracket's slack is listed):
(a) hip     fc_wire_pack_batch on prebuilt tables: one launch chain for the m packets
(b) torch   what a caller could do without the kernel: per packet the keep rule as torch
            elementwise ops over the slotted buffers, boolean-mask selection of idx / val, the
            table by sums over the mask, and torch.cat of the sections' bytes.  T64 and the
            header bytes are read before the clock starts.  Its bytes are first verified equal
            to the kernel's for every client and to tests/wire_model.py's for client 0.
    unpack  fc_wire_unpack_batch of (a)'s packets into a second set of slotted packets.
Bytes are algorithmic: pack reads the listed entries (6 B each) and the source table (8 B per
chunk) and writes the kept entries, the table (12 B per chunk) and the header; unpack reads what
pack wrote and writes the same entries, counts, offsets and header.
One process; after a warm-up the forms alternate over the rounds; median and min-max.

A round (--round MxN): Aggregator.aggregate_wire on M host payloads (Compression.compress_wire's
bytes) against Aggregator.aggregate_grads on the same clients' NumPy gradients ('top', fed_avg:
the "stream" route), host wall time to the host aggregate; then the stages of the wire round one
by one: validation (host clock), H2D, unpack and fold (events), the aggregate's D2H (host clock).
One JSON line.  Needs a GPU: no fallback.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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
        raise SystemExit("wire_bench needs a GPU")
    from openmsftl_amd import _lib as L
    from openmsftl_amd import codec
    from openmsftl_amd.compression import Compression, kept_count
    lib = L.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    CH = L.FC_CHUNK

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
        return packets

    def pad16(t):
        r = (-t.numel()) % 16
        return [t, torch.zeros(r, dtype=torch.uint8, device=dev)] if r else [t]

    def torch_pack(p, thresh, ib, hdr128):
        """One packet's wire bytes with torch ops (magnitude keys, no NaN among the values)."""
        nch = p.cnt.numel()
        pos = torch.arange(p.capacity, device=dev, dtype=torch.int64)
        listed = (pos % CH) < p.cnt.to(torch.int64).repeat_interleave(CH)
        loc = p.idx.to(torch.int64) & 0xFFFF
        key = p.val.view(torch.int32).to(torch.int64) & 0x7FFFFFFF
        comp = (key << ib) | ((pos // CH) * CH + loc)
        keep = listed & (comp >= thresh)
        idx, val = p.idx[keep], p.val[keep]
        per = torch.stack([(keep & ((loc >> 11) <= q)).view(nch, CH).sum(1) for q in range(4)])
        qoff = per[0] | (per[1] << 16) | (per[2] << 32) | (per[3] << 48)
        start = (torch.cumsum(per[3], 0) - per[3]).to(torch.int32)
        E = int(idx.numel())
        h = hdr128.clone()
        h[8:16] = torch.tensor([int(lib.fc_wire_bytes(p.n, E))], dtype=torch.int64).view(torch.uint8).to(dev)
        h[16:24] = torch.tensor([E], dtype=torch.int64).view(torch.uint8).to(dev)
        h[32 + 24:32 + 28] = torch.tensor([E], dtype=torch.int32).view(torch.uint8).to(dev)
        parts = [h] + pad16(qoff.view(torch.uint8)) + pad16(start.view(torch.uint8)) \
            + pad16(idx.view(torch.uint8)) + pad16(val.view(torch.uint8))
        return torch.cat(parts)

    res = {"bench": "wire_bench", "f": a.f, "rounds": a.rounds, "shapes": []}
    for shape in [s for s in a.shapes.split(",") if s]:
        m, n = (int(x) for x in shape.split("x"))
        k = kept_count(a.f, n)
        nch = int(lib.fc_num_chunks(n))
        packets = encode(n, m, k)
        hs = codec.headers(packets)
        listed = sum(int(h.n_entries) for h in hs)
        cap = int(lib.fc_wire_bytes(n, k))
        slab = torch.empty((m, (cap + 255) & ~255), dtype=torch.uint8, device=dev)
        bufs = [slab[i, :cap] for i in range(m)]
        views = codec.views_tensor(packets, [1.0] * m, dev)
        jobs = codec._wire_jobs(bufs, [cap] * m, dev)
        ws = codec.WireWorkspace.get(n, m, dev)
        stream = codec._stream(dev)

        def hip_pack():
            L.check(lib.fc_wire_pack_batch(codec._vp(views), codec._vp(jobs), m, n, codec._vp(ws.buf),
                                           ws.nbytes, stream), "fc_wire_pack_batch")

        # the canonical headers the torch form starts from (read before the clock)
        hip_pack()
        torch.cuda.synchronize()
        hdr128 = [b[:128].clone() for b in bufs]
        thr = [int(h.thresh) for h in hs]
        ib = int(hs[0].index_bits)

        def torch_pack_all():
            return [torch_pack(p, t, ib, h) for p, t, h in zip(packets, thr, hdr128)]

        got = torch_pack_all()
        equal = all(g.numel() == cap and torch.equal(g, b) for g, b in zip(got, bufs))
        model_equal = None
        if not res["shapes"]:                            # the model's bytes, client 0 of the first shape
            import wire_model as wm
            from oracle import packet_oracle as po
            p0 = packets[0]
            f = {"n": n, "fmt": po.FMT_IDXVAL, "idx": p0.idx.cpu().numpy().view(np.uint16),
                 "val": p0.val.cpu().numpy(), "cnt": p0.cnt.cpu().numpy().view(np.uint32),
                 "hdr": np.frombuffer(bytes(hs[0]), dtype=po.HDR_DTYPE)[0]}
            model_equal = wm.pack(f) == got[0].cpu().numpy().tobytes()
        del got
        dst = codec.Packet.alloc_batch(n, m, L.FC_FMT_IDXVAL, dev)
        dviews = codec.views_tensor(dst, [1.0] * m, dev)

        def hip_unpack():
            L.check(lib.fc_wire_unpack_batch(codec._vp(jobs), codec._vp(dviews), m, n, stream),
                    "fc_wire_unpack_batch")

        forms = (hip_pack, torch_pack_all, hip_unpack)
        for fn in forms:                                 # warm-up: code objects, the allocator's pools
            fn()
        torch.cuda.synchronize()
        t = [[] for _ in forms]
        for _ in range(a.rounds):                        # alternate: all see the same neighbours
            for i, fn in enumerate(forms):
                us, _ = timed(fn)
                t[i].append(us)
        first = slab.clone()
        hip_pack()
        torch.cuda.synchronize()
        same_twice = bool(torch.equal(first, slab))
        back_equal = bool(torch.equal(codec.decode(dst[0]).view(torch.int32),
                                      codec.decode(packets[0]).view(torch.int32)))
        E = m * k
        pack_bytes = 6 * listed + 8 * nch * m + 6 * E + 12 * nch * m + 128 * m
        unpack_bytes = 2 * (6 * E + 12 * nch * m) + (128 + 96) * m
        med = [statistics.median(x) for x in t]
        res["shapes"].append({
            "m": m, "n": n, "k": k, "listed_entries": listed, "kept_entries": E,
            "wire_bytes_per_packet": cap, "slotted_bytes_per_packet": 6 * nch * CH + 12 * nch + 96,
            "dense_bytes_per_gradient": 4 * n,
            "hip_pack": stats(t[0]), "torch_pack": stats(t[1]), "hip_unpack": stats(t[2]),
            "ratio_torch_over_hip_pack": round(med[1] / med[0], 1),
            "pack_algorithmic_bytes": pack_bytes, "pack_TBps": round(pack_bytes / med[0] / 1e6, 3),
            "unpack_algorithmic_bytes": unpack_bytes, "unpack_TBps": round(unpack_bytes / med[2] / 1e6, 3),
            "torch_equals_hip_bytes": bool(equal), "torch_equals_model_bytes_client0": model_equal,
            "same_bytes_twice": same_twice, "unpacked_decode_equal_client0": back_equal,
            "pack_workspace_bytes": int(lib.fc_wire_workspace_bytes(n, m)),
        })
        del packets, dst, slab, bufs, views, dviews, jobs, hdr128, first
        codec.WireWorkspace._cache.clear()
        torch.cuda.empty_cache()

    if a.round:
        from openmsftl_amd.aggregation import Aggregator
        m, n = (int(x) for x in a.round.split("x"))
        k = kept_count(a.f, n)
        rng = np.random.default_rng(5)
        grads = [rng.standard_normal(n, dtype=np.float32) for _ in range(m)]
        cfg = {"compression_function": "top", "fraction_coordinate": a.f}
        clients = [types.SimpleNamespace(C=Compression(dict(cfg)), grad=g, client_id=i)
                   for i, g in enumerate(grads)]
        payloads = [c.C.compress_wire(c.grad) for c in clients]          # the clients' side: not timed
        agg_w = Aggregator({"aggregation_scheme": "fed_avg"})
        agg_g = Aggregator({"aggregation_scheme": "fed_avg"})

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        forms = (lambda: agg_w.aggregate_wire(payloads), lambda: agg_g.aggregate_grads(clients))
        for fn in forms:
            fn()
        equal = agg_w.agg_grad.tobytes() == agg_g.agg_grad.tobytes()
        tw = [[], []]
        for _ in range(a.rounds):
            for i, fn in enumerate(forms):
                tw[i].append(wall(fn))
        # the wire round's stages, one by one
        tv, th, tu, tf, td = [], [], [], [], []
        arrs = [np.frombuffer(p, dtype=np.uint8) for p in payloads]
        pk = codec.Packet.alloc_batch(n, m, L.FC_FMT_IDXVAL, dev)
        out = torch.empty(n, dtype=torch.float32, device=dev)
        w = [float(np.float32(1.0 / m))] * m
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            for x in arrs:
                assert lib.fc_wire_validate(ctypes.c_void_p(x.ctypes.data), x.size, n) == 0
            tv.append((time.perf_counter() - t0) * 1e3)
            us, wires = timed(lambda: [codec.TOP.upload(x, L.WireHdr.from_buffer_copy(x[:128].tobytes()), dev)
                                       for x in arrs])
            th.append(us / 1e3)
            us, _ = timed(lambda: codec.unpack(wires, pk))
            tu.append(us / 1e3)
            us, _ = timed(lambda: codec.decode_accumulate(pk, w, out=out))
            tf.append(us / 1e3)
            td.append(wall(lambda: out.cpu().numpy()))
            del wires

        def ms(x):
            return {"ms": round(statistics.median(x), 2), "minmax": [round(min(x), 2), round(max(x), 2)]}

        res["round"] = {
            "m": m, "n": n, "k": k, "payload_bytes": sum(len(p) for p in payloads),
            "gradient_bytes": 4 * n * m,
            "aggregate_wire": ms(tw[0]), "aggregate_grads": ms(tw[1]),
            "ratio_grads_over_wire": round(statistics.median(tw[1]) / statistics.median(tw[0]), 2),
            "same_aggregate_bits": bool(equal),
            "stages": {"validate_host": ms(tv), "h2d_pageable": ms(th), "unpack": ms(tu), "fold": ms(tf),
                       "d2h_aggregate": ms(td)},
        }
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
