"""Where does a device np.random.permutation row's time go, and what does it buy the Aggregator?

* per-stage device times of fc_mt_permutation (HIP events around words / parse / link / trace /
  commit: fc_mt_perm_timing) at 16 M and 25.5 M elements, k = n/10 and k = n;
* the Aggregator's 'rand' rate at 25.5 M x 32 clients, NumPy in and NumPy out, with
  aggregation_config["device_permutation"] off (the host draws) and on, in one process.

    python tools/perm_probe.py [--clients 32] [--n 25557032]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openmsftl_amd import Compression, codec            # noqa: E402
from openmsftl_amd import _lib as L                     # noqa: E402
from openmsftl_amd.aggregation import Aggregator        # noqa: E402

STAGES = ("words", "parse", "link", "trace", "commit")


def stage_times(n, k, reps=3):
    lib = L.load()
    np.random.seed(1)
    key, pos, _, _ = codec.mt_state()
    R = codec.PermRound(n, key, pos)
    mask = torch.empty((n + 31) // 32, dtype=torch.int32, device="cuda")
    R.permutation(k, out_mask=mask)                     # warm: plan upload, first launches
    torch.cuda.synchronize()
    L.check(lib.fc_mt_perm_timing(1, None), "fc_mt_perm_timing")
    best = None
    for _ in range(reps):
        R.permutation(k, out_mask=mask)
        ms = (ctypes.c_double * 5)()
        L.check(lib.fc_mt_perm_timing(1, ms), "fc_mt_perm_timing")
        if best is None or sum(ms) < sum(best):
            best = list(ms)
    L.check(lib.fc_mt_perm_timing(0, None), "fc_mt_perm_timing")
    _, _, fallback, consumed = R.end_state()
    assert fallback == 0
    total = sum(best)
    print(f"n={n} k={k}: " + ", ".join(f"{s} {t:.3f}" for s, t in zip(STAGES, best))
          + f" ms; row {total:.3f} ms = {4.0 * n / total / 1e6:.2f} GB/s of gradient; "
          f"{consumed / (reps + 1) / n:.4f} outputs per element", flush=True)


class Cl:
    def __init__(self, i, g, C):
        self.client_id, self.grad, self.C = i, g, C


def rate(grads, on, reps):
    n, M = len(grads[0]), len(grads)
    agg = Aggregator({"aggregation_scheme": "fed_avg", "device_permutation": on})
    C = Compression({"compression_function": "rand", "fraction_coordinate": 0.1})
    best, out = 1e9, None
    for _ in range(reps):
        np.random.seed(1)
        t = time.perf_counter()
        agg.aggregate_grads([Cl(i, g, C) for i, g in enumerate(grads)])
        best = min(best, time.perf_counter() - t)
        out = (agg.agg_grad.tobytes(), int(np.random.randint(0, 2 ** 31 - 1)))
    print(f"Aggregator numpy->numpy rand x {M}, device_permutation={on} ({agg.agg_draws}): "
          f"{best:.3f} s = {4.0 * n * M / best / 1e9:.2f} GB/s of client gradients", flush=True)
    return 4.0 * n * M / best / 1e9, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=25_557_032)
    ap.add_argument("--clients", type=int, default=32)
    ap.add_argument("--stages-only", action="store_true")
    args = ap.parse_args()
    for n in (16 * 1024 * 1024, args.n):
        for k in (n // 10, n):
            stage_times(n, k)
    if args.stages_only:
        return
    rng = np.random.default_rng(0)
    grads = [rng.standard_normal(args.n, dtype=np.float32) for _ in range(args.clients)]
    on, a = rate(grads, True, 3)
    off, b = rate(grads, False, 1)
    print(f"on / off = {on / off:.1f}x; results and RNG equal: {a == b}", flush=True)


if __name__ == "__main__":
    main()
