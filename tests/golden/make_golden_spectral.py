"""Golden vectors for gar.SpectralGram against the reference's analytic SpectralFedAvg branch
(build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_spectral.py

Runs the REFERENCE (read-only /root/reference; ``import ftl.agents`` first):
``fast_lr_decomposition`` (spectral_aggregation.py:87-130) followed by ``weighted_average``
(gar.py:32-46), i.e. ``conventional_pca_aggregation`` (gar.py:123-134), on the seven oracle
'top' rows of the Aggregator tests (``round_rows``: seed 20261020, N = 3 * 8192 + 5, f = 0.25),
with ``np.random.seed`` called before each run, for five settings of (rank, adaptive_rank_th,
drop_top_comp).  Stored per setting: the reference's aggregate and S, the same aggregate from
an exact dense float64 SVD, and e_ref = max|agg_ref - agg_exact| / max|agg_exact| (the
reference computes in float32 with a randomized SVD: its own distance to the exact result is
the yardstick of the test).  Only results are written (``golden_spectral.NN.npz`` +
``manifest_spectral.json``); the rows are regenerated from the seed.
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import sys

import numpy as np

from npz_parts import save_parts

sys.dont_write_bytecode = True
REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

SEED, N, FRAC = 20261020, 3 * 8192 + 5, 0.25
SETTINGS = [(7, 0.95, False), (3, 0, False), (7, 0.95, True), (4, 0.5, True), (7, 0, True)]


def round_rows():
    """The oracle's 'top' rows of the Aggregator tests' seven clients (float32, M x N)."""
    from oracle import compression_oracle as co
    rng = np.random.default_rng(SEED)
    base = rng.standard_normal(N)
    rows = []
    for i in range(7):
        noise = rng.standard_normal(N)
        g = 5.0 * noise if i == 2 else -3.0 * base if i == 6 else base + 0.3 * noise
        rows.append(co.compress({"compression_function": "top", "fraction_coordinate": FRAC},
                                g.astype(np.float32)))
    return np.stack(rows)


def exact_aggregate(R, rank, th, drop):
    """The reference's algorithm on an exact float64 SVD of the rows."""
    X = R.astype(np.float64).T
    M = R.shape[0]
    if not rank or rank > min(X.shape):
        rank = min(X.shape)
    U, S, V = np.linalg.svd(X, full_matrices=False)
    U, S, V = U[:, :rank], S[:rank], V[:rank]
    U_k, S_k, V_k = U, S, V
    if th:
        ns = X.shape[0]
        ratio = (S ** 2) / (ns - 1) / np.var(X, ddof=1, axis=0).sum()
        ar = int(np.searchsorted(np.cumsum(ratio), th))
        if ar == 0:
            ar += 2 if drop else 1
        U_k, S_k, V_k = U[:, :ar], S[:ar], V[:ar]
    if drop:
        U_k, S_k, V_k = U_k[:, 1:], S_k[1:], V_k[1:]
    lr = ((U_k * S_k) @ V_k).T
    w = np.full(M, 1.0 / M, dtype=np.float32).astype(np.float64)
    return w @ lr, S


def main():
    sys.path.insert(0, REF)
    import ftl.agents  # noqa: F401  (import-order requirement)
    from ftl.gradient_aggregation.gar import FedAvg
    from ftl.gradient_aggregation.spectral_aggregation import fast_lr_decomposition
    R = round_rows()
    arrays, cases = {}, {}
    for rank, th, drop in SETTINGS:
        name = f"rank{rank}__th{th}__drop{int(drop)}"
        np.random.seed(SEED)
        with contextlib.redirect_stdout(io.StringIO()):
            G_approx, S = fast_lr_decomposition(X=R, rank=rank, adaptive_rank_th=th, drop_top_comp=drop)
            agg = FedAvg({"aggregation_scheme": "fed_avg"}).weighted_average(stacked_grad=G_approx)
        exact, S_exact = exact_aggregate(R, rank, th, drop)
        top = float(np.max(np.abs(exact)))
        e_ref = float(np.max(np.abs(agg.astype(np.float64) - exact)) / top) if top > 0 else 0.0
        arrays[f"{name}|agg_ref"] = np.asarray(agg)
        arrays[f"{name}|S_ref"] = np.asarray(S)
        arrays[f"{name}|agg_exact"] = exact
        cases[name] = {"rank": rank, "adaptive_rank_th": th, "drop_top_comp": drop, "e_ref": e_ref,
                       "agg_ref_dtype": str(np.asarray(agg).dtype), "max_abs_exact": top,
                       "S_rel_err_ref": float(np.max(np.abs(np.asarray(S, np.float64) - S_exact) / S_exact))}
        print(name, cases[name])
    save_parts(OUT, "golden_spectral", arrays)      # golden_spectral.NN.npz, each below 1 MiB
    with open(os.path.join(OUT, "manifest_spectral.json"), "w") as fh:
        json.dump({"seed": SEED, "n": N, "fraction": FRAC, "clients": 7, "cases": cases}, fh,
                  indent=1, sort_keys=True)
    print(f"wrote {len(cases)} spectral cases")


if __name__ == "__main__":
    main()
