#!/usr/bin/env python3
"""Times the t-SNE kernels (csrc/et_tsne.hip) with device events on eth train (29 809 rows of C_obs): affinities
(kNN + perplexity search + symmetrisation), one gradient evaluation (exact repulsion over all pairs), the whole
1 000-iteration optimisation, and the script's pipeline over the five splits.

    python tools/time_tsne.py [--reps 5] [--no-script]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

from eigentrajectory_amd import ops  # noqa: E402

VALU_FP32_PEAK = 157.3e12  # MI355X vector fp32 FLOP/s (MI355X_MICROARCH: 256 CUs x 2.4 GHz x 256 FLOP/clk)


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-script", action="store_true")
    args = ap.parse_args()
    import coeff_tsne as S
    dev = torch.device("cuda:0")
    obs, pred = S.load_train("eth", None, dev)
    C, _ = S.coefficients(obs, pred)
    n = C.shape[0]
    aff = ops.tsne_affinities(C)
    torch.cuda.synchronize()
    t_aff, aff = timed(lambda: ops.tsne_affinities(C), args.reps)
    Y = ops.tsne_pca_init(C)
    P32 = aff["P"].float()
    t_grad, _ = timed(lambda: ops.tsne_kl_grad(Y, aff["indptr"], aff["indices"], P32, want_kl=False), args.reps * 4)
    lr = float(np.maximum(n / 12.0 / 4, 50))
    t_opt, (_, kl, it) = timed(lambda: ops.tsne_optimize(Y, aff["indptr"], aff["indices"], aff["P"], 12.0, lr, 1000), 2)
    pairs = float(n) * (n - 1)
    print(f"eth train N={n} nnz={aff['P'].numel()}")
    print(f"affinities (kNN k=91 + perplexity + symmetrisation): {t_aff:.2f} ms")
    print(f"one gradient (exact repulsion, {pairs:.3g} pairs): {t_grad:.3f} ms = {pairs / t_grad * 1e3:.3g} pairs/s "
          f"(~20 fp32 VALU ops a pair: {20 * pairs / t_grad * 1e3 / VALU_FP32_PEAK * 2:.1%} of the FMA-counted peak)")
    print(f"optimisation, 1 000 iterations: {t_opt:.1f} ms ({t_opt / (it + 1):.3f} ms an iteration incl. update; "
          f"KL {kl:.4f}, n_iter {it})")
    if not args.no_script:
        t0 = time.perf_counter()
        for scene in S.SCENES:
            o, p = S.load_train(scene, None, dev)
            t1 = time.perf_counter()
            r = S.run_scene(o, p)
            torch.cuda.synchronize()
            print(f"  {scene}: N={o.shape[0]} KL {r['kl']:.4f} n_iter {r['n_iter']} "
                  f"clusters {len(np.unique(r['labels']))}: {time.perf_counter() - t1:.2f} s")
        print(f"script pipeline, five splits (coefficients + K-means + t-SNE): {time.perf_counter() - t0:.2f} s")


if __name__ == "__main__":
    main()
