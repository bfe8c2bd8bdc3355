#!/usr/bin/env python3
"""Times the curve-fitting table (scripts/descriptor_evaluation.py --curves) per ETH/UCY test split on the GPU: all 28
fits of a split (14 bases x obs / pred) in one et_curve_fit_batch call (pass 1, best-step reduce, pass 2).

    python tools/time_curve_fit.py [--steps 100000] [--scenes eth,univ]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from eigentrajectory_amd import curve, ops  # noqa: E402
from tests import _golden as G  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100000)
    ap.add_argument("--scenes", default=",".join(G.SCENES))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    total = 0.0
    for scene in args.scenes.split(","):
        obs, pred, _ = G.dataset(scene, "test")
        obs, pred = torch.from_numpy(obs).to(dev), torch.from_numpy(pred).to(dev)
        ori, rot, _ = ops.norm_params(obs, want_sca=False)
        trajs, bases = [], []
        for tn in (ops.normalize(obs, ori, rot), ops.normalize(pred, ori, rot)):
            for _, _, b in curve.table_bases(tn.shape[1]):
                trajs.append(tn)
                bases.append(b.to(dev))
        curve.curve_fitting_batch(trajs, bases, steps=10)  # load / first-launch costs out of the timing
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, best, _ = curve.curve_fitting_batch(trajs, bases, steps=args.steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        total += dt
        b = best.cpu().numpy()
        print(f"{scene}: N={obs.shape[0]} 28 fits x {args.steps} steps: {dt * 1e3:.1f} ms "
              f"(best step min {b.min()} median {int(np.median(b))})", flush=True)
    print(f"total {total * 1e3:.1f} ms")


if __name__ == "__main__":
    main()
