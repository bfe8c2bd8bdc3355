#!/usr/bin/env python3
"""The reference's script/descriptor_evaluation.py (the paper's Table 1) on the HIP kernels, per ETH/UCY test split:
reconstruction error of the rank-k descriptor, k = 1..12 (the SVD block, :87-112), and with --curves first the
curve-fitting baselines (:38-85): Linear, Bezier degree 2..5 and B-spline degree 1..3 x n_curve 2..5 descriptors fitted
by Adam (100 000 steps by default; all 28 fits of a split in one launch per pass, csrc/et_curve.hip).

    python scripts/descriptor_evaluation.py --data tests/golden/data        # committed fixtures
    python scripts/descriptor_evaluation.py --raw <dir with eth/test/*.txt ...>
    python scripts/descriptor_evaluation.py --curves [--steps N]

The curve fits are chaotic in their last digits (the reference itself moves its 4th printed decimal under a 1-ulp
change of the input), so their entries agree with the reference's to within that spread, not digit for digit."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from eigentrajectory_amd import ops  # noqa: E402


def svd_table(obs, pred, ks=range(1, 13)):
    """-> (len(ks), 2) mean L2 errors (obs, pred) with TrajNorm(ori, rot, sca=False), like the reference."""
    g_obs, g_pred, _ = ops.fit_gram(obs, pred, ops.MODE_STATIC, which=0)
    out = []
    for k in ks:
        (U_obs, _), (U_pred, _) = ops.eigh_topk_batch([g_obs, g_pred], k)
        c_obs, c_pred, nrm, _ = ops.norm_project(obs, pred, None, None, U_obs, U_pred, ops.MODE_STATIC, want_flag=False)
        r_obs = ops.anchor_reconstruct(c_obs.unsqueeze(-1), None, None, None, U_obs, ops.MODE_STATIC, nrm=nrm)[0]
        r_pred = ops.anchor_reconstruct(c_pred.unsqueeze(-1), None, None, None, U_pred, ops.MODE_STATIC, nrm=nrm)[0]
        out.append([(r_obs - obs).norm(p=2, dim=-1).mean().item(), (r_pred - pred).norm(p=2, dim=-1).mean().item()])
    return np.asarray(out)


def curve_table(obs, pred, steps=100000):
    """-> [(kind, params, obs error, pred error)] for the 14 curve bases of curve.table_bases in the reference's order,
    TrajNorm(ori, rot, sca=False) computed on obs, errors measured after denormalisation like the reference."""
    from eigentrajectory_amd import curve
    ori, rot, _ = ops.norm_params(obs, want_sca=False)
    parts = [(obs, ops.normalize(obs, ori, rot)), (pred, ops.normalize(pred, ori, rot))]
    specs = [curve.table_bases(p.shape[1]) for p, _ in parts]
    trajs = [tn for _, tn in parts for _ in range(len(specs[0]))]
    bases = [b for sp in specs for _, _, b in sp]
    recons = curve.curve_fitting_batch(trajs, bases, steps=steps)[0]
    nb = len(specs[0])
    errs = [[(ops.denormalize(recons[j * nb + i], ori, rot) - parts[j][0]).norm(p=2, dim=-1).mean().item()
             for i in range(nb)] for j in range(2)]
    return [(kind, prm, errs[0][i], errs[1][i]) for i, (kind, prm, _) in enumerate(specs[0])]


def print_curve_table(rows, dim=2):
    heads = {"linear": "===Linear===", "bezier": "===Bezier Curve===", "bspline": "===B-Spline==="}
    last = None
    for kind, prm, eo, ep in rows:
        if kind != last:
            print(heads[kind])
            last = kind
        if kind == "linear":
            lead = f"num params: {2 * dim}"
        elif kind == "bezier":
            lead = f"degree: {prm[0]}\tnum params: {(prm[0] + 1) * dim}"
        else:
            lead = f"n_curve: {prm[0]}\tdegree: {prm[1]}\tnum params: {(prm[0] + 1) * dim}"
        print(f"{lead}\tobs error: {eo:.4f}\tpred error: {ep:.4f}")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default=None, help="directory with <scene>_test.npz fixtures (tests/golden/data)")
    ap.add_argument("--raw", default=None, help="dataset root with <scene>/test/*.txt")
    ap.add_argument("--curves", action="store_true", help="print the Linear / Bezier / B-spline blocks before the SVD block")
    ap.add_argument("--steps", type=int, default=100000, help="Adam steps per curve fit (the reference's 100 000)")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    return args


def main():
    args = parse_args()
    dev = torch.device("cuda:0")
    for scene in ["eth", "hotel", "univ", "zara1", "zara2"]:
        if args.raw:
            from eigentrajectory_amd.data import TrajectoryData
            d = TrajectoryData(os.path.join(args.raw, scene, "test"))
            obs, pred = d.obs_traj.to(dev), d.pred_traj.to(dev)
        else:
            root = args.data or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "data")
            z = np.load(os.path.join(root, f"{scene}_test.npz"))
            full = torch.from_numpy((z["q"].astype(np.float64) / 1e4).astype(np.float32)).to(dev)
            obs, pred = full[:, :8].contiguous(), full[:, 8:].contiguous()
        if args.curves:
            print(f"=== {scene} ({obs.shape[0]} pedestrians) ===curve fitting, {args.steps} steps===")
            print_curve_table(curve_table(obs, pred, args.steps))
        print(f"=== {scene} ({obs.shape[0]} pedestrians) ===Singular Value Decomposition===")
        for k, (eo, ep) in zip(range(1, 13), svd_table(obs, pred)):
            print(f"k: {k}\tnum params: {k}\tobs error: {eo:.4f}\tpred error: {ep:.4f}")


if __name__ == "__main__":
    main()
