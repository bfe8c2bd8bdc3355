#!/usr/bin/env python3
"""Time ET-PECNet and ET-LBEBM inference over each test split (the seeded weights of tests/golden/g24_pecnet.npz,
descriptors of G2) three ways:

  split   EigenTrajectory.evaluate_split: projection -> et_pecnet_forward_scenes / et_lbebm_forward_scenes -> fused metrics
  hook    the default per-scene path with the native module: EigenTrajectory.evaluate once per scene (bridge pre-hook with
          an all-ones scene_mask, predict = et_pecnet_predict / et_lbebm_predict, post-hook, metrics)
  torch   the predictor's chain alone, written here with torch.nn.functional.linear (rocBLAS) on the same whole-split
          inputs, against ``scenes_ms``, the native predictor launches alone

    python tools/time_pecnet.py [--reps 5] [--splits eth,hotel,univ,zara1,zara2]

Prints one JSON line per predictor and split (median wall ms, with a device synchronisation at both ends)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def chain(mlp, x):
    for i, lin in enumerate(mlp.layers):
        x = F.linear(x, lin.weight, lin.bias)
        if i + 1 < len(mlp.layers):
            x = torch.relu(x)
    return x


def torch_scenes(net, kind, C_obs, nrm, sse):
    """the whole split with torch: the encoders and the predictor once over all rows, the pooling scene by scene"""
    ori = torch.cat([nrm[:2, s:e] - nrm[:2, s:e].mean(dim=1, keepdim=True) for s, e in sse], dim=1).T
    feat = torch.cat([chain(net.encoder_past, C_obs.T), chain(net.encoder_dest, ori)] + ([ori] if kind == "pecnet" else []), dim=1)
    for _ in range(net.nonlocal_pools if kind == "pecnet" else 0):
        th, ph, g = chain(net.non_local_theta, feat), chain(net.non_local_phi, feat), chain(net.non_local_g, feat)
        pooled = [F.normalize(torch.softmax(th[s:e] @ ph[s:e].T, dim=-1), p=1, dim=1) @ g[s:e] for s, e in sse]
        feat = torch.cat(pooled) + feat
    return chain(net.predictor, feat)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--splits", default="eth,hotel,univ,zara1,zara2")
    args = ap.parse_args()
    from eigentrajectory_amd import EigenTrajectory, ops
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    from tests import _golden as G
    from tests import _pecnet_np as PN
    z, g2 = G.load("g24_pecnet.npz"), G.load("g2_fit_all_scenes.npz")
    dev = torch.device("cuda:0")
    for kind in ("pecnet", "lbebm"):
        native = PN.native_module(kind)
        native.load_state_dict({k: torch.from_numpy(v) for k, v in PN.weights(z, kind).items()}, strict=True)
        forward_scenes = ops.pecnet_forward_scenes if kind == "pecnet" else ops.lbebm_forward_scenes
        for scene in args.splits.split(","):
            hp = default_hyper_params(static_dist=G.static_dist(scene))
            model = EigenTrajectory(native, get_hook_func(kind), hp)
            msd = model.state_dict()
            for k in msd:
                if k.startswith("ET_"):
                    msd[k] = torch.from_numpy(g2[f"{scene}.{k}"])
            model.load_state_dict(msd)
            model = model.to(dev).eval()
            obs_np, pred_np, sse = G.dataset(scene, "test")
            obs, pred = torch.from_numpy(obs_np).to(dev), torch.from_numpy(pred_np).to(dev)
            scenes = [(obs[s:e].contiguous(), pred[s:e].contiguous(),
                       {"scene_mask": torch.ones((e - s, e - s), dtype=torch.bool, device=dev), "num_samples": 20}) for s, e in sse]
            sizes = (sse[:, 1] - sse[:, 0]).tolist()
            U_obs_m, _, U_obs_s, _ = model._U()
            C_obs, _, nrm, _ = ops.norm_project(obs, None, U_obs_m, None, U_obs_s, None, ops.MODE_SPLIT, model.static_dist,
                                                want_flag=False)

            def per_scene():
                with torch.no_grad():
                    for o, p, info in scenes:
                        model.evaluate(o, p, addl_info=info)

            def with_torch():
                with torch.no_grad():
                    return torch_scenes(model.baseline_model, kind, C_obs, nrm, sse.tolist())

            mine = forward_scenes(model.baseline_model, C_obs, nrm, scene_sizes=sizes)
            ref = with_torch().view(-1, 6, 20).permute(1, 0, 2)
            rec = {"predictor": kind, "split": scene, "scenes": len(sse), "pedestrians": int(obs.shape[0]),
                   "max_scene": int(max(sizes)), "torch_diff": float((mine - ref).abs().max() / ref.abs().max()),
                   "split_ms": timed(lambda: model.evaluate_split(obs, pred, sse), args.reps),
                   "scenes_ms": timed(lambda: forward_scenes(model.baseline_model, C_obs, nrm, scene_sizes=sizes), args.reps),
                   "torch_ms": timed(with_torch, args.reps),
                   "hook_ms": timed(per_scene, args.reps)}
            rec["hook_over_split"] = rec["hook_ms"] / rec["split_ms"]
            rec["torch_over_scenes"] = rec["torch_ms"] / rec["scenes_ms"]
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
