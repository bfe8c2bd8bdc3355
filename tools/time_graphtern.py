#!/usr/bin/env python3
"""Time ET-Graph-TERN inference over each test split (weights of tests/golden/g27_graphtern.npz, descriptors of G2) two ways:

  split   EigenTrajectory.evaluate_split: projection -> et_graphtern_forward_scenes -> fused metrics, 3 launches per split
  hook    the default per-scene path with the native module: EigenTrajectory.evaluate once per scene (bridge pre-hook,
          GraphTERNLight.forward = et_graphtern_forward_graph, metrics)

    python tools/time_graphtern.py [--reps 5] [--splits eth,hotel,univ,zara1,zara2]

Prints one JSON line per split (median wall ms per whole split, with a device synchronisation at both ends; the
predictor's launch alone as ``scenes_ms``).  tools/time_dmrgcn.py is the comparator of like kind."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--splits", default="eth,hotel,univ,zara1,zara2")
    args = ap.parse_args()
    from eigentrajectory_amd import EigenTrajectory, ops
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.graphtern import GraphTERNLight
    from eigentrajectory_amd.utils import default_hyper_params
    from tests import _golden as G
    z, g2 = G.load("g27_graphtern.npz"), G.load("g2_fit_all_scenes.npz")
    dev = torch.device("cuda:0")
    sd = {k[4:]: torch.from_numpy(np.array(z[k])) for k in z.files if k.startswith("net.")}
    static_dist = G.manifest()["static_dist"]
    for scene in args.splits.split(","):
        hp = default_hyper_params(static_dist=float(static_dist[scene]))
        native = GraphTERNLight(n_epgcn=1, n_epcnn=6, input_feat=1, seq_len=8, pred_seq_len=6, n_smpl=20)
        native.load_state_dict(sd)
        model = EigenTrajectory(native, get_hook_func("graphtern"), hp)
        msd = model.state_dict()
        for k in msd:
            if k.startswith("ET_"):
                msd[k] = torch.from_numpy(g2[f"{scene}.{k}"])
        model.load_state_dict(msd)
        model = model.to(dev).eval()
        obs_np, pred_np, sse = G.dataset(scene, "test")
        obs, pred = torch.from_numpy(obs_np).to(dev), torch.from_numpy(pred_np).to(dev)
        scenes = [(obs[s:e].contiguous(), pred[s:e].contiguous()) for s, e in sse]
        sizes = (sse[:, 1] - sse[:, 0]).tolist()
        U_obs_m, _, U_obs_s, _ = model._U()
        C_obs, _, nrm, _ = ops.norm_project(obs, None, U_obs_m, None, U_obs_s, None, ops.MODE_SPLIT, model.static_dist,
                                            want_flag=False)

        def per_scene():
            with torch.no_grad():
                for o, p in scenes:
                    model.evaluate(o, p)

        rec = {"split": scene, "scenes": len(sse), "pedestrians": int(obs.shape[0]), "max_scene": int(max(sizes)),
               "scenes_in_lds": int(sum(s <= 35 for s in sizes)),
               "split_ms": timed(lambda: model.evaluate_split(obs, pred, sse), args.reps),
               "scenes_ms": timed(lambda: ops.graphtern_forward_scenes(model.baseline_model, C_obs, nrm, scene_sizes=sizes),
                                  args.reps),
               "hook_ms": timed(per_scene, args.reps)}
        rec["hook_over_split"] = rec["hook_ms"] / rec["split_ms"]
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
