#!/usr/bin/env python3
"""Time ET-STGCNN inference over each test split (weights of tests/golden/g19_stgcnn.npz) three ways:

  split   EigenTrajectory.evaluate_split: projection -> et_stgcnn_forward_scenes -> fused metrics, 3 launches per split
  hook    the default per-scene path with the native module: EigenTrajectory.evaluate once per scene (bridge pre-hook,
          SocialSTGCNN.forward = et_stgcnn_forward_graph, metrics)
  torch   the same per-scene path with a torch network of the reference's shape (the same weights, torch operators)

    python tools/time_stgcnn.py [--reps 5] [--splits eth,hotel,univ,zara1,zara2]

Prints one JSON line per split (median wall ms per whole split, with a device synchronisation at both ends)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)


class TorchSTGCNN(nn.Module):
    """The eval-mode forward of a SocialSTGCNN in torch operators (the reference network's shape), on its modules."""

    def __init__(self, native):
        super().__init__()
        self.m = native

    def forward(self, v, a):
        m = self.m
        for blk in m.st_gcns:
            res = v if blk.residual is None else blk.residual(v)
            x = blk.gcn.conv(v)
            n, kc, t, w = x.shape
            x = x.view(n, blk.gcn.kernel_size, kc // blk.gcn.kernel_size, t, w)
            x = torch.einsum("nkctv,kvw->nctw", (x, a)).contiguous()
            v = blk.prelu(blk.tcn(x) + res)
        v = v.view(v.shape[0], v.shape[2], v.shape[1], v.shape[3])
        v = m.prelus[0](m.tpcnns[0](v))
        for j in range(1, m.n_txpcnn - 1):
            v = m.prelus[j](m.tpcnns[j](v)) + v
        v = m.tpcnn_ouput(v)
        return v.view(v.shape[0], v.shape[2], v.shape[1], v.shape[3])


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
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.stgcnn import SocialSTGCNN
    from eigentrajectory_amd.utils import default_hyper_params
    from tests import _golden as G
    z = G.load("g19_stgcnn.npz")
    dev = torch.device("cuda:0")
    sd = {k[4:]: torch.from_numpy(np.array(z[k])) for k in z.files if k.startswith("net.")}
    for scene in args.splits.split(","):
        hp = default_hyper_params(static_dist=float(z[f"{scene}.static_dist"]))
        native = SocialSTGCNN(n_stgcnn=1, n_txpcnn=5, input_feat=1, output_feat=20, seq_len=8, pred_seq_len=6)
        native.load_state_dict(sd)
        model = EigenTrajectory(native, get_hook_func("stgcnn"), hp)
        msd = model.state_dict()
        for k in msd:
            if k.startswith("ET_"):
                msd[k] = torch.from_numpy(z[f"{scene}.ET.{k}"])
        model.load_state_dict(msd)
        model = model.to(dev).eval()
        tmodel = EigenTrajectory(TorchSTGCNN(model.baseline_model), get_hook_func("stgcnn"), hp)
        tmodel.load_state_dict({("baseline_model.m." + k[15:]) if k.startswith("baseline_model.") else k: v
                                for k, v in model.state_dict().items()})
        tmodel = tmodel.to(dev).eval()
        obs_np, pred_np, sse = G.dataset(scene, "test")
        obs, pred = torch.from_numpy(obs_np).to(dev), torch.from_numpy(pred_np).to(dev)
        scenes = [(obs[s:e].contiguous(), pred[s:e].contiguous()) for s, e in sse]

        def per_scene(m):
            def run():
                with torch.no_grad():
                    for o, p in scenes:
                        m.evaluate(o, p)
            return run

        rec = {"split": scene, "scenes": len(sse), "pedestrians": int(obs.shape[0]),
               "max_scene": int((sse[:, 1] - sse[:, 0]).max()),
               "split_ms": timed(lambda: model.evaluate_split(obs, pred, sse), args.reps),
               "hook_ms": timed(per_scene(model), args.reps),
               "torch_ms": timed(per_scene(tmodel), args.reps)}
        rec["hook_over_split"] = rec["hook_ms"] / rec["split_ms"]
        rec["torch_over_split"] = rec["torch_ms"] / rec["split_ms"]
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
