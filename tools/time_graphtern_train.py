#!/usr/bin/env python3
"""Time one sequenced training group of ET-Graph-TERN on eth's first training scenes at the reference's batch_size = 128
(one optimiser step: 128 scenes, each its own DropEdge draw, forward, losses and backward, then gradient clipping and
AdamW), two ways, in one process:

  native  GraphTERNLight after ``eigentrajectory_amd.enable_native_training``: the draw, forward = 1 launch, backward = 3
          launches per scene (csrc/et_graphtern_train.hip)
  twin    the same weights in stock torch operators under torch autograd, the draw included (tests/_graphtern_twin.py);
          everything around the predictor identical

    python tools/time_graphtern_train.py [--scenes 128] [--reps 5]

A sample is ONE group between two device synchronisations; the two variants alternate sample by sample and the figure is
the median of ``--reps`` samples after one warm-up sample each.  Also timed, per group of the same scenes:
  predictor_ms       the predictor alone: forward(S_obs) + backward from a fixed output gradient per scene, gradients
                     accumulating into .grad as in training
  native_kernels_ms  the native launches per scene called directly under a fixed mask (no draw, no autograd, nothing
                     accumulated)
Prints one JSON line.  Descriptors and anchors are G2's (tests/golden); the weights are
tests/_graphtern_train_cases.module("et").  Needs a HIP device; reads nothing outside the repository."""
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

from eigentrajectory_amd import EigenTrajectory, enable_native_training, ops  # noqa: E402
from eigentrajectory_amd.bridges import get_hook_func  # noqa: E402
from eigentrajectory_amd.data import TrajectoryData  # noqa: E402
from eigentrajectory_amd.trainer import ETTrainer  # noqa: E402
from eigentrajectory_amd.utils import default_hyper_params  # noqa: E402
from tests import _golden as G  # noqa: E402
from tests import _graphtern_train_cases as CS  # noqa: E402
from tests import _graphtern_twin as TW  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", type=int, default=128, help="scenes of one group (the reference's batch_size)")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_graphtern_train.py needs a HIP device: a CPU run measures nothing")
    dev = torch.device("cuda:0")
    obs, pred, sse = G.dataset("eth", "train")
    sse = sse[:a.scenes]
    data = TrajectoryData.from_arrays(obs[:sse[-1][1]], pred[:sse[-1][1]], [(int(s), int(e)) for s, e in sse])
    hp = default_hyper_params(static_dist=G.static_dist("eth"), batch_size=len(sse), lr=1e-3, weight_decay=1e-4, clip_grad=10,
                              lr_schd=False)
    g2 = G.load("g2_fit_all_scenes.npz")
    trainers, inputs = {}, []
    for name in ("native", "twin"):
        base = CS.module("et")
        hooks = get_hook_func("graphtern")
        if name == "native":
            call = hooks.model_forward

            def forward(net_in, baseline_model, call=call):
                inputs.append(net_in[0].detach().clone())
                return call(net_in, baseline_model)
            hooks.model_forward = forward
        model = EigenTrajectory(TW.Twin(base) if name == "twin" else base, hooks, hp)
        sd = model.state_dict()
        for k in sd:
            if k.startswith("ET_"):
                sd[k] = torch.from_numpy(g2[f"eth.{k}"])
        model.load_state_dict(sd)
        if name == "native":
            enable_native_training(model)
        tr = ETTrainer(model, hp, data, data, mode="sequenced", device=dev)
        tr.model.train()
        trainers[name] = tr
    batch = list(range(len(data)))

    def step(tr):
        tr.optimizer.zero_grad(set_to_none=True)
        loss = tr._train_batch(tr.train_data, batch)
        torch.nn.utils.clip_grad_norm_([p for p in tr.predictor.parameters() if p.grad is not None], hp.clip_grad)
        tr.optimizer.step()
        return loss

    step(trainers["native"])  # collects every scene's S_obs as the bridge builds it
    vs = inputs[:len(batch)]
    inputs.clear()
    trainers["native"].model.hook_func.model_forward = get_hook_func("graphtern").model_forward
    gs = [torch.randn((1, hp.k, s.shape[3], hp.num_samples), device=dev) for s in vs]

    def predictor_only(tr):
        for p in tr.predictor.parameters():
            p.grad = None
        for s, g in zip(vs, gs):
            tr.predictor(s).backward(g)

    net = trainers["native"].predictor
    keeps = {n: net.draw_keep(n, dev) for n in {s.shape[3] for s in vs}}

    def kernels_only(tr):
        for s, g in zip(vs, gs):
            ws = ops.graphtern_train_workspace(net, s.shape[3])
            ops.graphtern_train_forward_graph(net, s, ws, keep=keeps[s.shape[3]])
            ops.graphtern_backward_graph(net, ws, g)

    def sample(fn, tr):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(tr)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    res = {}
    plan = (("step_ms", step, ("native", "twin")), ("predictor_ms", predictor_only, ("native", "twin")),
            ("kernels_ms", kernels_only, ("native",)))
    for what, fn, names in plan:
        ts = {name: [] for name in names}
        for rep in range(a.reps + 1):  # the first sample of each variant is the warm-up
            for name in names:
                t = sample(fn, trainers[name])
                if rep:
                    ts[name].append(t)
        for name in names:
            res[f"{name}_{what}"] = round(float(np.median(ts[name])), 3)
            res[f"{name}_{what}_min_max"] = [round(min(ts[name]), 3), round(max(ts[name]), 3)]
    n_scenes = len(vs)
    res.update(scenes=n_scenes, pedestrians=int(sum(s.shape[3] for s in vs)), reps=a.reps,
               step_ratio_twin_over_native=round(res["twin_step_ms"] / res["native_step_ms"], 3),
               predictor_ratio_twin_over_native=round(res["twin_predictor_ms"] / res["native_predictor_ms"], 3),
               native_step_ms_per_scene=round(res["native_step_ms"] / n_scenes, 4),
               native_predictor_ms_per_scene=round(res["native_predictor_ms"] / n_scenes, 4),
               native_kernels_ms_per_scene=round(res["native_kernels_ms"] / n_scenes, 4),
               kernels_share_of_native_predictor=round(res["native_kernels_ms"] / res["native_predictor_ms"], 3),
               device=torch.cuda.get_device_name(0))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
