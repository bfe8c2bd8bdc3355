#!/usr/bin/env python3
"""Time one sequenced training group of ET-DMRGCN on eth's first training scenes at the reference's batch_size = 128 (one
optimiser step: 128 scenes, each its own DropEdge draw, forward, losses and backward, then gradient clipping and AdamW), two
ways, in one process:

  native  SocialDMRGCN after ``eigentrajectory_amd.enable_native_training``: the draw, forward = 1 launch, backward = 3
          launches per scene (csrc/et_dmrgcn_train.hip)
  twin    the same weights in stock torch operators under torch autograd, the draw included (tests/_dmrgcn_twin.py);
          everything around the predictor identical

    python tools/time_dmrgcn_train.py [--scenes 128] [--reps 5]

A sample is ONE group between two device synchronisations; the two variants alternate sample by sample and the figure is
the median of ``--reps`` samples after one warm-up sample each.  Also timed, per group of the same scenes:
  predictor_ms       the predictor alone: forward(v, a) + backward from a fixed output gradient per scene, gradients
                     accumulating into .grad as in training
  native_kernels_ms  the native launches per scene called directly under a fixed mask (no draw, no autograd, nothing
                     accumulated)
  accumulate_ms      one ``.grad.add_(g)`` per parameter and scene and nothing else: what autograd's per-parameter gradient
                     accumulation launches from the second scene of a group on
Prints one JSON line.  Descriptors and anchors are G2's (tests/golden); the weights are tests/_dmrgcn_train_cases.module("et").
Needs a HIP device."""
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
from tests import _dmrgcn_train_cases as CS  # noqa: E402
from tests import _dmrgcn_twin as TW  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", type=int, default=128, help="scenes of one group (the reference's batch_size)")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_dmrgcn_train.py needs a HIP device: a CPU run measures nothing")
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
        hooks = get_hook_func("dmrgcn")
        if name == "native":
            call = hooks.model_forward

            def forward(net_in, baseline_model, call=call):
                inputs.append((net_in[0].detach().clone(), net_in[1].detach().clone()))
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
        torch.nn.utils.clip_grad_norm_(tr.predictor.parameters(), hp.clip_grad)
        tr.optimizer.step()
        return loss

    step(trainers["native"])  # collects every scene's v and a as the bridge builds them
    vs = inputs[:len(batch)]
    inputs.clear()
    trainers["native"].model.hook_func.model_forward = get_hook_func("dmrgcn").model_forward
    gs = [torch.randn((1, hp.num_samples, hp.k, v.shape[3]), device=dev) for v, _ in vs]

    def predictor_only(tr):
        for p in tr.predictor.parameters():
            p.grad = None
        for (v, adj), g in zip(vs, gs):
            tr.predictor(v, adj)[0].backward(g)

    net = trainers["native"].predictor
    keeps = {n: net.draw_keep(n, dev) for n in {v.shape[3] for v, _ in vs}}

    def kernels_only(tr):
        for (v, adj), g in zip(vs, gs):
            ws = ops.dmrgcn_train_workspace(net, v.shape[3])
            ops.dmrgcn_train_forward_graph(net, v, adj, ws, keep=keeps[v.shape[3]])
            ops.dmrgcn_backward_graph(net, ws, g)

    unused = ()
    block = torch.randn((sum(p.numel() for p in net.parameters()),), device=dev)
    views = ops.dmrgcn_grad_views(net, block)
    params = [p for k, p in net.named_parameters() if k not in unused]
    add = [views[k] for k, _ in net.named_parameters() if k not in unused]

    def accumulate_only(tr):
        for p in params:
            p.grad = torch.zeros_like(p)
        for _ in vs:
            for p, g in zip(params, add):
                p.grad.add_(g)

    def sample(fn, tr):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(tr)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    res = {}
    plan = (("step_ms", step, ("native", "twin")), ("predictor_ms", predictor_only, ("native", "twin")),
            ("kernels_ms", kernels_only, ("native",)), ("accumulate_ms", accumulate_only, ("native",)))
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
    res.update(scenes=n_scenes, pedestrians=int(sum(v.shape[3] for v, _ in vs)), reps=a.reps,
               step_ratio_twin_over_native=round(res["twin_step_ms"] / res["native_step_ms"], 3),
               predictor_ratio_twin_over_native=round(res["twin_predictor_ms"] / res["native_predictor_ms"], 3),
               native_step_ms_per_scene=round(res["native_step_ms"] / n_scenes, 4),
               native_predictor_ms_per_scene=round(res["native_predictor_ms"] / n_scenes, 4),
               native_kernels_ms_per_scene=round(res["native_kernels_ms"] / n_scenes, 4),
               kernels_share_of_native_predictor=round(res["native_kernels_ms"] / res["native_predictor_ms"], 3),
               accumulate_ms_per_scene=round(res["native_accumulate_ms"] / n_scenes, 4),
               accumulate_share_of_native_step=round(res["native_accumulate_ms"] / res["native_step_ms"], 3),
               device=torch.cuda.get_device_name(0))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
