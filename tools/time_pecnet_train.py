#!/usr/bin/env python3
"""Time one ETTrainer step (collated mode) of ET-PECNet in the ET configuration at ``--batch-size`` pedestrians in scenes of
32 (512 pedestrians: 16 scenes, one block mask), two ways, in one process:

  native  the PECNet module after ``eigentrajectory_amd.enable_native_training``: predict = 2 + 2 * 3 launches, its backward
          3 + 3 * 3 (csrc/et_mlp_train.hip)
  twin    the same module and weights with ``predict`` written as the reference's formula in stock torch operators under
          torch autograd (rocBLAS, softmax and elementwise launches), everything around it identical

    python tools/time_pecnet_train.py [--batch-size 512] [--reps 5] [--inner 20]

A step is what ETTrainer.train runs per batch: zero_grad, forward, the three losses, backward, gradient clipping, the AdamW
step.  Every sample is ``--inner`` consecutive steps between two device synchronisations, divided by ``--inner``; the two
variants alternate sample by sample, and the figure is the median of ``--reps`` samples after one warm-up sample each.
``predictor_ms`` is the predictor alone on the same batch: predict + backward from a fixed output gradient.  Prints one JSON
line.  Synthetic trajectories (seeded), descriptors and anchors fitted on them; needs a HIP device."""
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

from eigentrajectory_amd import EigenTrajectory, PECNet, enable_native_training  # noqa: E402
from eigentrajectory_amd.bridges import get_hook_func  # noqa: E402
from eigentrajectory_amd.data import TrajectoryData  # noqa: E402
from eigentrajectory_amd.synth import synthetic_trajectories_np  # noqa: E402
from eigentrajectory_amd.trainer import ETTrainer  # noqa: E402
from eigentrajectory_amd.utils import default_hyper_params  # noqa: E402


def chain(mlp, x):
    for i, lin in enumerate(mlp.layers):
        x = F.linear(x, lin.weight, lin.bias)
        if i + 1 < len(mlp.layers):
            x = torch.relu(x)
    return x


class TwinPECNet(PECNet):
    """``predict`` as stock torch operators under torch autograd: the yardstick"""

    def predict(self, past, generated_dest, mask, initial_pos):
        feat = torch.cat([chain(self.encoder_past, past), chain(self.encoder_dest, generated_dest), initial_pos], dim=1)
        for _ in range(self.nonlocal_pools):
            f = torch.matmul(chain(self.non_local_theta, feat), chain(self.non_local_phi, feat).transpose(1, 0))
            w = F.normalize(F.softmax(f, dim=-1) * mask, p=1, dim=1)
            feat = torch.matmul(w, chain(self.non_local_g, feat)) + feat
        return chain(self.predictor, feat)


def et_pecnet(cls, hp):
    """the ET configuration (config/eigentrajectory-pecnet-*.json)"""
    return cls([512, 256], [8, 16], [8, 50], [1024, 512, 1024], [1024, 512, 256], [256, 128, 64], [256, 128, 64],
               [256, 128, 64], 16, 16, 3, 128, 1.3, hp.k // 2, hp.k * hp.num_samples // 2 + 1, False)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_pecnet_train.py needs a HIP device: a CPU run measures nothing")
    dev = torch.device("cuda:0")
    n = a.batch_size
    per_scene = 32  # pedestrians per synthetic scene: batch_size / 32 scenes are collated into one batch
    sizes = [per_scene] * max(1, n // per_scene) if n >= per_scene else [n]
    obs, pred = synthetic_trajectories_np(sum(sizes), seed=0)
    ends = np.cumsum(sizes)
    data = TrajectoryData.from_arrays(obs, pred, [(int(e - s), int(e)) for e, s in zip(ends, sizes)])
    hp = default_hyper_params(static_dist=0.3, batch_size=sum(sizes), lr=1e-3, weight_decay=1e-4, clip_grad=10, lr_schd=False)

    torch.manual_seed(0)
    native = enable_native_training(et_pecnet(PECNet, hp))
    twin = et_pecnet(TwinPECNet, hp)
    twin.load_state_dict(native.state_dict())
    trainers = {}
    for name, net in (("native", native), ("twin", twin)):
        model = EigenTrajectory(net, get_hook_func("pecnet"), hp)
        tr = ETTrainer(model, hp, data, data, mode="collated", device=dev)
        if trainers:
            model.load_state_dict(trainers["native"].model.state_dict())  # the same descriptors, anchors and weights
        else:
            tr.init_descriptor()
        tr.model.train()
        trainers[name] = tr
    batch = list(range(len(data)))

    def step(tr):
        tr.optimizer.zero_grad(set_to_none=True)
        loss = tr._train_batch(tr.train_data, batch)
        torch.nn.utils.clip_grad_norm_(tr.predictor.parameters(), hp.clip_grad)
        tr.optimizer.step()
        return loss

    total = sum(sizes)
    past = torch.randn(hp.k, total, device=dev).T  # as the bridge hands them over
    dest = torch.randn(2, total, device=dev).T
    mask = torch.block_diag(*[torch.ones(s, s) for s in sizes]).to(dev)
    g_out = torch.randn(total, native.predictor.layers[-1].out_features, device=dev)

    def predictor_only(tr):
        for p in tr.predictor.parameters():
            p.grad = None
        tr.predictor.predict(past, dest, mask, dest).backward(g_out)

    def sample(fn, tr):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.inner):
            fn(tr)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.inner

    res = {}
    for what, fn in (("step_ms", step), ("predictor_ms", predictor_only)):
        ts = {name: [] for name in trainers}
        for rep in range(a.reps + 1):  # the first sample of each variant is the warm-up
            for name, tr in trainers.items():
                t = sample(fn, tr)
                if rep:
                    ts[name].append(t)
        for name in trainers:
            res[f"{name}_{what}"] = round(float(np.median(ts[name])), 4)
            res[f"{name}_{what}_min_max"] = [round(min(ts[name]), 4), round(max(ts[name]), 4)]
    res.update(batch_size=total, scenes=len(sizes), reps=a.reps, inner=a.inner,
               step_ratio_twin_over_native=round(res["twin_step_ms"] / res["native_step_ms"], 3),
               predictor_ratio_twin_over_native=round(res["twin_predictor_ms"] / res["native_predictor_ms"], 3),
               device=torch.cuda.get_device_name(0))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
