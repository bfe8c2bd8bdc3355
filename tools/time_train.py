#!/usr/bin/env python3
"""Time one sequenced training group of a natively trained predictor on eth's first training scenes at the reference's
batch_size = 128 (one optimiser step: 128 scenes, each its own forward, losses and backward -- and its own DropEdge draw
where the predictor has one -- then gradient clipping and AdamW), two ways, in one process:

  native  the predictor after ``eigentrajectory_amd.enable_native_training`` (PREDICTORS below: its launches per scene)
  twin    the same weights in stock torch operators under torch autograd (tests/_*_twin.py: the draw,
          ``F.batch_norm(training=True)``, GP-Graph's merge loop on the host, Social-Implicit's ``bool(any)`` host
          synchronisation per scene and zone included); everything around the predictor identical

    python tools/time_train.py --predictor {stgcnn,sgcn,gpgraph_sgcn,dmrgcn,implicit,graphtern} [--scenes 128] [--reps 5]

A sample is ONE group between two device synchronisations; the two variants alternate sample by sample and the figure is
the median of ``--reps`` samples after one warm-up sample each.  Also timed, per group of the same scenes:
  predictor_ms       the predictor alone: forward + backward from a fixed output gradient per scene, gradients
                     accumulating into .grad as in training
  native_kernels_ms  the native launches per scene called directly (under a fixed mask; no draw, no autograd, nothing
                     accumulated)
  accumulate_ms      (not graphtern) one ``.grad.add_(g)`` per used parameter and scene and nothing else (sgcn 97, gpgraph_sgcn
                     103, implicit 76 = 4 cells x 19 tensors): what autograd's per-parameter gradient accumulation launches
                     from the second scene of a group on
Prints one JSON line.  Descriptors and anchors are G2's (tests/golden); the weights are the predictor's
tests/_*_train_cases.module("et").  gpgraph_sgcn: the threshold is chosen by that file's rule on all the group's scenes
together (about half as many close pairs as pedestrians), so that the grouping is not degenerate: the number of groups G
sets the size of the pooled pass and the length of the twin's merge loop, and its distribution over the scenes is part of
the result (``threshold``, ``groups``).  Needs a HIP device; reads nothing outside the repository."""
import argparse
import importlib
import json
import os
import sys
import time
from typing import Callable, NamedTuple, Optional

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


class Predictor(NamedTuple):
    """What differs between the predictors.  ``x`` below is one scene's network input as ``clone`` kept it."""
    hook: str             # get_hook_func's name
    tests: str            # the cases are tests/_{tests}_train_cases, the twin tests/_{tests}_twin
    clone: Callable       # the bridge's network input -> x: what the predictor reads, detached and cloned
    n_of: Callable        # x -> the scene's pedestrians
    d_out: Callable       # (hp, n, dev) -> the fixed gradient at the predictor's output
    out: Callable         # the predictor's return value -> the output tensor
    kernels: Callable     # (net, x, n, g, keep): the direct ops calls of one scene, its workspace included
    accumulate: Optional[Callable]  # (net, dev) -> (the parameters autograd accumulates into, a gradient for each), or None
    draws: bool = False   # DropEdge: kernels_ms runs under one fixed mask per scene size
    rezero: bool = True   # accumulate_ms: every sample starts from fresh zero .grad tensors
    kernels_share: bool = True      # the JSON line has kernels_share_of_native_predictor
    extra: Optional[Callable] = None  # (trainers, vs) -> further JSON entries, after setting the predictors up for the scenes


def _pair(net_in):
    return net_in[0].detach().clone(), net_in[1].detach().clone()


def _graph_d_out(hp, n, dev):
    return torch.randn((1, hp.num_samples, hp.k, n), device=dev)


def _stgcnn_kernels(net, x, n, g, keep):
    ws = ops.stgcnn_train_workspace(net, n)
    ops.stgcnn_train_forward_graph(net, *x, ws)
    ops.stgcnn_backward_graph(net, ws, g)


def _sgcn_kernels(net, x, n, g, keep):
    ws = ops.sgcn_train_workspace(net, n)
    ops.sgcn_train_forward_graph(net, *x, ws)
    ops.sgcn_backward_graph(net, x[1], ws, g)


def _gpgraph_kernels(net, x, n, g, keep):
    ws = ops.gpgraph_sgcn_train_workspace(net, n)
    ops.gpgraph_sgcn_train_forward_graph(net, *x, ws)
    ops.gpgraph_sgcn_backward_graph(net, ws, g)


def _dmrgcn_kernels(net, x, n, g, keep):
    ws = ops.dmrgcn_train_workspace(net, n)
    ops.dmrgcn_train_forward_graph(net, *x, ws, keep=keep)
    ops.dmrgcn_backward_graph(net, ws, g)


def _implicit_kernels(net, x, n, g, keep):
    ws = ops.implicit_workspace(net, n)
    ops.implicit_forward_graph(net, *x, workspace=ws)
    ops.implicit_backward_graph(net, *x, ws, g)


def _graphtern_kernels(net, x, n, g, keep):
    ws = ops.graphtern_train_workspace(net, n)
    ops.graphtern_train_forward_graph(net, *x, ws, keep=keep)
    ops.graphtern_backward_graph(net, ws, g)


def _flat_accumulate(grad_views, unused=lambda net: ()):
    """every parameter but ``unused(net)``, with its view of one random flat gradient buffer"""
    def make(net, dev):
        skip = unused(net)
        views = grad_views(net, torch.randn((sum(p.numel() for p in net.parameters()),), device=dev))
        named = [(k, p) for k, p in net.named_parameters() if k not in skip]
        return [p for _, p in named], [views[k] for k, _ in named]
    return make


def _implicit_accumulate(net, dev):
    """the four cells' parameters (noise_w included), zeroed once: they are not what predictor_ms resets"""
    params = net.cell_parameters()
    for p in params:
        p.grad = torch.zeros_like(p)
    views = ops.implicit_grad_views(net, torch.randn((4, ops.implicit_grad_size(net.et_params()[0])), device=dev))
    return params, [views.get(k, torch.zeros(1, device=dev)) for k in net.cell_parameter_names()]


def _gpgraph_threshold(trainers, vs):
    """the threshold of this group of scenes, written into both predictors; then every scene's number of groups"""
    from tests import _gpgraph_np as GN
    from tests import _gpgraph_train_cases as CS
    _, rest = GN.split_state(CS.state("et"))
    th = float(CS.threshold_of([GN.distances(rest, va[0, 0].cpu().numpy()) for va, _ in vs]))
    for tr in trainers.values():
        with torch.no_grad():
            getattr(tr.predictor, "net", tr.predictor).group_gen.th.fill_(th)   # (the twin holds the module as .net)
    n_groups = []
    with torch.no_grad():
        trainers["native"].predictor.eval()
        for va, vr in vs:
            n_groups.append(int(trainers["native"].predictor(va, vr)[1].max()) + 1)
        trainers["native"].predictor.train()
    peds = [va.shape[3] for va, _ in vs]
    return dict(threshold=round(th, 6),
                groups=dict(min=int(min(n_groups)), median=float(np.median(n_groups)), max=int(max(n_groups)),
                            total=int(sum(n_groups)), scenes_with_one_group=int(sum(g == 1 for g in n_groups)),
                            scenes_ungrouped=int(sum(g == n for g, n in zip(n_groups, peds))),
                            groups_over_pedestrians=round(sum(n_groups) / sum(peds), 3)))


PREDICTORS = {
    # forward = 2 launches, backward = 2 launches per scene (csrc/et_stgcnn_train.hip); a scene occupies one CU
    "stgcnn": Predictor("stgcnn", "stgcnn", _pair, lambda x: x[0].shape[3], _graph_d_out, lambda o: o, _stgcnn_kernels,
                        _flat_accumulate(ops.stgcnn_grad_views, lambda net: net.unused_parameter_names())),
    # forward = 6 + 7 launches, backward = 7 + 8 launches per scene (csrc/et_sgcn_train.inl); x = (graph, identities)
    "sgcn": Predictor("sgcn", "sgcn", lambda net_in: (net_in[0].detach().clone(), [t.detach().clone() for t in net_in[1]]),
                      lambda x: x[0].shape[2], lambda hp, n, dev: torch.randn((hp.k, n, hp.num_samples), device=dev),
                      lambda o: o, _sgcn_kernels, _flat_accumulate(ops.sgcn_grad_views)),
    # forward = 8 + 7 launches, backward = 7 + 13 launches per scene (csrc/et_gpgraph_train.inl on csrc/et_sgcn_train.inl)
    "gpgraph_sgcn": Predictor("gpgraphsgcn", "gpgraph", _pair, lambda x: x[0].shape[3], _graph_d_out, lambda o: o[0],
                              _gpgraph_kernels, _flat_accumulate(ops.gpgraph_sgcn_grad_views), extra=_gpgraph_threshold),
    # the draw, forward = 1 launch, backward = 3 launches per scene (csrc/et_dmrgcn_train.hip)
    "dmrgcn": Predictor("dmrgcn", "dmrgcn", _pair, lambda x: x[0].shape[3], _graph_d_out, lambda o: o[0], _dmrgcn_kernels,
                        _flat_accumulate(ops.dmrgcn_grad_views), draws=True),
    # forward = 2 launches, backward = 2 launches per scene (csrc/et_implicit.hip); d_out is the post-hook's view
    "implicit": Predictor("implicit", "implicit", lambda net_in: (net_in[0].detach().clone(),), lambda x: x[0].shape[-1],
                          lambda hp, n, dev: torch.randn((hp.k, n, hp.num_samples), device=dev).permute(2, 0, 1)[None],
                          lambda o: o, _implicit_kernels, _implicit_accumulate, rezero=False, kernels_share=False),
    # the draw, forward = 1 launch, backward = 3 launches per scene (csrc/et_graphtern_train.hip)
    "graphtern": Predictor("graphtern", "graphtern", lambda net_in: (net_in[0].detach().clone(),), lambda x: x[0].shape[3],
                           lambda hp, n, dev: torch.randn((1, hp.k, n, hp.num_samples), device=dev), lambda o: o,
                           _graphtern_kernels, None, draws=True),
}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--predictor", required=True, choices=list(PREDICTORS))
    ap.add_argument("--scenes", type=int, default=128, help="scenes of one group (the reference's batch_size)")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_train.py needs a HIP device: a CPU run measures nothing")
    P = PREDICTORS[a.predictor]
    CS = importlib.import_module(f"tests._{P.tests}_train_cases")
    TW = importlib.import_module(f"tests._{P.tests}_twin")
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
        hooks = get_hook_func(P.hook)
        if name == "native":
            call = hooks.model_forward

            def forward(net_in, baseline_model, call=call):
                inputs.append(P.clone(net_in))
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
        torch.nn.utils.clip_grad_norm_(tr.predictor.parameters(), hp.clip_grad)   # (skips a parameter without .grad)
        tr.optimizer.step()
        return loss

    step(trainers["native"])  # collects every scene's network input as the bridge builds it
    vs = inputs[:len(batch)]
    inputs.clear()
    trainers["native"].model.hook_func.model_forward = get_hook_func(P.hook).model_forward
    ns = [P.n_of(x) for x in vs]
    gs = [P.d_out(hp, n, dev) for n in ns]
    extra = P.extra(trainers, vs) if P.extra else {}

    def predictor_only(tr):
        for p in tr.predictor.parameters():
            p.grad = None
        for x, g in zip(vs, gs):
            P.out(tr.predictor(*x)).backward(g)

    net = trainers["native"].predictor
    keeps = {n: net.draw_keep(n, dev) if P.draws else None for n in set(ns)}

    def kernels_only(tr):
        for x, n, g in zip(vs, ns, gs):
            P.kernels(net, x, n, g, keeps[n])

    plan = [("step_ms", step, ("native", "twin")), ("predictor_ms", predictor_only, ("native", "twin")),
            ("kernels_ms", kernels_only, ("native",))]
    if P.accumulate:
        params, add = P.accumulate(net, dev)

        def accumulate_only(tr):
            if P.rezero:
                for p in params:
                    p.grad = torch.zeros_like(p)
            for _ in vs:
                for p, g in zip(params, add):
                    p.grad.add_(g)
        plan.append(("accumulate_ms", accumulate_only, ("native",)))

    def sample(fn, tr):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(tr)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    res = {}
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
    res.update(scenes=n_scenes, pedestrians=int(sum(ns)), reps=a.reps,
               step_ratio_twin_over_native=round(res["twin_step_ms"] / res["native_step_ms"], 3),
               predictor_ratio_twin_over_native=round(res["twin_predictor_ms"] / res["native_predictor_ms"], 3),
               native_step_ms_per_scene=round(res["native_step_ms"] / n_scenes, 4),
               native_predictor_ms_per_scene=round(res["native_predictor_ms"] / n_scenes, 4),
               native_kernels_ms_per_scene=round(res["native_kernels_ms"] / n_scenes, 4))
    if P.kernels_share:
        res.update(kernels_share_of_native_predictor=round(res["native_kernels_ms"] / res["native_predictor_ms"], 3))
    if P.accumulate:
        res.update(accumulate_ms_per_scene=round(res["native_accumulate_ms"] / n_scenes, 4),
                   accumulate_share_of_native_step=round(res["native_accumulate_ms"] / res["native_step_ms"], 3))
    res.update(**extra, device=torch.cuda.get_device_name(0))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
