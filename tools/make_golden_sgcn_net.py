#!/usr/bin/env python3
"""G20: ET-SGCN inference fixture -- the reference's wrapper + its sgcn bridge + its SGCN (TrajectoryPredictor) with the
ET constructor arguments (utils/trainer.py:288-290: number_asymmetric_conv_layer=7, n_tcn=5, in_dims=1, out_dims=S,
obs_len=k+2, pred_len=k), seeded, run on CPU in the build container.

    python tools/make_golden_sgcn_net.py --ref <reference checkout> --out tests/golden

The reference's SGCN moves itself to the GPU inside its constructor and its forward; as in tools/make_golden_sgcn.py,
`Tensor.cuda` / `Module.cuda` are the identity for the duration of this script and `torch.zeros_like(..., device='cuda')`
stays on the CPU -- the arithmetic is the reference's own.  Before anything is recorded every PReLU slope is set to a
non-default random value (0.25 everywhere would hide a swapped slope).  The ET descriptors and anchors are G2's
(tests/golden/g2_fit_all_scenes.npz), per split.  The values that enter the two sigmoids of the interaction mask (the
*logits*) are captured with forward pre-hooks on the reference's own Sigmoid modules.  Stored:
  net.<state_dict key>          the predictor's state_dict (one set for all splits: they share k = 6, S = 20)
  <split>.scene_size, .ade, .fde, .min_abs_logit
                                per test scene / per pedestrian (best-of-S, the inference form model(obs)) / per scene the
                                smallest |logit| over both masks, every test scene of eth, hotel, univ, zara1, zara2
  pick<i>.{split,index,v,identity_s,identity_t,net_out,logit_s,logit_t}
                                the largest scene of each split, one scene of N <= 2, the first scene with some
                                |logit| < 1e-5: the network input the bridge built, its output and its fp32 logits
  gen.<state_dict key>, gen.pick<i>, gen.net_out<i>, gen.logit_s<i>, gen.logit_t<i>
                                a second weight set (number_asymmetric_conv_layer = 3, n_tcn = 2, out_dims = 12) on the
                                inputs of two picks
Only data is written; nothing of the reference is copied."""
import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
DELTA = 1e-5


def randomise(net, gen):
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.PReLU):
                m.weight.copy_(0.05 + 0.4 * torch.rand(m.weight.shape, generator=gen))


def capture_logits(net, store):
    im = net.sparse_weighted_adjacency_matrices.interaction_mask
    im.spatial_output.register_forward_pre_hook(lambda m, a: store.__setitem__("logit_s", a[0].detach().clone()))
    im.temporal_output.register_forward_pre_hook(lambda m, a: store.__setitem__("logit_t", a[0].detach().clone()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    from tests import _golden as G
    sys.path.insert(0, args.ref)
    os.chdir(args.ref)

    # no GPU in the build container: keep the reference's SGCN on the CPU
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    _zeros_like = torch.zeros_like

    def zeros_like_cpu(x, *a, **k):
        k.pop("device", None)
        return _zeros_like(x, *a, **k)
    torch.zeros_like = zeros_like_cpu

    from baseline.sgcn import TrajectoryPredictor, model_forward, model_forward_post_hook, model_forward_pre_hook
    from EigenTrajectory import EigenTrajectory
    from utils.metrics import compute_batch_ade, compute_batch_fde
    from utils.utils import DotDict, get_exp_config

    torch.set_num_threads(1)
    g2 = G.load("g2_fit_all_scenes.npz")
    out, picks = {}, []
    have_small = have_undecided = False
    net_state = None
    t0 = time.time()
    for scene in G.SCENES:
        hp = get_exp_config(f"./config/eigentrajectory-{{baseline}}-{scene}.json")
        assert hp.k == 6 and hp.num_samples == 20, (hp.k, hp.num_samples)
        torch.manual_seed(1234)
        predictor = TrajectoryPredictor(number_asymmetric_conv_layer=7, embedding_dims=64, number_gcn_layers=1, dropout=0,
                                        obs_len=hp.k + 2, pred_len=hp.k, n_tcn=5, in_dims=1, out_dims=hp.num_samples)
        randomise(predictor, torch.Generator().manual_seed(4321))
        predictor.eval()
        if net_state is None:
            net_state = {k: v.detach().clone() for k, v in predictor.state_dict().items()}
        captured = {}
        capture_logits(predictor, captured)

        def forward_and_capture(input_data, baseline_model):
            v, eyes = input_data
            captured["v"] = v.detach().clone()
            captured["identity_s"], captured["identity_t"] = eyes[0].detach().clone(), eyes[1].detach().clone()
            res = model_forward(input_data, baseline_model)
            captured["net_out"] = res.detach().clone()
            return res

        hook = DotDict(model_forward_pre_hook=model_forward_pre_hook, model_forward=forward_and_capture,
                       model_forward_post_hook=model_forward_post_hook)
        model = EigenTrajectory(predictor, hook, hp).eval()
        sd = model.state_dict()
        for key in list(sd):
            if key.startswith("ET_"):
                sd[key] = torch.from_numpy(g2[f"{scene}.{key}"])
        model.load_state_dict(sd)
        obs, pred, sse = G.dataset(scene, "test")
        ades, fdes, sizes, minabs, records = [], [], [], [], []
        for i, (s, e) in enumerate(sse):
            o, p = torch.from_numpy(obs[s:e]), torch.from_numpy(pred[s:e])
            with torch.no_grad():
                res = model(o)  # the test loop's call (utils/trainer.py:183)
            ades.append(np.asarray(compute_batch_ade(res["recon_traj"], p), np.float32))
            fdes.append(np.asarray(compute_batch_fde(res["recon_traj"], p), np.float32))
            sizes.append(e - s)
            minabs.append(min(float(captured["logit_s"].abs().min()), float(captured["logit_t"].abs().min())))
            records.append((e - s, i, {k: captured[k].numpy() for k in captured}))
        out[f"{scene}.static_dist"] = np.float32(hp.static_dist)
        out[f"{scene}.scene_size"] = np.asarray(sizes, np.int64)
        out[f"{scene}.ade"] = np.concatenate(ades)
        out[f"{scene}.fde"] = np.concatenate(fdes)
        out[f"{scene}.min_abs_logit"] = np.asarray(minabs, np.float32)
        largest = max(records, key=lambda r: r[0])
        chosen = [largest]
        small = [r for r in records if r[0] <= 2]
        if small and not have_small:
            chosen.append(small[0])
            have_small = True
        und = [r for r, m in zip(records, minabs) if m < DELTA]
        if und and not have_undecided:
            if all(und[0][1] != c[1] for c in chosen):
                chosen.append(und[0])
            have_undecided = True
        for size, idx, cap in chosen:
            tag = f"pick{len(picks)}"
            picks.append(tag)
            out[f"{tag}.split"] = np.asarray(scene)
            out[f"{tag}.index"] = np.int64(idx)
            for key in ("v", "identity_s", "identity_t", "net_out", "logit_s", "logit_t"):
                out[f"{tag}.{key}"] = cap[key].astype(np.float32)
        print(f"{scene}: {len(sse)} scenes, {sum(sizes)} pedestrians, largest {largest[0]}, undecided scenes "
              f"{sum(m < DELTA for m in minabs)}, ADE {out[f'{scene}.ade'].mean():.5f} FDE {out[f'{scene}.fde'].mean():.5f}"
              f"  ({time.time() - t0:.0f} s)", flush=True)
    for key, val in net_state.items():
        out[f"net.{key}"] = val.numpy()

    # the generic loop structure: another number of asymmetric convolutions and of tcns, another output width
    torch.manual_seed(99)
    gen_net = TrajectoryPredictor(number_asymmetric_conv_layer=3, embedding_dims=64, number_gcn_layers=1, dropout=0,
                                  obs_len=8, pred_len=6, n_tcn=2, in_dims=1, out_dims=12)
    randomise(gen_net, torch.Generator().manual_seed(77))
    gen_net.eval()
    captured = {}
    capture_logits(gen_net, captured)
    for key, val in gen_net.state_dict().items():
        out[f"gen.{key}"] = val.detach().numpy()
    by_size = sorted(picks, key=lambda t: out[f"{t}.v"].shape[2])
    for i, tag in enumerate([t for t in by_size if out[f"{t}.v"].shape[2] >= 3][:2]):
        with torch.no_grad():
            res = gen_net(torch.from_numpy(out[f"{tag}.v"]), [torch.from_numpy(out[f"{tag}.identity_s"]),
                                                              torch.from_numpy(out[f"{tag}.identity_t"])])
        out[f"gen.pick{i}"] = np.asarray(tag)
        out[f"gen.net_out{i}"] = res.numpy()
        out[f"gen.logit_s{i}"] = captured["logit_s"].numpy()
        out[f"gen.logit_t{i}"] = captured["logit_t"].numpy()
    path = os.path.join(args.out, "g20_sgcn_net.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "picks",
          [(str(out[f'{t}.split']), int(out[f'{t}.index']), out[f'{t}.v'].shape[2]) for t in picks])


if __name__ == "__main__":
    main()
