#!/usr/bin/env python3
"""G19: ET-STGCNN inference fixture -- the reference's wrapper + its stgcnn bridge + its social_stgcnn with the ET
constructor arguments (utils/trainer.py:274-275: n_stgcnn=1, n_txpcnn=5, input_feat=1, output_feat=S, kernel_size=3,
seq_len=k+2, pred_seq_len=k), seeded, run on CPU in the build container.

    python tools/make_golden_stgcnn.py --ref /root/reference --out tests/golden

Before anything is recorded every BatchNorm's running statistics and affine parameters and every PReLU slope are set to
non-default random values (the defaults -- mean 0, var 1, weight 1, bias 0 -- would hide a missing or mis-ordered BN).
The ET descriptors and anchors are G2's (tests/golden/g2_fit_all_scenes.npz), per split.  Stored:
  net.<state_dict key>          the predictor's state_dict (one set for all splits: they share k = 6, S = 20)
  <split>.ET.<key>              the descriptor / anchor parameters used
  <split>.scene_size, .ade, .fde per test scene / per pedestrian (best-of-S, the inference form model(obs), every test
                                scene of eth, hotel, univ, zara1, zara2, scene order)
  pick<i>.{split,index,v,a,net_out,c_pred_refine}
                                a handful of scenes: the network input (v, a) the bridge built, its raw output and the
                                post-hook's C_pred_refine -- the largest scene of each split and the first with coincident
                                coefficient values
  gen.<state_dict key>, gen.net_out<i>
                                a second weight set, n_stgcnn = 2, n_txpcnn = 3, S = 12, on the inputs of picks 0 and 1

    python tools/make_golden_stgcnn.py --ref <reference checkout> --out tests/golden --generic

writes g19b_stgcnn_generic.npz instead (g19_stgcnn.npz is left alone): the reference's social_stgcnn alone, for the loop
structures the ET configuration never takes.  For each (n_stgcnn, n_txpcnn, S, k) of GENERIC, tag c<i>:
  c<i>.cfg                      the four numbers
  c<i>.sd.<state_dict key>      seeded weights, randomised like the above
  c<i>.{s3,s11,ns}.{v,a,out,out64}
                                three calls: scenes of 3 and of 11 pedestrians (two of the 11 coincident) with the v and
                                a the reference's bridge builds, and one with a dense NON-symmetric normal a (the network
                                takes any a); out is the float32 network's output, out64 the same network's in float64 on
                                the same float32 v and a
MANIFEST.json gets the entry `g19b_stgcnn_generic`.
Only data is written; nothing of the reference is copied."""
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


def randomise(net, gen):
    """non-default BatchNorm statistics / affine parameters and PReLU slopes"""
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                c = m.num_features
                m.weight.copy_(0.6 + 0.8 * torch.rand(c, generator=gen))
                m.bias.copy_(0.2 * torch.randn(c, generator=gen))
                m.running_mean.copy_(0.3 * torch.randn(c, generator=gen))
                m.running_var.copy_(0.4 + 1.2 * torch.rand(c, generator=gen))
            elif isinstance(m, torch.nn.PReLU):
                m.weight.copy_(0.05 + 0.4 * torch.rand(m.weight.shape, generator=gen))


GENERIC = [(1, 1, 20, 6), (1, 2, 5, 1), (3, 8, 7, 3), (8, 3, 4, 2)]  # (n_stgcnn, n_txpcnn, S, k)


def generic(out_dir):
    """g19b: the reference's network on CPU for the configurations of GENERIC (cwd and sys.path are the reference's)"""
    from baseline.stgcnn import TrajectoryPredictor, model_forward_pre_hook
    torch.set_num_threads(1)
    out, man = {}, {"configs": [list(c) for c in GENERIC], "torch": torch.__version__, "numpy": np.__version__,
                    "largest": {}}
    for i, (n_st, n_tp, S, k) in enumerate(GENERIC):
        tag = f"c{i}"
        torch.manual_seed(500 + i)
        net = TrajectoryPredictor(n_stgcnn=n_st, n_txpcnn=n_tp, input_feat=1, output_feat=S, kernel_size=3, seq_len=k + 2,
                                  pred_seq_len=k)
        randomise(net, torch.Generator().manual_seed(600 + i))
        net.eval()
        out[f"{tag}.cfg"] = np.asarray([n_st, n_tp, S, k], np.int64)
        for key, val in net.state_dict().items():
            out[f"{tag}.sd.{key}"] = val.detach().numpy().copy()
        gen = torch.Generator().manual_seed(700 + i)
        calls = {}
        for n in (3, 11):
            obs_data = torch.randn((k, n), generator=gen)
            obs_ori = 3.0 * torch.randn((2, n), generator=gen)
            if n == 11:
                obs_data[:, 4], obs_ori[:, 4] = obs_data[:, 3], obs_ori[:, 3]  # one coincident pair
            calls[f"s{n}"] = model_forward_pre_hook(obs_data, obs_ori)
        calls["ns"] = (torch.randn((1, 1, k + 2, 7), generator=gen), torch.randn((k + 2, 7, 7), generator=gen))
        net64 = TrajectoryPredictor(n_stgcnn=n_st, n_txpcnn=n_tp, input_feat=1, output_feat=S, kernel_size=3,
                                    seq_len=k + 2, pred_seq_len=k).double().eval()
        net64.load_state_dict({key: val.double() for key, val in net.state_dict().items()})
        for name, (v, a) in calls.items():
            with torch.no_grad():
                res, res64 = net(v, a), net64(v.double(), a.double())
            assert res.dtype == torch.float32 and res64.dtype == torch.float64 and res.shape == (1, S, k, v.shape[-1])
            out[f"{tag}.{name}.v"], out[f"{tag}.{name}.a"] = v.numpy().copy(), a.numpy().copy()
            out[f"{tag}.{name}.out"], out[f"{tag}.{name}.out64"] = res.numpy(), res64.numpy()
            man["largest"][f"{tag}.{name}"] = repr(float(res64.abs().max()))
        assert not np.allclose(out[f"{tag}.ns.a"], np.swapaxes(out[f"{tag}.ns.a"], 1, 2))
    path = os.path.join(out_dir, "g19b_stgcnn_generic.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path))
    mpath = os.path.join(out_dir, "MANIFEST.json")
    with open(mpath) as f:
        m = json.load(f)
    m["g19b_stgcnn_generic"] = man
    with open(mpath, "w") as f:
        json.dump(m, f, indent=1, sort_keys=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    ap.add_argument("--generic", action="store_true", help="write g19b_stgcnn_generic.npz only (g19_stgcnn.npz is not touched)")
    args = ap.parse_args()
    args.out = os.path.abspath(args.out)
    from tests import _golden as G
    sys.path.insert(0, args.ref)
    os.chdir(args.ref)
    if args.generic:
        return generic(args.out)

    from baseline.stgcnn import TrajectoryPredictor, model_forward, model_forward_post_hook, model_forward_pre_hook
    from EigenTrajectory import EigenTrajectory
    from utils.metrics import compute_batch_ade, compute_batch_fde
    from utils.utils import DotDict, get_exp_config

    torch.set_num_threads(1)
    g2 = G.load("g2_fit_all_scenes.npz")
    out = {}
    picks = []
    t0 = time.time()
    net_state = None
    for scene in G.SCENES:
        hp = get_exp_config(f"./config/eigentrajectory-{{baseline}}-{scene}.json")
        assert hp.k == 6 and hp.num_samples == 20, (hp.k, hp.num_samples)
        torch.manual_seed(1234)
        predictor = TrajectoryPredictor(n_stgcnn=1, n_txpcnn=5, input_feat=1, output_feat=hp.num_samples, kernel_size=3,
                                        seq_len=hp.k + 2, pred_seq_len=hp.k)
        randomise(predictor, torch.Generator().manual_seed(4321))
        predictor.eval()
        if net_state is None:
            net_state = {k: v.detach().clone() for k, v in predictor.state_dict().items()}
        captured = {}

        def forward_and_capture(input_data, baseline_model):
            v, a = input_data
            captured["v"], captured["a"] = v.detach().clone(), a.detach().clone()
            res = model_forward(input_data, baseline_model)
            captured["net_out"] = res.detach().clone()
            return res

        def post_and_capture(output_data, addl_info=None):
            res = model_forward_post_hook(output_data, addl_info)
            captured["c_pred_refine"] = res.detach().clone()
            return res

        hook = DotDict(model_forward_pre_hook=model_forward_pre_hook, model_forward=forward_and_capture,
                       model_forward_post_hook=post_and_capture)
        model = EigenTrajectory(predictor, hook, hp).eval()
        sd = model.state_dict()
        for key in list(sd):
            if key.startswith("ET_"):
                sd[key] = torch.from_numpy(g2[f"{scene}.{key}"])
                out[f"{scene}.ET.{key}"] = g2[f"{scene}.{key}"]
        model.load_state_dict(sd)
        obs, pred, sse = G.dataset(scene, "test")
        ades, fdes, sizes, records = [], [], [], []
        for i, (s, e) in enumerate(sse):
            o, p = torch.from_numpy(obs[s:e]), torch.from_numpy(pred[s:e])
            with torch.no_grad():
                res = model(o)  # the test loop's call (utils/trainer.py:183)
            ades.append(np.asarray(compute_batch_ade(res["recon_traj"], p), np.float32))
            fdes.append(np.asarray(compute_batch_fde(res["recon_traj"], p), np.float32))
            sizes.append(e - s)
            v = captured["v"][0, 0].numpy()
            coincident = any(len(np.unique(row)) < len(row) for row in v)
            records.append((e - s, coincident, i, {k: captured[k].numpy() for k in captured}))
        out[f"{scene}.static_dist"] = np.float32(hp.static_dist)
        out[f"{scene}.scene_size"] = np.asarray(sizes, np.int64)
        out[f"{scene}.ade"] = np.concatenate(ades)
        out[f"{scene}.fde"] = np.concatenate(fdes)
        largest = max(records, key=lambda r: r[0])
        chosen = [largest]
        co = [r for r in records if r[1] and 2 <= r[0] <= 30]
        if co and co[0][2] != largest[2]:
            chosen.append(co[0])
        for size, coincident, idx, cap in chosen:
            tag = f"pick{len(picks)}"
            picks.append(tag)
            out[f"{tag}.split"] = np.asarray(scene)
            out[f"{tag}.index"] = np.int64(idx)
            out[f"{tag}.coincident"] = np.bool_(coincident)
            for key in ("v", "a", "net_out", "c_pred_refine"):
                out[f"{tag}.{key}"] = cap[key].astype(np.float32)
        print(f"{scene}: {len(sse)} scenes, {sum(sizes)} pedestrians, largest {largest[0]}, ADE "
              f"{out[f'{scene}.ade'].mean():.5f} FDE {out[f'{scene}.fde'].mean():.5f}  ({time.time() - t0:.0f} s)",
              flush=True)
    for key, val in net_state.items():
        out[f"net.{key}"] = val.numpy()

    # the generic loop structure: two st_gcn blocks (the second with an identity residual), n_txpcnn = 3
    torch.manual_seed(99)
    gen_net = TrajectoryPredictor(n_stgcnn=2, n_txpcnn=3, input_feat=1, output_feat=12, kernel_size=3, seq_len=8,
                                  pred_seq_len=6)
    randomise(gen_net, torch.Generator().manual_seed(77))
    gen_net.eval()
    for key, val in gen_net.state_dict().items():
        out[f"gen.{key}"] = val.detach().numpy()
    for i, tag in enumerate(picks[:2]):
        with torch.no_grad():
            res = gen_net(torch.from_numpy(out[f"{tag}.v"]), torch.from_numpy(out[f"{tag}.a"]))
        out[f"gen.net_out{i}"] = res.numpy()
    path = os.path.join(args.out, "g19_stgcnn.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "picks", [(str(out[f'{t}.split']), int(out[f'{t}.index']),
                                                            out[f'{t}.v'].shape[-1], bool(out[f'{t}.coincident']))
                                                           for t in picks])


if __name__ == "__main__":
    main()
