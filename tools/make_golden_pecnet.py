#!/usr/bin/env python3
"""G24: ET-PECNet / ET-LBEBM inference fixture -- the reference's wrapper + its pecnet / lbebm bridges + its PECNet / LBEBM
with the ET constructor arguments (utils/trainer.py:296-316 and 399-430), run on the CPU.

    python tools/make_golden_pecnet.py --ref /root/reference --out tests/golden

Weights are NOT stored (the ET-size set is ~8 MB): tests/_pecnet_np.py's make_weights fills the recorded (key, shape) list from
np.random.default_rng(seed), tensor by tensor, uniform in +-1/sqrt(fan_in), the last layers of non_local_theta / non_local_phi
times `factor`; this script loads exactly those tensors into the reference's modules.  `factor` is the smallest power of two
for which, in every recorded scene of 8 or more pedestrians, every row's first-round logits span more than 5 (with
near-uniform attention a wrong softmax would pass).  The ET descriptors and anchors are G2's
(tests/golden/g2_fit_all_scenes.npz), per split.  Four configurations: `pecnet`, `lbebm` (ET: k = 6, S = 20) and `pecnet_gen`,
`lbebm_gen` (hidden (24, 12) everywhere, fdim 5, non_local_dim 7, nonlocal_pools 2, k = 4, S = 3; their `past` is the first 4
coefficient rows of the same inputs).  Stored:
  <cfg>.keys / .shapes / .seed / .factor / .sums / .k / .S
                           the state_dict's keys in order, their shapes (-1 padded), the generator's arguments, the fp64
                           sum of every generated tensor
  <tag>.u                  a call's input [C_obs; obs_ori] (k + 2, n) fp32: past = u[:k].T, dest = initial_pos = u[k:].T
  <tag>.mask               its (n, n) bool mask where it is not all ones
  <cfg>.<tag>.out / .c_pred_refine
                           the reference's predict output (n, k S) and the post-hook's (k, n, S)
      tags: pick<i> (.split, .index, .coincident: the largest test scene of each split and the first small scene in which a
      row of u holds a value twice, through the reference's wrapper), single (n = 1, hand-built), block (three scenes of 3,
      1, 5 rows collated under a block-diagonal mask; block.sizes), zerorow (n = 6, a random mask whose row 2 is all zero)
  <kind>.<split>.ade / .fde, <split>.scene_size / .static_dist
                           per pedestrian best-of-S of the inference form model(obs, addl_info) on every test scene of eth,
                           hotel and zara1, for both predictors
  ref_fp32_err             the worst distance of a recorded fp32 output from the reference's own float64 run
The script asserts what the tests rely on: the fp64 restatement (tests/_pecnet_np.py) reproduces every recorded output
within 1e-5 of its largest entry; every recorded output is within 2.5e-6 of the reference's float64 run; the restatement
with uniform attention misses every recorded PECNet output of a scene of 8 or more by more than 1e-3.
tests/_pecnet_np.py is hand-written and kept next to the tests; this script imports it (as tools/make_golden_dmrgcn.py imports
tests/_dmrgcn_np.py) and does not generate it.  Only data is written; nothing of the reference is copied."""
import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

TOL = 1e-5
SEED = 24
NL = dict(non_local_theta_size=[256, 128, 64], non_local_phi_size=[256, 128, 64], non_local_g_size=[256, 128, 64],
          non_local_dim=128, nonlocal_pools=3)
GEN = [24, 12]


def build(kind, gen, PECNet, LBEBM, DotDict):
    """-> (the reference's module, k, S)"""
    if not gen:
        k, S = 6, 20
        if kind == "pecnet":  # baseline/pecnet/optimal.yaml
            net = PECNet([512, 256], [8, 16], [8, 50], [1024, 512, 1024], [1024, 512, 256], NL["non_local_theta_size"],
                         NL["non_local_phi_size"], NL["non_local_g_size"], 16, 16, 3, 128, 1.3, k // 2, k * S // 2 + 1, False)
        else:
            args = DotDict(dict(NL, sub_goal_indexes=[11], ny=1, memory_size=200000))
            net = LBEBM([512, 256], [256, 128], [256, 512], [1024, 512, 1024], [1024, 512, 256], 16, 16, 1.3, k // 2,
                        k * S // 2, args=args)
    else:
        k, S = 4, 3
        if kind == "pecnet":
            net = PECNet(GEN, GEN, GEN, GEN, GEN, GEN, GEN, GEN, 5, 3, 2, 7, 1.3, k // 2, k * S // 2 + 1, False)
        else:
            args = DotDict(non_local_theta_size=GEN, non_local_phi_size=GEN, non_local_g_size=GEN, non_local_dim=7,
                           nonlocal_pools=2, sub_goal_indexes=[11], ny=1, memory_size=10)
            net = LBEBM(GEN, GEN, GEN, GEN, GEN, 5, 3, 1.3, k // 2, k * S // 2, args=args)
    return net.eval(), k, S


def load(net, sd):
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)


def predict(kind, net, u, mask, k, dtype=torch.float32):
    """the bridge's call on u (K, n): past = the first k rows"""
    past = torch.from_numpy(np.ascontiguousarray(u[:k].T)).to(dtype)
    ori = torch.from_numpy(np.ascontiguousarray(u[-2:].T)).to(dtype)
    with torch.no_grad():
        if kind == "pecnet":
            m = torch.ones(u.shape[1], u.shape[1], dtype=torch.bool) if mask is None else torch.from_numpy(mask)
            return net.predict(past, ori, m, ori).numpy()
        return net.predict(past, ori).numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    from tests import _golden as G
    from tests import _pecnet_np as PN
    sys.path.insert(0, args.ref)
    os.chdir(args.ref)

    # no GPU in the build container: keep the reference's normalizer on the CPU
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self

    from baseline.lbebm import bridge as lb_bridge
    from baseline.lbebm.model import LBEBM
    from baseline.pecnet import bridge as pc_bridge
    from baseline.pecnet.model import PECNet
    from EigenTrajectory import EigenTrajectory
    from utils.metrics import compute_batch_ade, compute_batch_fde
    from utils.utils import DotDict, get_exp_config

    torch.set_num_threads(1)
    g2 = G.load("g2_fit_all_scenes.npz")
    out = {}
    t0 = time.time()
    CFGS = [("pecnet", False), ("lbebm", False), ("pecnet", True), ("lbebm", True)]
    name = lambda kind, gen: kind + ("_gen" if gen else "")
    nets, lists = {}, {}
    for kind, gen in CFGS:
        net, k, S = build(kind, gen, PECNet, LBEBM, DotDict)
        keys = list(net.state_dict().keys())
        shapes = [tuple(v.shape) for v in net.state_dict().values()]
        nets[name(kind, gen)], lists[name(kind, gen)] = (net, k, S), (keys, shapes)

    # ---- the inputs: real scenes through the reference's wrapper (the pecnet bridge; lbebm's hands over the same rows)
    inputs, masks, meta = {}, {}, {}
    bridges = {"pecnet": pc_bridge, "lbebm": lb_bridge}
    captured = {}

    def wrapper(kind, scene):
        hp = get_exp_config(f"./config/eigentrajectory-{{baseline}}-{scene}.json")
        assert hp.k == 6 and hp.num_samples == 20, (hp.k, hp.num_samples)
        br = bridges[kind]

        def pre_and_capture(obs_data, obs_ori, addl_info=None):
            captured["u"] = torch.cat([obs_data, obs_ori], dim=0).detach().clone().numpy()
            return br.model_forward_pre_hook(obs_data, obs_ori, addl_info)

        hook = DotDict(model_forward_pre_hook=pre_and_capture, model_forward=br.model_forward,
                       model_forward_post_hook=br.model_forward_post_hook)
        model = EigenTrajectory(nets[kind][0], hook, hp).eval()
        sd = model.state_dict()
        for key in list(sd):
            if key.startswith("ET_"):
                sd[key] = torch.from_numpy(g2[f"{scene}.{key}"])
        model.load_state_dict(sd)
        return model, hp

    def run_scene(model, hp, obs_rows):
        o = torch.from_numpy(obs_rows)
        info = {"scene_mask": torch.ones(len(o), len(o), dtype=torch.bool), "num_samples": hp.num_samples}
        with torch.no_grad():
            return model(o, addl_info=info)

    # weights with factor 1 first: the inputs do not depend on them
    picks, first_coincident = [], None
    for scene in G.SCENES:
        model, hp = wrapper("pecnet", scene)
        obs, pred, sse = G.dataset(scene, "test")
        out[f"{scene}.static_dist"] = np.float32(hp.static_dist)
        sizes = [int(e - s) for s, e in sse]
        chosen = [int(np.argmax(sizes))]
        if first_coincident is None:
            for i, (s, e) in enumerate(sse):
                if 2 <= e - s <= 30 and i != chosen[0]:
                    run_scene(model, hp, obs[s:e])
                    if any(len(np.unique(row)) < len(row) for row in captured["u"]):
                        first_coincident = (scene, i)
                        chosen.append(i)
                        break
        for i in chosen:
            s, e = sse[i]
            run_scene(model, hp, obs[s:e])
            tag = f"pick{len(picks)}"
            picks.append(tag)
            inputs[tag], masks[tag] = captured["u"].astype(np.float32), None
            out[f"{tag}.split"], out[f"{tag}.index"] = np.asarray(scene), np.int64(i)
            out[f"{tag}.coincident"] = np.bool_((scene, i) == first_coincident)
    assert first_coincident is not None
    rng = np.random.default_rng(2424)
    inputs["single"], masks["single"] = np.asarray([[0.5], [-1.25], [2.0], [0.0], [3.0], [-0.75], [0.0], [0.0]], np.float32), None
    sizes = [3, 1, 5]
    u = rng.normal(0, 1.5, (8, sum(sizes))).astype(np.float32)
    block = np.zeros((sum(sizes), sum(sizes)), np.bool_)
    lo = 0
    for n in sizes:
        u[6:, lo:lo + n] -= u[6:, lo:lo + n].mean(axis=1, keepdims=True)
        block[lo:lo + n, lo:lo + n] = True
        lo += n
    inputs["block"], masks["block"] = u, block
    out["block.sizes"] = np.asarray(sizes, np.int64)
    u = rng.normal(0, 1.5, (8, 6)).astype(np.float32)
    zr = rng.random((6, 6)) < 0.6
    zr[np.arange(6), np.arange(6)] = True
    zr[2] = False
    inputs["zerorow"], masks["zerorow"] = u, zr
    tags = picks + ["single", "block", "zerorow"]
    for tag in tags:
        out[f"{tag}.u"] = inputs[tag]
        if masks[tag] is not None:
            out[f"{tag}.mask"] = masks[tag]

    # ---- the weights: the smallest power-of-two factor that spreads every row's logits by more than 5
    factors = {}
    for cfg, (net, k, S) in nets.items():
        keys, shapes = lists[cfg]
        factor = 1.0
        while True:
            sd = PN.make_weights(keys, shapes, SEED, factor)
            if not cfg.startswith("pecnet"):
                break
            span = min(float(np.ptp(PN.first_logits(sd, inputs[t][:k].T, inputs[t][-2:].T, inputs[t][-2:].T), axis=1).min())
                       for t in picks if inputs[t].shape[1] >= 8)
            if span > 5:
                print(f"{cfg}: factor {factor}, the narrowest row of logits spans {span:.2f}")
                break
            factor *= 2
            assert factor <= 2 ** 20
        factors[cfg] = factor
        load(net, sd)
        out[f"{cfg}.keys"] = np.asarray(keys)
        out[f"{cfg}.shapes"] = np.asarray([list(s) + [-1] * (2 - len(s)) for s in shapes], np.int64)
        out[f"{cfg}.seed"], out[f"{cfg}.factor"] = np.int64(SEED), np.float64(factor)
        out[f"{cfg}.sums"] = np.asarray([sd[key].sum(dtype=np.float64) for key in keys])
        out[f"{cfg}.k"], out[f"{cfg}.S"] = np.int64(k), np.int64(S)
        PN.check_weights(out, cfg, PN.make_weights(keys, shapes, SEED, factor))

    # ---- the recorded calls
    ref_fp32_err = worst_np = 0.0
    for cfg, (net, k, S) in nets.items():
        kind = cfg.split("_")[0]
        sd = PN.make_weights(*lists[cfg], SEED, factors[cfg])
        pools = net.nonlocal_pools if kind == "pecnet" else 0
        for tag in tags:
            u, mask = inputs[tag], masks[tag]
            res = predict(kind, net, u, mask, k)
            res64 = predict(kind, net.double(), u, mask, k, torch.float64)
            net.float()
            load(net, sd)  # (.double().float() round-trips exactly; reload to be plain about it)
            scale = np.abs(res64).max()
            err = float(np.abs(res - res64).max() / scale)
            assert err <= 2.5e-6, (cfg, tag, err)
            ref_fp32_err = max(ref_fp32_err, err)
            ones = np.ones((u.shape[1], u.shape[1]))
            if kind == "pecnet":
                got = PN.pecnet_predict(sd, u[:k].T, u[-2:].T, ones if mask is None else mask, u[-2:].T, pools)
                if u.shape[1] >= 8:
                    flat = PN.pecnet_predict(sd, u[:k].T, u[-2:].T, ones if mask is None else mask, u[-2:].T, pools, uniform=True)
                    miss = float(np.abs(flat - res).max() / np.abs(res).max())
                    assert miss > 100 * TOL, (cfg, tag, miss)
            else:
                got = PN.lbebm_predict(sd, u[:k].T, u[-2:].T)
            e_np = float(np.abs(got - res).max() / np.abs(res).max())
            assert e_np <= TOL, (cfg, tag, e_np)
            worst_np = max(worst_np, e_np)
            out[f"{cfg}.{tag}.out"] = res.astype(np.float32)
            post = bridges[kind].model_forward_post_hook(torch.from_numpy(res), {"num_samples": S}).numpy()
            assert np.array_equal(post, PN.post_hook(res, S))
            out[f"{cfg}.{tag}.c_pred_refine"] = np.ascontiguousarray(post, np.float32)
    out["ref_fp32_err"] = np.float64(ref_fp32_err)
    print(f"fp32 outputs against the reference's float64 run: {ref_fp32_err:.2e}; fp64 restatement against the recorded "
          f"outputs: {worst_np:.2e}  ({time.time() - t0:.0f} s)", flush=True)

    # ---- whole splits end to end, the inference form
    for scene in ("eth", "hotel", "zara1"):
        obs, pred, sse = G.dataset(scene, "test")
        out[f"{scene}.scene_size"] = np.asarray([e - s for s, e in sse], np.int64)
        for kind in ("pecnet", "lbebm"):
            model, hp = wrapper(kind, scene)
            ades, fdes = [], []
            for s, e in sse:
                res = run_scene(model, hp, obs[s:e])
                p = torch.from_numpy(pred[s:e])
                ades.append(np.asarray(compute_batch_ade(res["recon_traj"], p), np.float32))
                fdes.append(np.asarray(compute_batch_fde(res["recon_traj"], p), np.float32))
            out[f"{kind}.{scene}.ade"], out[f"{kind}.{scene}.fde"] = np.concatenate(ades), np.concatenate(fdes)
            print(f"{kind} {scene}: {len(sse)} scenes, ADE {np.concatenate(ades).mean():.5f} FDE "
                  f"{np.concatenate(fdes).mean():.5f}  ({time.time() - t0:.0f} s)", flush=True)

    path = os.path.join(args.out, "g24_pecnet.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "picks",
          [(str(out[f"{t}.split"]), int(out[f"{t}.index"]), inputs[t].shape[1], bool(out[f"{t}.coincident"])) for t in picks])
    assert os.path.getsize(path) < 1000 * 1000


if __name__ == "__main__":
    main()
