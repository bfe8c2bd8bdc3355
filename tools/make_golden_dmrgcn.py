#!/usr/bin/env python3
"""G23: ET-DMRGCN inference fixture -- the reference's wrapper + its dmrgcn bridge + its social_dmrgcn with the ET
constructor arguments (utils/trainer.py:491-502: n_stgcn=1, n_tpcnn=4, input_feat=1, output_feat=S, kernel_size=3,
seq_len=k+2, pred_seq_len=k), seeded, run on CPU in the build container.

    python tools/make_golden_dmrgcn.py --ref /root/reference --out tests/golden

The reference's normalizer moves its identity matrices to the GPU (`torch.eye(...).cuda()`, baseline/dmrgcn/normalizer.py);
there is no GPU here, so for the duration of this script `Tensor.cuda` / `Module.cuda` are the identity -- the arithmetic is
the reference's own.  Before anything is recorded EVERY PReLU slope is set to its own random value (the default 0.25
everywhere would hide a swapped slope).  The ET descriptors and anchors are G2's (tests/golden/g2_fit_all_scenes.npz), per
split; they are not copied here.  Stored:
  net.<state_dict key>          the predictor's state_dict (one set for all splits: they share k = 6, S = 20)
  <split>.static_dist, .scene_size, .ade, .fde, .robust
                                per test scene / per pedestrian (best-of-S, the inference form model(obs), every test scene
                                of eth, hotel, univ, zara1, zara2, scene order).  robust (per scene): in the reference's own
                                v every pair distance of both relations is farther than 1e-5 max(1, s) from every non-zero
                                split value s, every exact zero off the diagonal is a tie at 0.0, between identical columns
                                or on an obs_ori row, and no pedestrian's moving / static decision is within 1e-5 of
                                static_dist: a scene on which an input computed a few ulp away decides every bin alike
  pick<i>.{split,index,v,a,net_out,c_pred_refine,coincident,boundary}
                                a handful of scenes: the network input (v, a) the bridge built, its raw output v and the
                                post-hook's C_pred_refine -- the largest scene of each split, the first small scene with
                                coincident columns, the first scene with a pair distance exactly on a split value
  grid.*, single.*              two hand-built scenes through the reference's bridge and network: n = 12 with every entry of v
                                a multiple of 0.25 in [-3, 3] (many distances exactly 0.25, 0.5, 0.75, 1, 2, 4, several 0),
                                and n = 1
  gen.<state_dict key>, gen.net_out<i>
                                a second weight set, n_stgcn = 2, n_tpcnn = 2, S = 12, on the inputs of picks 0 and 1
The script asserts what the GPU tests rely on: at least 95 % of the scenes of eth, zara1 and zara2 are robust, and the
fp64 restatement (tests/_dmrgcn_np.py) reproduces every recorded output within 1e-5 of its largest entry.
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

SPLIT = ((0.0, 0.25, 0.5, 0.75, 1.0), (0.0, 0.5, 1.0, 2.0, 4.0))
MARGIN = 1e-5


def randomise(net, gen):
    """every PReLU slope its own non-default value"""
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.PReLU):
                m.weight.copy_(0.05 + 0.4 * torch.rand(m.weight.shape, generator=gen))


def scene_facts(v, a, k):
    """v (K, n), a (2, K, n, n) as the reference built them -> (robust up to the moving/static decision, a pair exactly on a
    split value, columns that coincide in some time row)"""
    n = v.shape[1]
    off = ~np.eye(n, dtype=bool)
    robust, boundary = True, False
    same_col = (v[:, :, None] == v[:, None, :]).all(axis=0)
    for r in range(2):
        src = v if r == 1 else np.concatenate([np.zeros_like(v[:1]), v[1:] - v[:-1]])
        for s in SPLIT[r][1:]:
            gap = np.abs(a[r].astype(np.float64) - s)
            boundary |= bool((a[r] == np.float32(s)).any())
            robust &= bool((gap > MARGIN * max(1.0, s)).all())
        for t in range(v.shape[0]):
            zero = (a[r][t] == 0) & off
            tie0 = (src[t][:, None] == 0) & (src[t][None, :] == 0)
            ori_row = t >= k + (1 if r == 0 else 0)  # v_rel[k] mixes the last coefficient row into obs_ori's first
            if not ori_row and bool((zero & ~tie0 & ~same_col).any()):
                robust = False
    coincident = any(len(np.unique(row)) < len(row) for row in v)  # equal values in one time row
    return robust, boundary, coincident


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    from tests import _dmrgcn_np as DN
    from tests import _golden as G
    sys.path.insert(0, args.ref)
    os.chdir(args.ref)

    # no GPU in the build container: keep the reference's normalizer on the CPU
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self

    from baseline.dmrgcn import TrajectoryPredictor, model_forward, model_forward_post_hook, model_forward_pre_hook
    from EigenTrajectory import EigenTrajectory
    from utils.metrics import compute_batch_ade, compute_batch_fde
    from utils.utils import DotDict, get_exp_config

    torch.set_num_threads(1)
    g2 = G.load("g2_fit_all_scenes.npz")
    out = {}
    picks = []
    t0 = time.time()
    net_state = None
    first_boundary = first_coincident = None
    for scene in G.SCENES:
        hp = get_exp_config(f"./config/eigentrajectory-{{baseline}}-{scene}.json")
        assert hp.k == 6 and hp.num_samples == 20, (hp.k, hp.num_samples)
        torch.manual_seed(1234)
        predictor = TrajectoryPredictor(n_stgcn=1, n_tpcnn=4, input_feat=1, output_feat=hp.num_samples, kernel_size=3,
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
            captured["net_out"] = res[0].detach().clone()
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
        model.load_state_dict(sd)
        obs, pred, sse = G.dataset(scene, "test")
        ades, fdes, sizes, robust, records = [], [], [], [], []
        for i, (s, e) in enumerate(sse):
            o, p = torch.from_numpy(obs[s:e]), torch.from_numpy(pred[s:e])
            with torch.no_grad():
                res = model(o)  # the test loop's call (utils/trainer.py:183)
            ades.append(np.asarray(compute_batch_ade(res["recon_traj"], p), np.float32))
            fdes.append(np.asarray(compute_batch_fde(res["recon_traj"], p), np.float32))
            sizes.append(e - s)
            cap = {k: captured[k].numpy() for k in captured}
            rob, boundary, coincident = scene_facts(cap["v"][0, 0], cap["a"][0], hp.k)
            # the moving / static decision (EigenTrajectory/model.py: half the last two-frame displacement against static_dist)
            half = np.linalg.norm((obs[s:e, -1] - obs[s:e, -3]).astype(np.float64) / 2, axis=1)
            rob &= bool((np.abs(half - float(hp.static_dist)) > MARGIN).all())
            robust.append(rob)
            records.append((e - s, coincident, boundary, i, cap))
        out[f"{scene}.static_dist"] = np.float32(hp.static_dist)
        out[f"{scene}.scene_size"] = np.asarray(sizes, np.int64)
        out[f"{scene}.ade"] = np.concatenate(ades)
        out[f"{scene}.fde"] = np.concatenate(fdes)
        out[f"{scene}.robust"] = np.asarray(robust, np.bool_)
        largest = max(records, key=lambda r: r[0])
        chosen = [largest]
        if first_coincident is None:
            co = [r for r in records if r[1] and 2 <= r[0] <= 30 and r[3] != largest[3]]
            if co:
                first_coincident = co[0]
                chosen.append(co[0])
        if first_boundary is None:
            bo = [r for r in records if r[2]]
            if bo:
                first_boundary = bo[0]
                if all(bo[0][3] != c[3] for c in chosen):
                    chosen.append(bo[0])
        for size, coincident, boundary, idx, cap in chosen:
            tag = f"pick{len(picks)}"
            picks.append(tag)
            out[f"{tag}.split"] = np.asarray(scene)
            out[f"{tag}.index"] = np.int64(idx)
            out[f"{tag}.coincident"] = np.bool_(coincident)
            out[f"{tag}.boundary"] = np.bool_(boundary)
            for key in ("v", "a", "net_out", "c_pred_refine"):
                out[f"{tag}.{key}"] = cap[key].astype(np.float32)
        print(f"{scene}: {len(sse)} scenes, {sum(sizes)} pedestrians, largest {largest[0]}, robust "
              f"{np.mean(robust):.4f}, ADE {out[f'{scene}.ade'].mean():.5f} FDE {out[f'{scene}.fde'].mean():.5f}  "
              f"({time.time() - t0:.0f} s)", flush=True)
    assert first_coincident is not None and first_boundary is not None
    for key, val in net_state.items():
        out[f"net.{key}"] = val.numpy()

    # hand-built scenes through the reference's bridge and network (the last split's predictor: the same weights)
    rng = np.random.default_rng(23)
    grid = (rng.integers(-12, 13, size=(8, 12)) * 0.25).astype(np.float32)
    grid[:, 5] = grid[:, 2]  # identical columns
    for tag, v in (("grid", grid), ("single", np.asarray([[0.5], [-1.25], [2.0], [0.0], [3.0], [-0.75], [1.5], [-2.0]],
                                                         np.float32))):
        with torch.no_grad():
            inp = model_forward_pre_hook(torch.from_numpy(v[:6]), torch.from_numpy(v[6:]))
            res = model_forward(inp, predictor)
            out[f"{tag}.v"], out[f"{tag}.a"] = inp[0].numpy(), inp[1].numpy()
            out[f"{tag}.net_out"] = res[0].numpy()
            out[f"{tag}.c_pred_refine"] = model_forward_post_hook(res).numpy()
    hit = {(r, s): int((out["grid.a"][0, r] == np.float32(s)).sum()) for r in range(2) for s in SPLIT[r][1:]}
    assert all(c > 0 for c in hit.values()), hit
    off12 = ~np.eye(12, dtype=bool)
    assert int(((out["grid.a"][0, 1] == 0) & off12).sum()) > 16  # zeros beyond the identical pair of columns

    # the generic loop structure: two st_dmrgcn blocks (the second with C_in = S and an identity residual), two tpcnn blocks
    torch.manual_seed(99)
    gen_net = TrajectoryPredictor(n_stgcn=2, n_tpcnn=2, input_feat=1, output_feat=12, kernel_size=3, seq_len=8,
                                  pred_seq_len=6)
    randomise(gen_net, torch.Generator().manual_seed(77))
    gen_net.eval()
    for key, val in gen_net.state_dict().items():
        out[f"gen.{key}"] = val.detach().numpy()
    for i, tag in enumerate(picks[:2]):
        with torch.no_grad():
            res = gen_net(torch.from_numpy(out[f"{tag}.v"]), torch.from_numpy(out[f"{tag}.a"]))
        out[f"gen.net_out{i}"] = res[0].numpy()

    # what the GPU tests rely on
    for scene in ("eth", "zara1", "zara2"):
        assert out[f"{scene}.robust"].mean() >= 0.95, (scene, out[f"{scene}.robust"].mean())
    sd_np = {k[4:]: v for k, v in out.items() if k.startswith("net.")}
    gen_np = {k[4:]: v for k, v in out.items() if k.startswith("gen.") and not k.startswith("gen.net_out")}
    worst = 0.0
    for tag in picks + ["grid", "single"]:
        ref = out[f"{tag}.net_out"][0].astype(np.float64)
        got = DN.forward(sd_np, out[f"{tag}.v"][0, 0], out[f"{tag}.a"][0])
        worst = max(worst, float(np.abs(got - ref).max() / np.abs(ref).max()))
    for i, tag in enumerate(picks[:2]):
        ref = out[f"gen.net_out{i}"][0].astype(np.float64)
        got = DN.forward(gen_np, out[f"{tag}.v"][0, 0], out[f"{tag}.a"][0], n_stgcn=2, n_tpcnn=2)
        worst = max(worst, float(np.abs(got - ref).max() / np.abs(ref).max()))
    print(f"fp64 restatement against the recorded outputs: {worst:.2e} of the largest entry")
    assert worst <= 1e-5, worst
    path = os.path.join(args.out, "g23_dmrgcn.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "picks", [(str(out[f'{t}.split']), int(out[f'{t}.index']),
                                                            out[f'{t}.v'].shape[-1], bool(out[f'{t}.coincident']),
                                                            bool(out[f'{t}.boundary'])) for t in picks])
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()
