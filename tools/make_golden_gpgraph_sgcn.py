#!/usr/bin/env python3
"""G21: ET-GPGraph-SGCN inference fixture -- the reference's wrapper + its gpgraphsgcn bridge + get_GPGraph_SGCN_model with
the ET constructor arguments (utils/trainer.py:505-516: obs_len=k+2, pred_len=k, in_dims=1, out_dims=S), seeded, run on CPU.

    python tools/make_golden_gpgraph_sgcn.py --ref <reference checkout> --out tests/golden

As in tools/make_golden_sgcn_net.py, `Tensor.cuda` / `Module.cuda` are the identity for the duration of this script and
`torch.zeros_like(..., device='cuda')` stays on the CPU -- the arithmetic is the reference's own -- and every PReLU slope,
the mix one included, is set to a non-default random value before anything is recorded.  The ET descriptors and anchors are
G2's (tests/golden/g2_fit_all_scenes.npz), per split.  The weights' seed is 1235: with 1234, the seed of G20, the reference's
own run leaves 1.4e-4 of the ragged synthetic scenes' sigmoid entries within 1e-5 of zero, above the 1e-4 a set may have
(tests/_sgcn_np.py CAP_SPLIT) -- a condition on the inputs, checked on the CPU; 1235 is the next seed, and meets it.

The threshold.  With fresh weights `group_gen.th` = 1 lies below nearly every pair distance of the synthetic scenes, so
nothing would group.  th is chosen from the pair distances of the synthetic scenes of tests/_sgcn_np.py (RAGGED, SPLIT_SIZES;
20 270 pairs): the midpoint of the widest gap between adjacent sorted distances inside their 5 % .. 12 % quantile window, so
none of them has a pair near th.  The hand-built scenes are scaled from th; the recorded real scenes take th as it is (their
margins are recorded, and the picks are checked to have no pair within 1e-5 th).

Stored (data only; nothing of the reference is copied):
  net.<state_dict key>          the predictor's state_dict (th as chosen), one set for all splits (k = 6, S = 20)
  th_margin                     min |d - th| / th over the synthetic scenes' pairs
  <split>.static_dist, .scene_size, .ade, .fde, .margin, .min_abs_logit, .n_groups   (eth, hotel, zara1)
                                per test scene / per pedestrian (best-of-S) / per scene min |d - th| / th (inf without a
                                pair), the smallest |logit| over the three passes, the number of groups
  pick<i>.{split,index,v_abs,v_rel,dist,indices,out,out0,out1,out2}
                                the largest scene of each of the five splits, one scene of N <= 2, the four hand-built
                                scenes (split "hand"): what the bridge built, the reference's fp32 distance matrix, its
                                group indices, its output (1,S,k,N) and the three passes' outputs (k,n_m,S)
  pick<i>.logit_s<m>, .logit_t<m>   the three passes' fp32 logits -- for scenes of at most 32 pedestrians; for larger ones
                                (a committed file stays below 1 MiB) pick<i>.near_s<m> / near_t<m>, the flat positions and
                                values of the entries with |logit| < 1e-3, and pick<i>.min_abs_logit
  gen.<state_dict key>, gen.pick<i>, gen.out<i>, gen.indices<i>, gen.dist<i>, gen.logit_s<i>_<m>, gen.logit_t<i>_<m>
                                a second weight set (number_asymmetric_conv_layer = 3, n_tcn = 2, out_dims = 12) on the
                                inputs of two picks"""
import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
FULL_LOGITS_MAX_N = 32
NEAR = 1e-3
HAND = {"pair": ([0.0, 0.5], [0, 0]), "chain": ([0.0, 0.75, 1.5], [0, 0, 1]), "triangle": ([0.0, 0.4, 0.8], [0, 0, 0]),
        "four": ([0.0, 2.4, 0.8, 1.6], [0, 1, 0, 1])}  # positions along one direction in units of th -> expected labels


def randomise(net, gen):
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.PReLU):
                m.weight.copy_(0.05 + 0.4 * torch.rand(m.weight.shape, generator=gen))


class Capture:
    """the reference's own intermediate values of one forward: the three passes' logits and outputs, the distance matrix"""

    def __init__(self, net):
        self.net = net
        self.clear()
        im = net.baseline_model.sparse_weighted_adjacency_matrices.interaction_mask
        im.spatial_output.register_forward_pre_hook(lambda m, a: self.ls.append(a[0].detach().clone()))
        im.temporal_output.register_forward_pre_hook(lambda m, a: self.lt.append(a[0].detach().clone()))
        net.baseline_model.register_forward_hook(lambda m, a, out: self.outs.append(out.detach().clone()))
        gg = net.group_gen
        find = gg.find_group_indices

        def find_and_record(v, dist_mat):
            self.dist = dist_mat.detach().clone()
            return find(v, dist_mat)
        gg.find_group_indices = find_and_record

    def clear(self):
        self.ls, self.lt, self.outs, self.dist = [], [], [], None

    def run(self, v_abs, v_rel):
        self.clear()
        with torch.no_grad():
            out, idx = self.net(v_abs, v_rel)
        assert len(self.ls) == len(self.lt) == len(self.outs) == 3
        rec = {"v_abs": v_abs.numpy(), "v_rel": v_rel.numpy(), "dist": self.dist.numpy(), "indices": idx.numpy().astype(np.int64),
               "out": out.numpy()}
        for m in range(3):
            rec[f"logit_s{m}"], rec[f"logit_t{m}"], rec[f"out{m}"] = self.ls[m].numpy(), self.lt[m].numpy(), self.outs[m].numpy()
        rec["min_abs_logit"] = min(float(x.abs().min()) for x in self.ls + self.lt)
        return rec


def pair_distances(net, v_abs):
    """the reference's dist_mat of one scene (GroupGenerator.forward, d_type 'learned_l2norm'), lower triangle"""
    with torch.no_grad():
        n = v_abs.size(-1)
        temp = net.group_gen.group_cnn(v_abs).unsqueeze(dim=-1).repeat_interleave(repeats=n, dim=-1)
        d = (temp - temp.transpose(-2, -1)).norm(p=2, dim=1).squeeze(dim=0).mean(dim=0)
    return d.numpy()[np.tril(np.ones((n, n), bool), -1)]


def store_pick(out, tag, split, index, rec, th):
    from tests import _gpgraph_np as GN
    assert GN.pair_margin(rec["dist"].astype(np.float64), th) > GN.BAND_D, (tag, split, index)  # no undecided pair in a pick
    out[f"{tag}.split"], out[f"{tag}.index"] = np.asarray(split), np.int64(index)
    n = rec["v_abs"].shape[-1]
    for key in ("v_abs", "v_rel", "dist", "indices", "out", "out0", "out1", "out2"):
        out[f"{tag}.{key}"] = rec[key]
    out[f"{tag}.min_abs_logit"] = np.float32(rec["min_abs_logit"])
    for m in range(3):
        for kind in ("s", "t"):
            l = rec[f"logit_{kind}{m}"]
            if n <= FULL_LOGITS_MAX_N:
                out[f"{tag}.logit_{kind}{m}"] = l
            else:
                at = np.nonzero(np.abs(l.ravel()) < NEAR)[0]
                out[f"{tag}.near_{kind}{m}"] = np.stack([at.astype(np.float64), l.ravel()[at].astype(np.float64)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    ap.add_argument("--seed", type=int, default=1235, help="of the weights")
    args = ap.parse_args()
    args.out = os.path.abspath(args.out)
    from tests import _golden as G
    from tests import _gpgraph_np as GN
    from tests import _sgcn_np as SN
    sys.path.insert(0, args.ref)
    os.chdir(args.ref)

    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    _zeros_like = torch.zeros_like

    def zeros_like_cpu(x, *a, **k):
        k.pop("device", None)
        return _zeros_like(x, *a, **k)
    torch.zeros_like = zeros_like_cpu

    from baseline.gpgraphsgcn import TrajectoryPredictor, model_forward, model_forward_post_hook, model_forward_pre_hook
    from baseline.gpgraphsgcn.model_baseline import TrajectoryModel
    from baseline.gpgraphsgcn.model_groupwrapper import GPGraph
    from EigenTrajectory import EigenTrajectory
    from utils.metrics import compute_batch_ade, compute_batch_fde
    from utils.utils import DotDict, get_exp_config

    torch.set_num_threads(1)
    g2 = G.load("g2_fit_all_scenes.npz")
    t0 = time.time()
    torch.manual_seed(args.seed)
    predictor = TrajectoryPredictor(obs_len=8, pred_len=6, in_dims=1, out_dims=20)
    randomise(predictor, torch.Generator().manual_seed(4321))
    predictor.eval()
    cap = Capture(predictor)

    # ---- the network inputs of every scene (the wrapper's own projection and pre-hook; the predictor is not run yet)
    inputs = {}
    for scene in G.SCENES:
        hp = get_exp_config(f"./config/eigentrajectory-{{baseline}}-{scene}.json")
        assert hp.k == 6 and hp.num_samples == 20, (hp.k, hp.num_samples)
        seen = []

        def record_only(input_data, baseline_model):
            seen.append((input_data[0].detach().clone(), input_data[1].detach().clone()))
            return torch.zeros((1, 20, 6, input_data[0].size(-1))), None

        hook = DotDict(model_forward_pre_hook=model_forward_pre_hook, model_forward=record_only,
                       model_forward_post_hook=model_forward_post_hook)
        model = EigenTrajectory(predictor, hook, hp).eval()
        sd = model.state_dict()
        for key in list(sd):
            if key.startswith("ET_"):
                sd[key] = torch.from_numpy(g2[f"{scene}.{key}"])
        model.load_state_dict(sd)
        obs, pred, sse = G.dataset(scene, "test")
        sizes = sse[:, 1] - sse[:, 0]
        which = range(len(sse)) if scene in ("eth", "hotel", "zara1") else [int(np.argmax(sizes))]
        for i in which:
            s, e = sse[i]
            with torch.no_grad():
                model(torch.from_numpy(obs[s:e]))
        inputs[scene] = dict(model=model, hp=hp, which=list(which), seen=seen, obs=obs, pred=pred, sse=sse)
    synthetic = [GN.bridge_input(SN.synthetic_v(n)) for n in SN.RAGGED]
    C_obs, nrm = SN.synthetic_split(SN.SPLIT_SIZES, SN.SPLIT_SEED)
    lo = 0
    for n in SN.SPLIT_SIZES:
        synthetic.append(GN.bridge_input(SN.scene_input(C_obs, nrm, lo, lo + n)))
        lo += n

    # ---- the threshold
    pairs = [pair_distances(predictor, torch.from_numpy(va)[None, None]) for va, _ in synthetic]
    pairs = np.sort(np.concatenate(pairs).astype(np.float64))
    q5, q12 = np.quantile(pairs, [0.05, 0.12])
    win = pairs[(pairs >= q5) & (pairs <= q12)]
    at = int(np.argmax(np.diff(win)))
    th = float(np.float32(0.5 * (win[at] + win[at + 1])))
    margin = float(np.abs(pairs - th).min() / th)
    print(f"{pairs.size} pairs, smallest {pairs[0]:.4f}, median {np.median(pairs):.4f}; window [{q5:.4f}, {q12:.4f}] -> th = {th:.6f}, "
          f"relative margin {margin:.3e}", flush=True)
    assert margin > 10 * GN.BAND_D, margin
    with torch.no_grad():
        predictor.group_gen.th.fill_(th)
    out = {"th_margin": np.float64(margin)}
    net_state = {k: v.detach().clone() for k, v in predictor.state_dict().items()}
    for key, val in net_state.items():
        out[f"net.{key}"] = val.numpy()

    # ---- the recorded runs
    picks, have_small = [], False
    for scene in G.SCENES:
        d = inputs[scene]
        captured = {}

        def forward_and_capture(input_data, baseline_model):
            captured["rec"] = cap.run(*input_data)
            return torch.from_numpy(captured["rec"]["out"]), torch.from_numpy(captured["rec"]["indices"])

        d["model"].hook_func = DotDict(model_forward_pre_hook=model_forward_pre_hook, model_forward=forward_and_capture,
                                       model_forward_post_hook=model_forward_post_hook)
        ades, fdes, margins, minabs, groups, records = [], [], [], [], [], []
        for i in d["which"]:
            s, e = d["sse"][i]
            o, p = torch.from_numpy(d["obs"][s:e]), torch.from_numpy(d["pred"][s:e])
            with torch.no_grad():
                res = d["model"](o)
            rec = captured["rec"]
            ades.append(np.asarray(compute_batch_ade(res["recon_traj"], p), np.float32))
            fdes.append(np.asarray(compute_batch_fde(res["recon_traj"], p), np.float32))
            margins.append(GN.pair_margin(rec["dist"].astype(np.float64), th))
            minabs.append(rec["min_abs_logit"])
            groups.append(int(rec["indices"].max()) + 1)
            records.append((e - s, i, rec))
        if scene in ("eth", "hotel", "zara1"):
            out[f"{scene}.static_dist"] = np.float32(d["hp"].static_dist)
            out[f"{scene}.scene_size"] = np.asarray([r[0] for r in records], np.int64)
            out[f"{scene}.ade"], out[f"{scene}.fde"] = np.concatenate(ades), np.concatenate(fdes)
            out[f"{scene}.margin"] = np.asarray(margins, np.float64)
            out[f"{scene}.min_abs_logit"] = np.asarray(minabs, np.float32)
            out[f"{scene}.n_groups"] = np.asarray(groups, np.int64)
        chosen = [max(records, key=lambda r: r[0])]
        small = [r for r in records if r[0] <= 2]
        if small and not have_small:
            chosen.append(small[0])
            have_small = True
        for size, idx, rec in chosen:
            store_pick(out, f"pick{len(picks)}", scene, idx, rec, th)
            picks.append(f"pick{len(picks)}")
        print(f"{scene}: {len(records)} scenes, largest {chosen[0][0]} ({int(chosen[0][2]['indices'].max()) + 1} groups), "
              f"grouped scenes {sum(g < r[0] for g, r in zip(groups, records))}, smallest margin {min(margins):.3e}, undecided-logit "
              f"scenes {sum(m < SN.DELTA for m in minabs)}  ({time.time() - t0:.0f} s)", flush=True)
    assert have_small

    # ---- the hand-built scenes: d(i, j) depends on x_i - x_j only and is 1-homogeneous in it
    rng = np.random.default_rng(21)
    x0 = SN.synthetic_v(1)[:, 0]
    delta = rng.normal(0, 1, x0.shape).astype(np.float32)
    unit = pair_distances(predictor, torch.from_numpy(np.stack([x0, x0 + delta], axis=1))[None, None])[0]
    for name, (pos, expect) in HAND.items():
        v = np.stack([x0 + np.float32(a * th / unit) * delta for a in pos], axis=1).astype(np.float32)
        va, vr = GN.bridge_input(v)
        rec = cap.run(torch.from_numpy(va)[None, None], torch.from_numpy(vr)[None])
        assert rec["indices"].tolist() == expect, (name, rec["indices"], expect, rec["dist"] / th)
        assert GN.pair_margin(rec["dist"].astype(np.float64), th) > 0.05
        store_pick(out, f"pick{len(picks)}", "hand", len(picks), rec, th)
        out[f"pick{len(picks)}.name"] = np.asarray(name)
        picks.append(f"pick{len(picks)}")
        print(f"hand-built {name}: d / th =\n{np.round(rec['dist'] / th, 3)}\nindices {rec['indices'].tolist()}", flush=True)

    # ---- the synthetic scenes: recorded group counts only (the GPU tests compare with the restatement)
    syn_groups = []
    for va, vr in synthetic:
        rec = cap.run(torch.from_numpy(va)[None, None], torch.from_numpy(vr)[None])
        syn_groups.append(int(rec["indices"].max()) + 1)
    out["synthetic.n_groups"] = np.asarray(syn_groups, np.int64)
    print("synthetic group counts", list(zip(list(SN.RAGGED) + list(SN.SPLIT_SIZES), syn_groups)), flush=True)

    # ---- the generic loop structure: another number of asymmetric convolutions and of tcns, another output width
    torch.manual_seed(99)
    base = TrajectoryModel(number_asymmetric_conv_layer=3, embedding_dims=64, number_gcn_layers=1, dropout=0, obs_len=8,
                           pred_len=6, n_tcn=2, in_dims=1, out_dims=12)
    gen_net = GPGraph(baseline_model=base, in_channels=1, out_channels=12, obs_seq_len=8, pred_seq_len=6,
                      d_type="learned_l2norm", d_th="learned", mix_type="mlp", group_type=(True, True, True), weight_share=True)
    randomise(gen_net, torch.Generator().manual_seed(77))
    with torch.no_grad():
        gen_net.group_gen.group_cnn[0].load_state_dict(predictor.group_gen.group_cnn[0].state_dict())  # (th's distances)
        gen_net.group_gen.th.fill_(th)
    gen_net.eval()
    gcap = Capture(gen_net)
    for key, val in gen_net.state_dict().items():
        out[f"gen.{key}"] = val.detach().numpy()
    grouped = [t for t in picks if 3 <= out[f"{t}.v_abs"].shape[-1] <= 8  # (small ones: the file stays below 1 MiB)
               and int(out[f"{t}.indices"].max()) + 1 < out[f"{t}.v_abs"].shape[-1]]
    for i, tag in enumerate(sorted(grouped, key=lambda t: -out[f"{t}.v_abs"].shape[-1])[:2]):
        rec = gcap.run(torch.from_numpy(out[f"{tag}.v_abs"]), torch.from_numpy(out[f"{tag}.v_rel"]))
        out[f"gen.pick{i}"] = np.asarray(tag)
        out[f"gen.out{i}"], out[f"gen.indices{i}"], out[f"gen.dist{i}"] = rec["out"], rec["indices"], rec["dist"]
        for m in range(3):
            out[f"gen.logit_s{i}_{m}"], out[f"gen.logit_t{i}_{m}"] = rec[f"logit_s{m}"], rec[f"logit_t{m}"]
    path = os.path.join(args.out, "g21_gpgraph_sgcn_net.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "picks",
          [(str(out[f'{t}.split']), int(out[f'{t}.index']), out[f'{t}.v_abs'].shape[-1], int(out[f'{t}.indices'].max()) + 1)
           for t in picks])
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
