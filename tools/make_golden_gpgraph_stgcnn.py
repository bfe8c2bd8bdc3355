#!/usr/bin/env python3
"""G22: ET-GPGraph-STGCNN inference fixture -- the reference's wrapper + its gpgraphstgcnn bridge + the classes behind
get_GPGraph_STGCNN_model with the ET constructor arguments (utils/trainer.py:505-530: obs_len=k+2, pred_len=k, in_dims=1,
out_dims=S), seeded, run on CPU.

    python tools/make_golden_gpgraph_stgcnn.py --ref <reference checkout> --out tests/golden
    python tools/make_golden_gpgraph_stgcnn.py --family --ref <reference checkout>     # G34 only, see family(); G22 is left alone

As in tools/make_golden_gpgraph_sgcn.py, `Tensor.cuda` / `Module.cuda` are the identity for the duration of this script, the
reference's classes are constructed directly, and the arithmetic is the reference's own.  Every BatchNorm's running
statistics and affine parameters and every PReLU slope, the mix one included, are set to non-default random values before
anything is recorded (tools/make_golden_stgcnn.py's randomise).  The ET descriptors and anchors are G2's, per split.

The threshold is chosen as for G21: from the pair distances of the synthetic scenes of tests/_sgcn_np.py (RAGGED,
SPLIT_SIZES), the midpoint of the widest gap between adjacent sorted distances inside their 5 % .. 12 % quantile window.

Every recorded scene is run twice, in fp32 and -- the same modules converted with .double() -- in fp64: `cond` is the
largest difference of the two outputs relative to the fp64 output's largest entry, the reference's OWN error on that scene
(1 / |u_i - u_j| is as ill conditioned as the closest pair of a time row).  `ties_robust` says that every exact off-diagonal
tie in the three graph inputs is at value 0.0 -- such ties survive v' = (v - s) + s; a non-zero one need not -- or between
two pedestrians whose whole input columns are identical (tests/_gpgraph_stgcnn_np.ties_robust).

Stored (data only; nothing of the reference is copied):
  net.<state_dict key>          the predictor's state_dict (th as chosen), one set for all splits (k = 6, S = 20)
  th_margin                     min |d - th| / th over the synthetic scenes' pairs
  eth.static_dist, .scene_size, .margin, .cond, .ties_robust, .n_groups (per test scene), .ade, .fde (per pedestrian)
  pick<i>.{split,index,v,dist,indices,v_intra,v_group,out,out0,out1,out2,cond,ties_robust}
                                the largest scene of each of the five splits, one scene of N <= 2, the four hand-built
                                scenes and `twins` (two identical pedestrians in one group: a whole-column tie) (split
                                "hand", with .name): v (T,N) as the bridge built it, the reference's fp32 distance matrix,
                                its group indices, the inputs of passes 2 and 1 as the base received them, its output
                                (1,S,k,N) and the three passes' outputs (1,S,k,n_m)
  gen.<state_dict key>, gen.pick<i>, gen.out<i>, gen.indices<i>, gen.v_intra<i>, gen.v_group<i>, gen.cond<i>
                                a second weight set (n_stgcnn = 2, n_txpcnn = 3, out_dims = 12) on two small grouped picks
Asserted here, on the CPU: no pick has a pair within 1e-5 th; the hand-built and small picks have cond <= 1e-6 and are
ties_robust; at least 90 % of eth's scenes are decided, ties_robust and have cond <= 1e-6."""
import argparse
import copy
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
HAND = {"pair": ([0.0, 0.5], [0, 0]), "chain": ([0.0, 0.75, 1.5], [0, 0, 1]), "triangle": ([0.0, 0.4, 0.8], [0, 0, 0]),
        "four": ([0.0, 2.4, 0.8, 1.6], [0, 1, 0, 1]),   # positions along one direction in units of th -> expected labels
        "twins": ([0.0, 0.0, 2.4], [0, 0, 1])}


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


class Capture:
    """the reference's own intermediate values of one forward: the three passes' inputs and outputs, the distance matrix"""

    def __init__(self, net):
        self.net = net
        self.clear()
        net.baseline_model.register_forward_pre_hook(lambda m, a: self.ins.append(a[0].detach().clone()))
        net.baseline_model.register_forward_hook(lambda m, a, out: self.outs.append(out[0].detach().clone()))
        gg = net.group_gen
        find = gg.find_group_indices

        def find_and_record(v, dist_mat):
            self.dist = dist_mat.detach().clone()
            return find(v, dist_mat)
        gg.find_group_indices = find_and_record

    def clear(self):
        self.ins, self.outs, self.dist = [], [], None

    def run(self, v):
        """v (T, N) float tensor -> the record of one forward in v's dtype"""
        self.clear()
        x = v[None, None]
        with torch.no_grad():
            out, idx = self.net(x, x)
        assert len(self.ins) == len(self.outs) == 3
        rec = {"v": v.numpy(), "dist": self.dist.numpy(), "indices": idx.numpy().astype(np.int64), "out": out.numpy(),
               "v_group": self.ins[1][0, 0].numpy(), "v_intra": self.ins[2][0, 0].numpy()}
        for m in range(3):
            rec[f"out{m}"] = self.outs[m].numpy()
        return rec


class Both:
    """a network and its .double() copy: every scene is run in fp32 and in fp64"""

    def __init__(self, net):
        self.cap = Capture(net)
        self.cap64 = Capture(copy.deepcopy(net).double())

    def run(self, v):
        from tests import _gpgraph_stgcnn_np as GS
        rec = self.cap.run(torch.from_numpy(np.asarray(v, np.float32)))
        torch.set_default_dtype(torch.float64)   # (the wrapper allocates its pooling buffers in the default dtype)
        try:
            r64 = self.cap64.run(torch.from_numpy(np.asarray(v, np.float64)))
        finally:
            torch.set_default_dtype(torch.float32)
        same = np.array_equal(rec["indices"], r64["indices"])
        rec["cond"] = np.float64(GS.rel_err(rec["out"], r64["out"]) if same else np.inf)
        rec["ties_robust"] = np.bool_(GS.ties_robust(rec["v"], rec["v_group"], rec["v_intra"]))
        return rec


def pair_distances(net, v):
    """the reference's dist_mat of one scene (GroupGenerator.forward, d_type 'learned_l2norm'), lower triangle"""
    with torch.no_grad():
        v_abs = torch.from_numpy(np.asarray(v, np.float32))[None, None]
        n = v_abs.size(-1)
        temp = net.group_gen.group_cnn(v_abs).unsqueeze(dim=-1).repeat_interleave(repeats=n, dim=-1)
        d = (temp - temp.transpose(-2, -1)).norm(p=2, dim=1).squeeze(dim=0).mean(dim=0)
    return d.numpy()[np.tril(np.ones((n, n), bool), -1)]


KEYS = ("v", "dist", "indices", "v_intra", "v_group", "out", "out0", "out1", "out2", "cond", "ties_robust")


def store_pick(out, tag, split, index, rec, th):
    from tests import _gpgraph_np as GN
    assert GN.pair_margin(rec["dist"].astype(np.float64), th) > GN.BAND_D, (tag, split, index)  # no undecided pair in a pick
    out[f"{tag}.split"], out[f"{tag}.index"] = np.asarray(split), np.int64(index)
    for key in KEYS:
        out[f"{tag}.{key}"] = rec[key]


def family(args):
    """G34 (--family): the reference's GPGraph around its social_stgcnn at every member of tests/_gpgraph_stgcnn_np.py:
    CONFIGS, under that configuration's seeded weights (GS.random_state, loaded with strict=True) and the case thresholds, on
    the graph-form scenes of 3 and 13 pedestrians (GS.graph_case; `max`: 3 only) -- each with the bridge's v_rel = v_abs and
    with the odd v_rel that no bridge builds.  Every case is run in fp32 and, the same modules converted with .double(), in
    fp64.  Stored per case <name>.<g3|g13>[odd], data only:
      .v_abs, .v_rel (T, n), .th, .dist (n, n), .indices, .v_group (T, G), .v_intra (T, n) (pass 0's input is .v_rel),
      .out (S, k, n) fp32, .cond (the reference's own fp32-against-fp64 difference, of the largest entry), .ties_robust
    and per configuration <name>.sums, the fp64 sum of every tensor of the generated state in the module's order: the weights
    are not stored, the tests regenerate them from the seed, and a drifted generator shows here before any kernel is blamed.
    Asserted before anything is written: v_abs, v_rel and th are GS.graph_case's, no pair is within 1e-5 th, and every case
    of 3 pedestrians with the bridge's v_rel has cond <= GS.COND and robust ties."""
    import json
    from tests import _gpgraph_np as GN
    from tests import _gpgraph_stgcnn_np as GS
    sys.path.insert(0, args.ref)
    os.chdir(args.ref)
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    from baseline.gpgraphstgcnn.model_baseline import social_stgcnn
    from baseline.gpgraphstgcnn.model_groupwrapper import GPGraph
    torch.set_num_threads(1)
    out, per_case = {}, {}
    for name, (n_st, n_tp, S, k) in GS.CONFIGS.items():
        sd = GS.random_state(name)
        out[f"{name}.sums"] = np.asarray([np.asarray(v, np.float64).sum() for v in sd.values()], np.float64)
        nets = []
        for _ in range(2):  # (the identity residuals are lambdas: the fp64 copy is built afresh, not deep-copied)
            base = social_stgcnn(n_stgcnn=n_st, n_txpcnn=n_tp, input_feat=1, output_feat=S, kernel_size=3, seq_len=k + 2,
                                 pred_seq_len=k)
            net = GPGraph(baseline_model=base, in_channels=1, out_channels=S, obs_seq_len=k + 2, pred_seq_len=k,
                          d_type="learned_l2norm", d_th="learned", mix_type="mlp", group_type=(True, True, True),
                          weight_share=True)
            net.load_state_dict({key: torch.from_numpy(v) for key, v in sd.items()}, strict=True)
            nets.append(net.eval())
        caps = [Capture(nets[0]), Capture(nets[1].double())]
        for which, odd in GS.graph_cases(name):
            if which == "gL1" or (name == "max" and which != "g3"):  # (S k = 2048: the scene of 3 keeps the file small)
                continue
            v_abs, v_rel, th = GS.graph_case(name, which, odd)
            recs = []
            for cap, dt in zip(caps, (torch.float32, torch.float64)):
                torch.set_default_dtype(dt)  # (the wrapper allocates its pooling buffers in the default dtype)
                try:
                    with torch.no_grad():
                        cap.net.group_gen.th.fill_(float(th))
                        cap.clear()
                        o, idx = cap.net(torch.from_numpy(v_abs).to(dt)[None, None], torch.from_numpy(v_rel).to(dt)[None, None])
                finally:
                    torch.set_default_dtype(torch.float32)
                assert len(cap.ins) == 3 and torch.equal(cap.ins[0][0, 0], torch.from_numpy(v_rel).to(dt))
                recs.append({"out": o[0].numpy(), "indices": idx.numpy().astype(np.int64), "dist": cap.dist.numpy(),
                             "v_group": cap.ins[1][0, 0].numpy(), "v_intra": cap.ins[2][0, 0].numpy()})
            rec, r64 = recs
            tag = f"{name}.{which}{'odd' if odd else ''}"
            assert rec["out"].dtype == np.float32 and rec["out"].shape == (S, k, v_abs.shape[1]), tag
            margin = GN.pair_margin(r64["dist"], float(th))
            assert margin > GN.BAND_D and np.array_equal(rec["indices"], r64["indices"]), (tag, margin)
            cond = GS.rel_err(rec["out"], r64["out"])
            robust = GS.ties_robust(v_rel, rec["v_group"], rec["v_intra"])
            if which == "g3" and not odd:
                assert cond <= GS.COND and robust, (tag, cond, robust)
            out[f"{tag}.v_abs"], out[f"{tag}.v_rel"], out[f"{tag}.th"] = v_abs, v_rel, np.float32(th)
            for key in ("dist", "indices", "v_group", "v_intra", "out"):
                out[f"{tag}.{key}"] = rec[key]
            out[f"{tag}.cond"], out[f"{tag}.ties_robust"] = np.float64(cond), np.bool_(robust)
            per_case[tag] = {"n": int(v_abs.shape[1]), "n_groups": int(rec["indices"].max()) + 1, "cond": cond,
                             "ties_robust": bool(robust), "pair_margin": margin, "largest_entry": float(np.abs(rec["out"]).max())}
            print(f"{tag}: n = {v_abs.shape[1]}, {per_case[tag]['n_groups']} groups, cond {cond:.2e}, ties_robust {robust}",
                  flush=True)
    path = os.path.join(args.out, "g34_gpgraph_stgcnn_family.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 512 * 1024, size
    manifest = {"g34_gpgraph_stgcnn_family": {
        "cases": sorted(per_case), "state_seed": GS.STATE_SEED, "configs": {n: list(c) for n, c in GS.CONFIGS.items()},
        "numpy": np.__version__, "torch": torch.__version__, "bytes": size, "per_case": per_case}}
    with open(os.path.join(args.out, "MANIFEST_g34_gpgraph_stgcnn_family.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")
    print("wrote", path, size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    ap.add_argument("--seed", type=int, default=1234, help="of the weights")
    ap.add_argument("--family", action="store_true",
                    help="write g34_gpgraph_stgcnn_family.npz (the members of tests/_gpgraph_stgcnn_np.py: CONFIGS) and leave "
                         "g22 alone")
    args = ap.parse_args()
    args.out = os.path.abspath(args.out)
    if args.family:
        return family(args)
    from tests import _golden as G
    from tests import _gpgraph_np as GN
    from tests import _gpgraph_stgcnn_np as GS
    from tests import _sgcn_np as SN
    sys.path.insert(0, args.ref)
    os.chdir(args.ref)

    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self

    from baseline.gpgraphstgcnn import model_forward_post_hook, model_forward_pre_hook
    from baseline.gpgraphstgcnn.model_baseline import social_stgcnn
    from baseline.gpgraphstgcnn.model_groupwrapper import GPGraph
    from EigenTrajectory import EigenTrajectory
    from utils.metrics import compute_batch_ade, compute_batch_fde
    from utils.utils import DotDict, get_exp_config

    def build(n_st, n_tp, S):
        base = social_stgcnn(n_stgcnn=n_st, n_txpcnn=n_tp, input_feat=1, output_feat=S, kernel_size=3, seq_len=8,
                             pred_seq_len=6)
        return GPGraph(baseline_model=base, in_channels=1, out_channels=S, obs_seq_len=8, pred_seq_len=6,
                       d_type="learned_l2norm", d_th="learned", mix_type="mlp", group_type=(True, True, True), weight_share=True)

    torch.set_num_threads(1)
    g2 = G.load("g2_fit_all_scenes.npz")
    t0 = time.time()
    torch.manual_seed(args.seed)
    predictor = build(1, 5, 20)
    randomise(predictor, torch.Generator().manual_seed(4321))
    predictor.eval()

    # ---- the network inputs of every scene (the wrapper's own projection and pre-hook; the predictor is not run yet)
    inputs = {}
    for scene in G.SCENES:
        hp = get_exp_config(f"./config/eigentrajectory-{{baseline}}-{scene}.json")
        assert hp.k == 6 and hp.num_samples == 20, (hp.k, hp.num_samples)
        seen = []

        def record_only(input_data, baseline_model):
            seen.append(input_data[0].detach().clone())
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
        which = range(len(sse)) if scene == "eth" else [int(np.argmax(sizes))]
        for i in which:
            s, e = sse[i]
            with torch.no_grad():
                model(torch.from_numpy(obs[s:e]))
        inputs[scene] = dict(model=model, hp=hp, which=list(which), seen=seen, obs=obs, pred=pred, sse=sse)
    synthetic = [SN.synthetic_v(n) for n in SN.RAGGED]
    C_obs, nrm = SN.synthetic_split(SN.SPLIT_SIZES, SN.SPLIT_SEED)
    lo = 0
    for n in SN.SPLIT_SIZES:
        synthetic.append(SN.scene_input(C_obs, nrm, lo, lo + n))
        lo += n

    # ---- the threshold
    pairs = np.sort(np.concatenate([pair_distances(predictor, v) for v in synthetic]).astype(np.float64))
    q5, q12 = np.quantile(pairs, [0.05, 0.12])
    win = pairs[(pairs >= q5) & (pairs <= q12)]
    at = int(np.argmax(np.diff(win)))
    th = float(np.float32(0.5 * (win[at] + win[at + 1])))
    margin = float(np.abs(pairs - th).min() / th)
    print(f"{pairs.size} pairs, smallest {pairs[0]:.4f}, median {np.median(pairs):.4f}; window [{q5:.4f}, {q12:.4f}] -> th = "
          f"{th:.6f}, relative margin {margin:.3e}", flush=True)
    assert margin > 10 * GN.BAND_D, margin
    with torch.no_grad():
        predictor.group_gen.th.fill_(th)
    out = {"th_margin": np.float64(margin)}
    for key, val in predictor.state_dict().items():
        out[f"net.{key}"] = val.detach().clone().numpy()
    both = Both(predictor)

    # ---- the recorded runs
    picks, have_small = [], False
    for scene in G.SCENES:
        d = inputs[scene]
        captured = {}

        def forward_and_capture(input_data, baseline_model):
            captured["rec"] = both.run(input_data[0][0, 0].numpy())
            return torch.from_numpy(captured["rec"]["out"]), torch.from_numpy(captured["rec"]["indices"])

        d["model"].hook_func = DotDict(model_forward_pre_hook=model_forward_pre_hook, model_forward=forward_and_capture,
                                       model_forward_post_hook=model_forward_post_hook)
        ades, fdes, records = [], [], []
        for i in d["which"]:
            s, e = d["sse"][i]
            o, p = torch.from_numpy(d["obs"][s:e]), torch.from_numpy(d["pred"][s:e])
            with torch.no_grad():
                res = d["model"](o)
            rec = captured["rec"]
            ades.append(np.asarray(compute_batch_ade(res["recon_traj"], p), np.float32))
            fdes.append(np.asarray(compute_batch_fde(res["recon_traj"], p), np.float32))
            rec["margin"] = GN.pair_margin(rec["dist"].astype(np.float64), th)
            records.append((e - s, i, rec))
        if scene == "eth":
            out["eth.static_dist"] = np.float32(d["hp"].static_dist)
            out["eth.scene_size"] = np.asarray([r[0] for r in records], np.int64)
            out["eth.ade"], out["eth.fde"] = np.concatenate(ades), np.concatenate(fdes)
            out["eth.margin"] = np.asarray([r[2]["margin"] for r in records], np.float64)
            out["eth.cond"] = np.asarray([r[2]["cond"] for r in records], np.float64)
            out["eth.ties_robust"] = np.asarray([r[2]["ties_robust"] for r in records], bool)
            out["eth.n_groups"] = np.asarray([int(r[2]["indices"].max()) + 1 for r in records], np.int64)
            good = (out["eth.margin"] > GN.BAND_D) & out["eth.ties_robust"] & (out["eth.cond"] <= GS.COND)
            print(f"eth: {int(good.sum())} of {good.size} scenes decided, ties_robust and cond <= {GS.COND}; largest cond "
                  f"{out['eth.cond'].max():.3e}, not ties_robust {int((~out['eth.ties_robust']).sum())}", flush=True)
            assert good.mean() >= 0.9, good.mean()
        chosen = [max(records, key=lambda r: r[0])]
        small = [r for r in records if r[0] <= 2]
        if small and not have_small:
            chosen.append(small[0])
            have_small = True
        for size, idx, rec in chosen:
            if size <= 2:
                assert rec["cond"] <= GS.COND and rec["ties_robust"], (scene, idx, rec["cond"], rec["ties_robust"])
            store_pick(out, f"pick{len(picks)}", scene, idx, rec, th)
            picks.append(f"pick{len(picks)}")
        big = chosen[0][2]
        print(f"{scene}: {len(records)} scenes, largest {chosen[0][0]} ({int(big['indices'].max()) + 1} groups, cond "
              f"{big['cond']:.2e}, ties_robust {bool(big['ties_robust'])})  ({time.time() - t0:.0f} s)", flush=True)
    assert have_small

    # ---- the hand-built scenes: d(i, j) depends on x_i - x_j only and is 1-homogeneous in it
    rng = np.random.default_rng(21)
    x0 = SN.synthetic_v(1)[:, 0]
    delta = rng.normal(0, 1, x0.shape).astype(np.float32)
    unit = pair_distances(predictor, np.stack([x0, x0 + delta], axis=1))[0]
    for name, (pos, expect) in HAND.items():
        v = np.stack([x0 + np.float32(a * th / unit) * delta for a in pos], axis=1).astype(np.float32)
        rec = both.run(v)
        assert rec["indices"].tolist() == expect, (name, rec["indices"], expect, rec["dist"] / th)
        assert GN.pair_margin(rec["dist"].astype(np.float64), th) > 0.05
        assert rec["cond"] <= GS.COND and rec["ties_robust"], (name, rec["cond"], rec["ties_robust"])
        store_pick(out, f"pick{len(picks)}", "hand", len(picks), rec, th)
        out[f"pick{len(picks)}.name"] = np.asarray(name)
        picks.append(f"pick{len(picks)}")
        print(f"hand-built {name}: indices {rec['indices'].tolist()}, cond {rec['cond']:.2e}", flush=True)

    # ---- the generic loop structure: another number of st_gcns and of tpcnns, another output width
    torch.manual_seed(99)
    gen_net = build(2, 3, 12)
    randomise(gen_net, torch.Generator().manual_seed(77))
    with torch.no_grad():
        gen_net.group_gen.group_cnn[0].load_state_dict(predictor.group_gen.group_cnn[0].state_dict())  # (th's distances)
        gen_net.group_gen.th.fill_(th)
    gen_net.eval()
    gboth = Both(gen_net)
    for key, val in gen_net.state_dict().items():
        out[f"gen.{key}"] = val.detach().numpy()
    grouped = [t for t in picks if 3 <= out[f"{t}.v"].shape[-1] <= 8
               and int(out[f"{t}.indices"].max()) + 1 < out[f"{t}.v"].shape[-1]]
    assert len(grouped) >= 2, grouped
    for i, tag in enumerate(sorted(grouped, key=lambda t: -out[f"{t}.v"].shape[-1])[:2]):
        rec = gboth.run(out[f"{tag}.v"])
        assert rec["cond"] <= GS.COND, (tag, rec["cond"])
        out[f"gen.pick{i}"] = np.asarray(tag)
        for key in ("out", "indices", "v_intra", "v_group", "cond"):
            out[f"gen.{key}{i}"] = rec[key]
    path = os.path.join(args.out, "g22_gpgraph_stgcnn_net.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "picks",
          [(str(out[f'{t}.split']), int(out[f'{t}.index']), out[f'{t}.v'].shape[-1], int(out[f'{t}.indices'].max()) + 1,
            f"{float(out[f'{t}.cond']):.1e}", bool(out[f'{t}.ties_robust'])) for t in picks])
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
