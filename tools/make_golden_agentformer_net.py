#!/usr/bin/env python3
"""G26: ET-AgentFormer network fixture -- the reference's AgentFormerLight with the ET settings (utils/trainer.py:387-392 on
top of baseline/agentformer/agentformer_pre.yml: past_frames = k + 2, future_frames = k, motion_dim = 1, forecast_dim = S,
input_type ['pos'], pred_type 'pos', nz = 0, no learnt prior; 256 / 512 / 8 heads, 2 + 2 layers), run on the CPU
with GENERATED weights.

    python tools/make_golden_agentformer_net.py --ref <reference checkout> --out tests/golden

The weights are not the reference's initialisation: after construction its layers 0 and 1 hold identical tensors (the layer
is deep-copied) and every in_proj bias is zero, which would hide swapped layers and dropped biases.  Every tensor is drawn
by tests/_agentformer_np.py: make_weights(keys, shapes, seed) and loaded into the reference; the fixture stores the key and
shape lists, the seed and every tensor's fp64 sum -- not the weights (14.7 MB at the ET size).  Stored:
  et.keys, et.shapes, et.seed, et.sums, et.nhead, et.pe_enc, et.pe_dec     (gen.* the same for the generic configuration)
                                the state_dict's keys in order, their shapes (padded to 3 with zeros), the generator's seed,
                                the sums, and the first past_frames rows of both pe buffers
  et.<scene>.u, .seq_out        pre_motion (T, n) and the reference's _seq_out (k, n, S): univ57 (the largest univ test
                                scene), univ_mid (the first univ test scene of 17 to 31 pedestrians), n1, n2, n16, n17, n128
                                (hand-built; at n = 128 the same-pedestrian entries lie on the diagonal of every 16 x 16 score
                                tile whose key block is congruent to the query block mod 8, at 17 and 57 they cross tile edges)
  gen.<scene>.u, .seq_out       n1, n2, n16, n17 under model_dim 64, 4 heads, ff 96, 1 encoder + 3 decoder layers, k = 4, S = 3
  ref_fp32_err                  per recorded output, against the reference's own float64 run, over the largest entry
  <split>.static_dist, .scene_index, .scene_size, .ade, .fde, .robust
                                per-pedestrian best-of-S ADE / FDE of the reference's wrapper + bridge + this network (G2
                                descriptors, the inference form model(obs)) for every test scene of eth and hotel and every
                                tenth of univ; robust (per scene): no pedestrian's moving / static decision is within 1e-5
                                of static_dist
The script asserts what the tests rely on: the fp64 restatement (tests/_agentformer_np.py) is within 1e-5 of the largest
entry of every recorded output, in its one-pass and its k-pass form; ref_fp32_err <= 2.5e-6; every mutant of the
restatement misses every recorded output it can affect by more than 1e-3, and the only vacuous cases are the ones named in
VACUOUS below.  Only data is written; nothing of the reference is copied."""
import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

SEED_ET, SEED_GEN = 2601, 2602
GEN = dict(tf_model_dim=64, tf_nhead=4, tf_ff_dim=96, context_encoder={"nlayer": 1}, future_decoder={"nlayer": 3})
GEN_K, GEN_S = 4, 3
MARGIN = 1e-5
END_TO_END = {"eth": 1, "hotel": 1, "univ": 10}  # split -> every how-manieth test scene
# (mutant, scene) pairs on which a mutant cannot change anything, and why -- asserted to be exactly the vacuous ones
VACUOUS = {}


def hand_scene(rng, T, n):
    return rng.normal(0, 1.0, (T, n)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="a checkout of the reference implementation")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    args.out = os.path.abspath(args.out)
    from tests import _agentformer_np as AN
    from tests import _golden as G
    sys.path.insert(0, args.ref)
    os.chdir(args.ref)
    torch.Tensor.cuda = lambda self, *a, **k: self  # no GPU where the fixture is made
    torch.nn.Module.cuda = lambda self, *a, **k: self

    from baseline.agentformer import (TrajectoryPredictor, model_forward, model_forward_post_hook,
                                      model_forward_pre_hook)
    from baseline.agentformer.utils.config import Config
    from EigenTrajectory import EigenTrajectory
    from utils.metrics import compute_batch_ade, compute_batch_fde
    from utils.utils import DotDict, get_exp_config

    torch.set_num_threads(4)
    t0 = time.time()

    def build(k, S, seed, **over):
        cfg = Config("./baseline/agentformer/agentformer_pre.yml")
        cfg.past_frames, cfg.future_frames = k + 2, k
        cfg.motion_dim, cfg.forecast_dim = 1, S
        cfg.input_type, cfg.pred_type, cfg.sn_out_type, cfg.scene_orig_all_past = ['pos'], 'pos', None, False
        cfg.nz, cfg.ar_train, cfg.learn_prior = 0, False, False
        for key, val in over.items():
            setattr(cfg, key, val)
        net = TrajectoryPredictor(cfg).eval()
        sd = net.state_dict()
        keys, shapes = list(sd), [tuple(v.shape) for v in sd.values()]
        drawn = AN.make_weights(keys, shapes, seed)
        net.load_state_dict({key: sd[key] if drawn[key] is None else torch.from_numpy(drawn[key]) for key in keys},
                            strict=True)
        sd_np = {key: val.detach().numpy().copy() for key, val in net.state_dict().items()}
        return net, cfg, keys, shapes, sd_np

    def run(net, u, double=False):
        """the bridge's call on pre_motion (T, n, 1) -> _seq_out (k, n, S)"""
        t = torch.from_numpy(np.asarray(u))
        t = t.double() if double else t
        with torch.no_grad():
            data = model_forward({"pre_motion": t.unsqueeze(-1).contiguous()}, net)
        return data["_seq_out"].numpy().copy(), data["_dec_motion"].numpy().copy()

    out = {}
    worst_rest, worst_loop, ref_errs = 0.0, 0.0, {}
    mutant_min = {m: np.inf for m in AN.MUTANTS}
    vacuous = {}

    def record(tag, net, net64, sd_np, nhead, scenes):
        nonlocal worst_rest, worst_loop
        for name, u in scenes.items():
            seq, dec = run(net, u)
            assert np.array_equal(dec, np.transpose(seq, (1, 0, 2)))  # _dec_motion is the transpose, nothing more
            seq64, _ = run(net64, u, double=True)
            scale = np.abs(seq64).max()
            ref_errs[f"{tag}.{name}"] = float(np.abs(seq - seq64).max() / scale)
            out[f"{tag}.{name}.u"], out[f"{tag}.{name}.seq_out"] = u, seq
            mine = AN.forward(sd_np, u, nhead)
            worst_rest = max(worst_rest, float(np.abs(mine - seq).max() / np.abs(seq).max()))
            if u.shape[1] <= 17:
                worst_loop = max(worst_loop, float(np.abs(AN.forward(sd_np, u, nhead, loop=True) - mine).max()))
            if u.shape[1] <= 57:
                for m in AN.MUTANTS:
                    miss = float(np.abs(AN.forward(sd_np, u, nhead, mutant=m) - seq).max() / np.abs(seq).max())
                    if miss <= 1e-3:
                        vacuous[(m, f"{tag}.{name}")] = miss
                    else:
                        mutant_min[m] = min(mutant_min[m], miss)
            print(f"  {tag}.{name}: n = {u.shape[1]}, fp32 vs fp64 {ref_errs[f'{tag}.{name}']:.2e}  ({time.time() - t0:.0f} s)",
                  flush=True)

    def header(tag, keys, shapes, seed, sd_np, nhead, T):
        out[f"{tag}.keys"] = np.asarray(keys)
        out[f"{tag}.shapes"] = np.asarray([list(s) + [0] * (3 - len(s)) for s in shapes], np.int64)
        out[f"{tag}.seed"], out[f"{tag}.nhead"] = np.int64(seed), np.int64(nhead)
        out[f"{tag}.sums"] = np.asarray([sd_np[key].astype(np.float64).sum() for key in keys], np.float64)
        out[f"{tag}.pe_enc"] = sd_np["context_encoder.pos_encoder.pe"][:T, 0].copy()
        out[f"{tag}.pe_dec"] = sd_np["future_decoder.pos_encoder.pe"][:T, 0].copy()

    # ---- the ET configuration (k = 6, S = 20 in all five splits)
    hp = get_exp_config("./config/eigentrajectory-{baseline}-univ.json")
    assert hp.k == 6 and hp.num_samples == 20
    net, cfg, keys, shapes, sd_np = build(hp.k, hp.num_samples, SEED_ET)
    assert len(keys) == 84 and cfg.tf_model_dim == 256 and cfg.tf_ff_dim == 512 and cfg.tf_nhead == 8
    header("et", keys, shapes, SEED_ET, sd_np, cfg.tf_nhead, hp.k + 2)
    net64, *_ = build(hp.k, hp.num_samples, SEED_ET)
    net64 = net64.double()

    g2 = G.load("g2_fit_all_scenes.npz")
    univ_scenes = {}
    for scene, step in END_TO_END.items():
        hps = get_exp_config(f"./config/eigentrajectory-{{baseline}}-{scene}.json")
        assert hps.k == hp.k and hps.num_samples == hp.num_samples
        captured = {}

        def forward_and_capture(input_data, baseline_model):
            captured["u"] = input_data["pre_motion"][:, :, 0].detach().numpy().copy()
            return model_forward(input_data, baseline_model)

        hook = DotDict(model_forward_pre_hook=model_forward_pre_hook, model_forward=forward_and_capture,
                       model_forward_post_hook=model_forward_post_hook)
        model = EigenTrajectory(net, hook, hps).eval()
        sd = model.state_dict()
        for key in list(sd):
            if key.startswith("ET_"):
                sd[key] = torch.from_numpy(g2[f"{scene}.{key}"])
        model.load_state_dict(sd)
        obs, pred, sse = G.dataset(scene, "test")
        sizes = np.asarray(sse)[:, 1] - np.asarray(sse)[:, 0]
        want = set(range(0, len(sse), step))
        if scene == "univ":
            largest = int(np.argmax(sizes))
            mid = int(np.flatnonzero((sizes >= 17) & (sizes <= 31))[0])
            want |= {largest, mid}
        ades, fdes, robust, index = [], [], [], []
        for i in sorted(want):
            s, e = sse[i]
            o, p = torch.from_numpy(obs[s:e]), torch.from_numpy(pred[s:e])
            with torch.no_grad():
                res = model(o)
            if scene == "univ" and i in (largest, mid):
                univ_scenes["univ57" if i == largest else "univ_mid"] = captured["u"]
            if i % step:
                continue
            index.append(i)
            ades.append(np.asarray(compute_batch_ade(res["recon_traj"], p), np.float32))
            fdes.append(np.asarray(compute_batch_fde(res["recon_traj"], p), np.float32))
            half = np.linalg.norm((obs[s:e, -1] - obs[s:e, -3]).astype(np.float64) / 2, axis=1)
            robust.append(bool((np.abs(half - float(hps.static_dist)) > MARGIN).all()))
        out[f"{scene}.static_dist"] = np.float32(hps.static_dist)
        out[f"{scene}.scene_index"] = np.asarray(index, np.int64)
        out[f"{scene}.scene_size"] = sizes[index].astype(np.int64)
        out[f"{scene}.ade"], out[f"{scene}.fde"] = np.concatenate(ades), np.concatenate(fdes)
        out[f"{scene}.robust"] = np.asarray(robust, np.bool_)
        print(f"{scene}: {len(index)} scenes, {int(sizes[index].sum())} pedestrians, robust {np.mean(robust):.4f}, ADE "
              f"{out[f'{scene}.ade'].mean():.5f} FDE {out[f'{scene}.fde'].mean():.5f}  ({time.time() - t0:.0f} s)", flush=True)
        assert np.mean(robust) >= 0.95
    assert univ_scenes["univ57"].shape == (8, 57) and 17 <= univ_scenes["univ_mid"].shape[1] <= 31

    rng = np.random.default_rng(26)
    scenes = dict(univ_scenes)
    for n in (1, 2, 16, 17, 128):
        scenes[f"n{n}"] = hand_scene(rng, hp.k + 2, n)
    record("et", net, net64, sd_np, cfg.tf_nhead, scenes)

    # ---- a generic configuration: nothing in the kernels is tied to the ET shape
    gnet, gcfg, gkeys, gshapes, gsd = build(GEN_K, GEN_S, SEED_GEN, **GEN)
    header("gen", gkeys, gshapes, SEED_GEN, gsd, GEN["tf_nhead"], GEN_K + 2)
    gnet64, *_ = build(GEN_K, GEN_S, SEED_GEN, **GEN)
    record("gen", gnet, gnet64.double(), gsd, GEN["tf_nhead"], {f"n{n}": hand_scene(rng, GEN_K + 2, n) for n in (1, 2, 16, 17)})

    out["ref_fp32_err.names"] = np.asarray(list(ref_errs))
    out["ref_fp32_err"] = np.asarray(list(ref_errs.values()), np.float64)
    print(f"fp64 restatement against the recorded outputs: {worst_rest:.2e}; k-pass against one-pass form: {worst_loop:.2e}; "
          f"reference fp32 against its fp64: {max(ref_errs.values()):.2e}")
    print("smallest miss of every mutant:", {m: f"{v:.2e}" for m, v in mutant_min.items()})
    print("vacuous:", vacuous)
    assert worst_rest <= 1e-5 and worst_loop <= 1e-12, (worst_rest, worst_loop)
    assert max(ref_errs.values()) <= 2.5e-6
    assert set(vacuous) == set(VACUOUS), (vacuous, VACUOUS)
    assert all(np.isfinite(v) and v > 1e-3 for v in mutant_min.values())
    path = os.path.join(args.out, "g26_agentformer_net.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path))
    assert os.path.getsize(path) < 1000 * 1000


if __name__ == "__main__":
    main()
