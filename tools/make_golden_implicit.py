#!/usr/bin/env python3
"""G25: ET-Implicit inference fixture -- the reference's wrapper + its implicit bridge + its SocialImplicitLight with the ET
constructor arguments (utils/trainer.py:547-564: spatial_input=1, spatial_output=S, temporal_input=k+2, temporal_output=k,
bins=[0, 0.01, 0.1, 1.2], noise_weight=[0.05, 1, 4, 8]), seeded, run on CPU in the build container.

    python tools/make_golden_implicit.py --ref <reference checkout> --out tests/golden

The reference moves its bins (and its normalizer's identity matrices) to the GPU with `.cuda()`; there is no GPU here, so
for the duration of this script `Tensor.cuda` / `Module.cuda` are the identity -- the arithmetic is the reference's own.
Before anything is recorded every cell's global_w, local_w and noise_w is set to its own random non-zero value: they
initialise to 0, which would make every output 0.  The ET descriptors and anchors are G2's
(tests/golden/g2_fit_all_scenes.npz), per split; they are not copied here.  Stored:
  net.<state_dict key>          the predictor's state_dict (one set for all splits: they share k = 6, S = 20)
  <split>.static_dist, .scene_size, .ade, .fde, .robust
                                per test scene / per pedestrian (best-of-S, the inference form model(obs), every test scene
                                of eth, hotel, univ, zara1, zara2, scene order).  robust (per scene): no pedestrian's
                                |C_obs[0]| is within 1e-5 max(1, b) of a non-zero bin value b, and no pedestrian's moving /
                                static decision is within 1e-5 of static_dist: a scene on which an input computed a few ulp
                                away puts every pedestrian in the same zone (a flipped zone changes the compacted
                                neighbours of its scene-mates too, hence per scene)
  pick<i>.{split,index,v,zone,net_out,c_pred_refine}
                                a handful of scenes: the network input v the bridge built, the zones (the reference's own
                                bucketize call on v), its raw output and the post-hook's C_pred_refine -- the largest scene
                                of each split, and the first scene whose pedestrians fall in at least three zones
  single.*, edges.*, lonely.*, nan.*
                                hand-built scenes through the reference's bridge and network: n = 1; n = 16 whose first
                                coefficients are 0, -0.0, +-0.01f, +-0.1f, +-1.2f and the fp32 neighbours either side of
                                the three non-zero bin values, interleaved so that every zone's members are non-adjacent
                                (these sixteen values put four members in every zone, so the zone with a single member is
                                in a scene of its own: lonely, n = 7, zone 1 has one member); nan: n = 8, one pedestrian's
                                first coefficient is NaN -- its zone as the reference's bucketize gives it, and net_out
                                with the NaNs where the reference has them
  gen.<state_dict key>, gen.v<i>, gen.net_out<i>
                                a second weight set, S = 12, T = 10, T_out = 5, bins [0, 0.5, 2], on synthetic 10-row
                                inputs with as many pedestrians as picks 0 and 1
The script asserts what the tests rely on: at least 95 % of the scenes of every split used end to end (END_TO_END below)
are robust, and the fp64 restatement (tests/_implicit_np.py) reproduces every recorded output within 1e-5 of its largest
entry, zones and NaN pattern exactly.  Only data is written; nothing of the reference is copied."""
import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

BINS = (0.0, 0.01, 0.1, 1.2)
NOISE_WEIGHT = (0.05, 1, 4, 8)
GEN = dict(spatial_input=1, spatial_output=12, temporal_input=10, temporal_output=5, bins=[0, 0.5, 2],
           noise_weight=[0.05, 1, 4])
MARGIN = 1e-5
END_TO_END = ("eth", "hotel", "univ", "zara1", "zara2")  # the splits tests/test_gpu_implicit.py compares row by row


def randomise(net, gen):
    """every cell's three scalars their own non-zero value, of either sign"""
    with torch.no_grad():
        for cell in net.implicit_cells:
            for w in (cell.global_w, cell.local_w, cell.noise_w):
                val = 0.4 + torch.rand(1, generator=gen)
                w.copy_(val if torch.rand(1, generator=gen) < 0.7 else -val)


def ref_zones(v, bins):
    """the reference's zone decision (model.py:149-151) on the bridge's v (1, 1, T, N)"""
    norm = torch.linalg.norm(v.permute(0, 3, 1, 2)[0, :, :, 0], float("inf"), dim=1)
    return (torch.bucketize(norm, bins, right=True) - 1).numpy().astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="a checkout of the reference implementation")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    args.out = os.path.abspath(args.out)  # (the reference reads its configuration relative to its own root)
    from tests import _golden as G
    from tests import _implicit_np as IN
    sys.path.insert(0, args.ref)
    os.chdir(args.ref)

    # no GPU in the build container: keep the reference's bins and normalizer on the CPU
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self

    from baseline.implicit import TrajectoryPredictor, model_forward, model_forward_post_hook, model_forward_pre_hook
    from EigenTrajectory import EigenTrajectory
    from utils.metrics import compute_batch_ade, compute_batch_fde
    from utils.utils import DotDict, get_exp_config

    torch.set_num_threads(1)
    g2 = G.load("g2_fit_all_scenes.npz")
    out = {}
    picks = []
    t0 = time.time()
    net_state = None
    three_zones = None
    for scene in G.SCENES:
        hp = get_exp_config(f"./config/eigentrajectory-{{baseline}}-{scene}.json")
        assert hp.k == 6 and hp.num_samples == 20, (hp.k, hp.num_samples)
        torch.manual_seed(1234)
        predictor = TrajectoryPredictor(spatial_input=1, spatial_output=hp.num_samples, temporal_input=hp.k + 2,
                                        temporal_output=hp.k, bins=list(BINS), noise_weight=list(NOISE_WEIGHT))
        randomise(predictor, torch.Generator().manual_seed(4321))
        predictor.eval()
        if net_state is None:
            net_state = {k: v.detach().clone() for k, v in predictor.state_dict().items()}
        captured = {}

        def forward_and_capture(input_data, baseline_model):
            captured["v"] = input_data[0].detach().clone()
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
        model.load_state_dict(sd)
        obs, pred, sse = G.dataset(scene, "test")
        ades, fdes, sizes, robust, records = [], [], [], [], []
        hist = np.zeros(len(BINS), np.int64)
        for i, (s, e) in enumerate(sse):
            o, p = torch.from_numpy(obs[s:e]), torch.from_numpy(pred[s:e])
            with torch.no_grad():
                res = model(o)  # the test loop's call (utils/trainer.py:183)
            ades.append(np.asarray(compute_batch_ade(res["recon_traj"], p), np.float32))
            fdes.append(np.asarray(compute_batch_fde(res["recon_traj"], p), np.float32))
            sizes.append(e - s)
            zone = ref_zones(captured["v"], predictor.bins)
            cap = {k: captured[k].numpy() for k in captured}
            cap["zone"] = zone
            hist += np.bincount(zone, minlength=len(BINS))
            first = np.abs(cap["v"][0, 0, 0].astype(np.float64))
            rob = all(bool((np.abs(first - b) > MARGIN * max(1.0, b)).all()) for b in BINS[1:])
            # the moving / static decision (EigenTrajectory/model.py: half the last two-frame displacement against static_dist)
            half = np.linalg.norm((obs[s:e, -1] - obs[s:e, -3]).astype(np.float64) / 2, axis=1)
            rob &= bool((np.abs(half - float(hp.static_dist)) > MARGIN).all())
            robust.append(rob)
            records.append((e - s, len(np.unique(zone)), i, cap))
        out[f"{scene}.static_dist"] = np.float32(hp.static_dist)
        out[f"{scene}.scene_size"] = np.asarray(sizes, np.int64)
        out[f"{scene}.ade"] = np.concatenate(ades)
        out[f"{scene}.fde"] = np.concatenate(fdes)
        out[f"{scene}.robust"] = np.asarray(robust, np.bool_)
        largest = max(records, key=lambda r: r[0])
        chosen = [largest]
        if three_zones is None:
            tz = [r for r in records if r[1] >= 3 and r[2] != largest[2]]
            if tz:
                three_zones = tz[0]
                chosen.append(tz[0])
        for size, nz, idx, cap in chosen:
            tag = f"pick{len(picks)}"
            picks.append(tag)
            out[f"{tag}.split"] = np.asarray(scene)
            out[f"{tag}.index"] = np.int64(idx)
            out[f"{tag}.zone"] = cap["zone"]
            for key in ("v", "net_out", "c_pred_refine"):
                out[f"{tag}.{key}"] = cap[key].astype(np.float32)
        print(f"{scene}: {len(sse)} scenes, {sum(sizes)} pedestrians, largest {largest[0]}, zones {hist.tolist()}, robust "
              f"{np.mean(robust):.4f}, ADE {out[f'{scene}.ade'].mean():.5f} FDE {out[f'{scene}.fde'].mean():.5f}  "
              f"({time.time() - t0:.0f} s)", flush=True)
    assert three_zones is not None
    for key, val in net_state.items():
        out[f"net.{key}"] = val.numpy()

    # hand-built scenes through the reference's bridge and network (the last split's predictor: the same weights)
    rng = np.random.default_rng(25)
    f32 = np.float32
    up = lambda x: np.nextafter(f32(x), f32(np.inf))
    down = lambda x: np.nextafter(f32(x), f32(-np.inf))
    by_zone = [[f32(0.0), f32(-0.0), down(0.01), -down(0.01)], [f32(0.01), -f32(0.01), up(0.01), down(0.1)],
               [f32(0.1), -f32(0.1), up(0.1), down(1.2)], [f32(1.2), -f32(1.2), up(1.2), -up(1.2)]]
    edges = rng.normal(0, 1, (8, 16)).astype(np.float32)
    edges[0] = np.asarray([by_zone[i % 4][i // 4] for i in range(16)], np.float32)  # zones 0, 1, 2, 3, 0, 1, ...
    single = np.asarray([[0.5], [-1.25], [2.0], [0.0], [3.0], [-0.75], [1.5], [-2.0]], np.float32)
    lonely = rng.normal(0, 1, (8, 7)).astype(np.float32)
    lonely[0] = np.asarray([0.5, 2.0, -0.3, 0.05, 1.5, 0.7, -3.0], np.float32)      # zones 2, 3, 2, 1, 3, 2, 3
    nan = rng.normal(0, 1, (8, 8)).astype(np.float32)
    nan[0] = np.asarray([1.5, 0.5, -2.0, 3.0, 0.05, np.nan, 0.3, -1.25], np.float32)  # zone 3: 0, 2, 3, NaN, 7
    hand = {"single": single, "edges": edges, "lonely": lonely, "nan": nan}
    for tag, v in hand.items():
        with torch.no_grad():
            inp = model_forward_pre_hook(torch.from_numpy(v[:6]), torch.from_numpy(v[6:]))
            res = model_forward(inp, predictor)
            out[f"{tag}.v"] = inp[0].numpy()
            out[f"{tag}.zone"] = ref_zones(inp[0], predictor.bins)
            out[f"{tag}.net_out"] = res.numpy()
            out[f"{tag}.c_pred_refine"] = model_forward_post_hook(res).numpy()
    assert np.array_equal(out["edges.zone"], np.arange(16) % 4), out["edges.zone"]
    assert np.array_equal(out["lonely.zone"], [2, 3, 2, 1, 3, 2, 3]) and out["single.zone"].tolist() == [2]
    nan_cols = np.isnan(out["nan.net_out"][0]).any(axis=(0, 1))
    print("nan: zone", out["nan.zone"].tolist(), "NaN columns", np.flatnonzero(nan_cols).tolist())
    assert nan_cols.any() and not nan_cols.all()

    # a second shape: S = 12, T = 10, T_out = 5, three bins
    torch.manual_seed(99)
    gen_net = TrajectoryPredictor(**GEN)
    randomise(gen_net, torch.Generator().manual_seed(77))
    gen_net.eval()
    for key, val in gen_net.state_dict().items():
        out[f"gen.{key}"] = val.detach().numpy()
    for i, tag in enumerate(picks[:2]):
        n = out[f"{tag}.v"].shape[-1]
        v = rng.normal(0, 1.5, (1, 1, 10, n)).astype(np.float32)
        with torch.no_grad():
            res = gen_net(torch.from_numpy(v))
        out[f"gen.v{i}"], out[f"gen.net_out{i}"] = v, res.numpy()
        assert len(np.unique(ref_zones(torch.from_numpy(v), gen_net.bins))) == 3

    # what the tests rely on
    for scene in END_TO_END:
        assert out[f"{scene}.robust"].mean() >= 0.95, (scene, out[f"{scene}.robust"].mean())
    sd_np = {k[4:]: v for k, v in out.items() if k.startswith("net.")}
    gen_np = {k[4:]: v for k, v in out.items() if k.startswith("gen.") and k[4:].startswith("implicit_cells")}
    worst = 0.0

    def check(got, ref):
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        return float(np.nanmax(np.abs(got - ref)) / np.nanmax(np.abs(ref)))

    for tag in picks + list(hand):
        v = out[f"{tag}.v"][0, 0]
        assert np.array_equal(IN.zones(v), out[f"{tag}.zone"]), tag
        raw = IN.forward(sd_np, v)
        worst = max(worst, check(raw, out[f"{tag}.net_out"][0].astype(np.float64)),
                    check(IN.c_pred_refine(raw), out[f"{tag}.c_pred_refine"].astype(np.float64)))
    for i in range(2):
        worst = max(worst, check(IN.forward(gen_np, out[f"gen.v{i}"][0, 0], bins=GEN["bins"]),
                                 out[f"gen.net_out{i}"][0].astype(np.float64)))
    print(f"fp64 restatement against the recorded outputs: {worst:.2e} of the largest entry")
    assert worst <= 1e-5, worst
    path = os.path.join(args.out, "g25_implicit.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "picks", [(str(out[f'{t}.split']), int(out[f'{t}.index']),
                                                            out[f'{t}.v'].shape[-1], np.unique(out[f'{t}.zone']).tolist())
                                                           for t in picks])
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()
