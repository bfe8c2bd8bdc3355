#!/usr/bin/env python3
"""G16: the reference's TCC and COL (utils/metrics.py:105-155), per pedestrian, on the CPU in the build container.

    python tools/make_golden_tcc_col.py --ref /root/reference --out tests/golden

(a) cases: G9's seeded pred / gt as one scene, plus crafted scenes for each quirk of the metric -- motionless gt with an
    exact and an inexact mean (TCC's 0/0 and its rounding-noise case), a crossing pair whose closest approach falls at
    dense instant 13 (inside the 14-instant window) and at 14 (just outside), identical twins, a one-pedestrian scene, tied
    final errors, a NaN row and T = 3.  Stored per case: pred, gt, and the reference's per-pedestrian ADE, FDE, TCC, COL,
    the best sample (:114), per (sample, pedestrian) the collision bit (compute_batch_col on that sample alone) and the
    minimum distance to any other pedestrian over the window (the expression of :150-152, NaN pairs left out).
(b) G14's splits (every test scene of eth / hotel / zara1 / zara2, the tenth of univ) through the reference wrapper exactly
    as tools/make_golden_sgcn_full.py made G14 (its ADE / FDE are checked against G14's before anything is recorded), then
    the reference's compute_batch_tcc / compute_batch_col scene by scene (utils/trainer.py:183-190).  Stored per split:
    per-pedestrian TCC, COL, the split means, per (sample, pedestrian) collision bits and minimum distances, and a
    per-pedestrian flag for TCC rounding noise (a gt coordinate constant over the steps whose mean is not exact).

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


def window_min_dist(pred):
    """(S,N,T,2) -> (S,N): min over the other pedestrians of the pair's minimum same-instant distance over the window,
    utils/metrics.py:140-152's expression (NaN pairs left out; +inf without a partner)."""
    p = pred.permute(0, 2, 1, 3)
    rel = p[:, 1:] - p[:, :-1]
    dense = torch.cat([p[:, [0]], rel.div(4).unsqueeze(2).repeat_interleave(4, dim=2).reshape(
        p.size(0), 4 * (p.size(1) - 1), p.size(2), p.size(3))], dim=1).cumsum(dim=1)[:, :14]
    out = torch.full((p.size(0), p.size(2)), float("inf"))
    for i0 in range(0, p.size(2), 256):
        d = (dense[:, :, i0:i0 + 256, None] - dense[:, :, None, :]).norm(p=2, dim=-1).min(dim=1)[0]  # (S, b, N)
        idx = torch.arange(i0, min(i0 + 256, p.size(2)))
        d[:, idx - i0, idx] = float("inf")
        d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
        out[:, i0:i0 + 256] = d.min(dim=-1)[0]
    return out.numpy()


def noise_rows(gt):
    """(N,T,2) -> (N,) bool: a gt coordinate constant over the steps whose torch mean differs from the value."""
    g = torch.from_numpy(np.ascontiguousarray(gt))
    const = (g == g[:, :1]).all(dim=1)                           # (N, 2)
    exact = g.mean(dim=1) == g[:, 0]
    return (const & ~exact).any(dim=1).numpy()


def reference_metrics(M, pred, gt):
    """The reference's per-pedestrian metrics of one scene + per-(sample, pedestrian) collision bits."""
    p, g = torch.from_numpy(pred), torch.from_numpy(gt)
    temp = (p - g).norm(p=2, dim=-1)
    res = dict(ade=np.asarray(M.compute_batch_ade(p, g), np.float32), fde=np.asarray(M.compute_batch_fde(p, g), np.float32),
               tcc=np.asarray(M.compute_batch_tcc(p, g), np.float32), col=np.asarray(M.compute_batch_col(p, g), np.float32),
               best=temp[:, :, -1].argmin(dim=0).numpy().astype(np.int32))
    res["col_bits"] = np.stack([np.asarray(M.compute_batch_col(p[s:s + 1], g), np.float32) > 0
                                for s in range(p.shape[0])]).astype(np.uint8)
    res["min_dist"] = window_min_dist(p).astype(np.float32)
    return res


def crafted_cases(g9):
    rng = np.random.default_rng(16)
    cases = {"g9": (g9["pred"], g9["gt"])}

    def walk(n, T=12, S=20, spread=3.0):
        start = rng.uniform(-spread, spread, (n, 1, 2))
        vel = rng.normal(0, 0.4, (n, 1, 2))
        t = np.arange(T)[None, :, None]
        gt = (start + vel * t).astype(np.float32)
        pred = (gt[None] + rng.normal(0, 0.3, (S, n, T, 2))).astype(np.float32)
        return pred, gt

    # motionless gt: exact means (0.5, 2.0, 0.0) and values whose 12-term mean is inexact in fp32
    pred, gt = walk(8)
    vals = np.float32([0.5, 2.0, 0.0, 0.1, 0.3, 1.7, 3.3, 0.7])
    gt[:, :, 0] = vals[:, None]
    gt[:4, :, 1] = vals[::-1][:4, None]
    cases["motionless"] = (pred, gt)
    # crossing pair: x(t) = +-(v (t - t0)), closest approach at dense instant 13 and at 14 (outside the window)
    for name, inst in (("cross13", 13), ("cross14", 14)):
        T, S = 12, 2
        tt = np.arange(T, dtype=np.float32)
        t0 = inst / 4.0  # dense instant m sits at step m / 4
        a = np.stack([(tt - t0) * 1.0, np.full(T, 0.05, np.float32)], -1)  # one step = 4 instants = 2.0 apart in x
        b = np.stack([(tt - t0) * -1.0, np.full(T, -0.05, np.float32)], -1)
        gt = np.stack([a, b]).astype(np.float32)
        pred = np.repeat(gt[None], S, axis=0).copy()
        pred[1, 0, :, 1] += 0.5  # sample 1: the pair stays 1.1 apart in y
        pred[1, 1, :, 1] -= 0.5
        cases[name] = (pred.astype(np.float32), gt)
    pred, gt = walk(4, S=5)
    pred[:, 1] = pred[:, 0]
    gt[1] = gt[0]
    cases["twins"] = (pred, gt)
    cases["single"] = walk(1)
    pred, gt = walk(3, S=6)
    d = pred[:, :, -1] - gt[None, :, -1]
    pred[3, :, -1] = gt[:, -1] + d[1]  # samples 1 and 3 tie on the final error
    cases["ties"] = (pred, gt)
    pred, gt = walk(5, S=4)
    pred[2, 1, 7, 0] = np.nan  # one NaN point in one sample of row 1
    pred[:, 3, 2, 1] = np.nan  # row 3: NaN in every sample
    cases["nan"] = (pred, gt)
    cases["t3"] = walk(6, T=3, S=7, spread=0.4)
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    ap.add_argument("--skip-splits", action="store_true", help="write part (a) only")
    args = ap.parse_args()
    args.out = os.path.abspath(args.out)
    from tests import _golden as G
    sys.path.insert(0, args.ref)
    os.chdir(args.ref)
    torch.set_num_threads(1)
    import utils.metrics as M

    out = {}
    cases = crafted_cases(G.load("g9_metrics.npz"))
    out["cases"] = np.asarray(sorted(cases))
    for name, (pred, gt) in cases.items():
        res = reference_metrics(M, pred, gt)
        out[f"a.{name}.pred"], out[f"a.{name}.gt"] = pred, gt
        out[f"a.{name}.noise"] = noise_rows(gt)
        for key, val in res.items():
            out[f"a.{name}.{key}"] = val
        print(f"(a) {name}: N={gt.shape[0]} S={pred.shape[0]} T={gt.shape[1]} COL={res['col']} TCC={res['tcc'].round(4)}")

    if not args.skip_splits:
        torch.Tensor.cuda = lambda self, *a, **k: self
        torch.nn.Module.cuda = lambda self, *a, **k: self
        _zeros_like = torch.zeros_like

        def zeros_like_cpu(x, *a, **k):
            k.pop("device", None)
            return _zeros_like(x, *a, **k)
        torch.zeros_like = zeros_like_cpu
        from baseline.sgcn import TrajectoryPredictor, model_forward, model_forward_post_hook, model_forward_pre_hook
        from EigenTrajectory import EigenTrajectory
        from utils.utils import DotDict, get_exp_config

        g2, g14 = G.load("g2_fit_all_scenes.npz"), G.load("g14_sgcn_full_splits.npz")
        t0 = time.time()
        for scene in G.SCENES:
            hp = get_exp_config(f"./config/eigentrajectory-{{baseline}}-{scene}.json")
            torch.manual_seed(1234)  # as tools/make_golden_sgcn_full.py
            predictor = TrajectoryPredictor(number_asymmetric_conv_layer=7, embedding_dims=64, number_gcn_layers=1, dropout=0,
                                            obs_len=hp.k + 2, pred_len=hp.k, n_tcn=5, in_dims=1,
                                            out_dims=hp.num_samples).eval()
            hook = DotDict(model_forward_pre_hook=model_forward_pre_hook, model_forward=model_forward,
                           model_forward_post_hook=model_forward_post_hook)
            model = EigenTrajectory(predictor, hook, hp).eval()
            sd = model.state_dict()
            for key in list(sd):
                if key.startswith("ET_"):
                    sd[key] = torch.from_numpy(g2[f"{scene}.{key}"])
            model.load_state_dict(sd)
            obs, pred, sse = G.dataset(scene, "test")
            ades, fdes, tccs, cols, bits, mind, noise = [], [], [], [], [], [], []
            for i in g14[f"{scene}.scene_index"]:
                s, e = sse[int(i)]
                o, p = torch.from_numpy(obs[s:e]), torch.from_numpy(pred[s:e])
                with torch.no_grad():
                    rec = model(o)["recon_traj"]  # utils/trainer.py:183
                res = reference_metrics(M, rec.numpy(), pred[s:e])
                ades.append(res["ade"])
                fdes.append(res["fde"])
                tccs.append(res["tcc"])
                cols.append(res["col"])
                bits.append(res["col_bits"])
                mind.append(res["min_dist"])
                noise.append(noise_rows(pred[s:e]))
            ade, fde = np.concatenate(ades), np.concatenate(fdes)
            assert np.array_equal(ade, g14[f"{scene}.ade"]) and np.array_equal(fde, g14[f"{scene}.fde"]), scene
            tcc, col = np.concatenate(tccs), np.concatenate(cols)
            out[f"b.{scene}.tcc"], out[f"b.{scene}.col"] = tcc, col
            out[f"b.{scene}.col_bits"] = np.packbits(np.concatenate(bits, axis=1), axis=0)  # (ceil(S/8), N)
            out[f"b.{scene}.min_dist"] = np.concatenate(mind, axis=1).astype(np.float32)
            out[f"b.{scene}.noise"] = np.concatenate(noise)
            out[f"b.{scene}.tcc_col_mean"] = np.asarray([tcc.mean(dtype=np.float64), col.mean(dtype=np.float64)])
            print(f"(b) {scene}: {len(tcc)} pedestrians, TCC {tcc.mean():.5f} COL {col.mean():.5f}, "
                  f"{int(out[f'b.{scene}.noise'].sum())} noise rows ({time.time() - t0:.0f} s)", flush=True)
    path = os.path.join(args.out, "g16_tcc_col.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
