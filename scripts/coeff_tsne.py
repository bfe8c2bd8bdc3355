#!/usr/bin/env python3
"""The reference's script/plot_coeff_tsne.py on the GPU, for the five ETH/UCY splits: per split the train set (not
augmented), TrajNorm(ori=True, rot=True, sca=False), rank-6 SVD coefficients C_obs of the observed part, K-means with 20
clusters (sklearn's recipe: anchor.sklearn_style_kmeans) and the 2-D t-SNE of C_obs (eigentrajectory_amd.tsne.TSNE, the
reference's TSNE(n_components=2, random_state=42) with exact repulsion).

    python scripts/coeff_tsne.py [--raw DATASET_ROOT] [--out DIR] [--png] [--scenes eth,univ]

Prints the reference's lines (k, num params, obs error, pred error; number of clusters) and writes
<out>/coeff_tsne_<scene>.npz with C_obs, labels, embedding, kl and n_iter; with --png also a scatter plot, if
matplotlib imports."""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from eigentrajectory_amd import ops  # noqa: E402
from eigentrajectory_amd.anchor import sklearn_style_kmeans  # noqa: E402
from eigentrajectory_amd.tsne import TSNE  # noqa: E402

SCENES = ["eth", "hotel", "univ", "zara1", "zara2"]


def load_train(scene, raw=None, dev=None):
    """-> obs (N,8,2), pred (N,12,2) of a split's train set on `dev`: from a dataset tree (<raw>/<scene>/train/*.txt)
    or from the committed fixtures (tests/golden/data)."""
    if raw:
        from eigentrajectory_amd.data import TrajectoryData
        d = TrajectoryData(os.path.join(raw, scene, "train"))
        return d.obs_traj.to(dev), d.pred_traj.to(dev)
    from tests import _golden as G
    obs, pred, _ = G.dataset(scene, "train")
    return torch.from_numpy(obs).to(dev), torch.from_numpy(pred).to(dev)


def coefficients(obs, pred, k=6):
    """-> C_obs (N,k) and the reference's obs / pred reconstruction errors for rank k."""
    g_obs, g_pred, _ = ops.fit_gram(obs, pred, ops.MODE_STATIC, which=0)
    (U_obs, _), (U_pred, _) = ops.eigh_topk_batch([g_obs, g_pred], k)
    c_obs, c_pred, nrm, _ = ops.norm_project(obs, pred, None, None, U_obs, U_pred, ops.MODE_STATIC, want_flag=False)
    r_obs = ops.anchor_reconstruct(c_obs.unsqueeze(-1), None, None, None, U_obs, ops.MODE_STATIC, nrm=nrm)[0]
    r_pred = ops.anchor_reconstruct(c_pred.unsqueeze(-1), None, None, None, U_pred, ops.MODE_STATIC, nrm=nrm)[0]
    errs = ((r_obs - obs).norm(p=2, dim=-1).mean().item(), (r_pred - pred).norm(p=2, dim=-1).mean().item())
    return c_obs.t().contiguous(), errs


def clusters(C, n_clusters=20):
    """KMeans(n_clusters, random_state=0, init='k-means++', n_init=10).fit(C).labels_ on the device."""
    Ct = C.t().contiguous()
    centres, _, _ = sklearn_style_kmeans(Ct, n_clusters, random_state=0, n_init=10)
    return ops.kmeans_predict(Ct, centres, want_maxsims=False)[0]


def run_scene(obs, pred, k=6, n_clusters=20):
    """-> dict C_obs, errs, labels, embedding, kl, n_iter for one split."""
    C, errs = coefficients(obs, pred, k)
    labels = clusters(C, n_clusters)
    ts = TSNE(n_components=2, random_state=42)
    emb = ts.fit_transform(C)
    return {"C_obs": C.cpu().numpy(), "errs": errs, "labels": labels.cpu().numpy(), "embedding": emb,
            "kl": ts.kl_divergence_, "n_iter": ts.n_iter_}


def save_png(path, emb, labels, scene):
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        print("matplotlib is not available: no PNG written")
        return
    n = int(labels.max()) + 1
    plt.figure(figsize=(12, 10))
    plt.scatter(emb[:, 0], emb[:, 1], c=labels, cmap=plt.get_cmap("tab20" if n <= 20 else "hsv", n), s=8, alpha=0.7,
                edgecolors="none")
    plt.title(f"t-SNE Visualization of {n} Clusters for {scene}")
    plt.xlabel("t-SNE Dimension 1")
    plt.ylabel("t-SNE Dimension 2")
    plt.tight_layout()
    plt.savefig(path, dpi=300)
    plt.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--raw", default=None, help="dataset root with <scene>/train/*.txt (default: tests/golden fixtures)")
    ap.add_argument("--out", default="output_vis")
    ap.add_argument("--png", action="store_true")
    ap.add_argument("--scenes", default=",".join(SCENES))
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    os.makedirs(args.out, exist_ok=True)
    for scene in args.scenes.split(","):
        print(f"Scene: {scene}")
        obs, pred = load_train(scene, args.raw, dev)
        r = run_scene(obs, pred)
        print(f"k: 6\tnum params: 6\tobs error: {r['errs'][0]:.4f}\tpred error: {r['errs'][1]:.4f}")
        print(f"Number of clusters: {len(np.unique(r['labels']))}")
        print(f"t-SNE: KL divergence {r['kl']:.4f} after {r['n_iter'] + 1} iterations")
        np.savez(os.path.join(args.out, f"coeff_tsne_{scene}.npz"), C_obs=r["C_obs"], labels=r["labels"],
                 embedding=r["embedding"], kl=np.float64(r["kl"]), n_iter=np.int64(r["n_iter"]))
        if args.png:
            save_png(os.path.join(args.out, f"EigenTrajectory_k_clusters_tSNE_{scene}.png"), r["embedding"],
                     r["labels"], scene)


if __name__ == "__main__":
    main()
