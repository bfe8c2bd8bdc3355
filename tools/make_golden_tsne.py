#!/usr/bin/env python3
"""G18: sklearn's t-SNE (sklearn.manifold.TSNE, Barnes-Hut path) on the coefficients of the reference's
script/plot_coeff_tsne.py, on the CPU.

    python tools/make_golden_tsne.py --ref /path/to/reference --out tests/golden [--threads 16] [--skip-default]
    python tools/make_golden_tsne.py --edges --out tests/golden      (numpy and sklearn only, no reference tree)

C_obs is computed with the reference's own code: TrajNorm(ori=True, rot=True, sca=False) on the train split (not
augmented), rank-6 SVD of the normalised observed part, C_obs = (U[:, :6].T @ A).T.  Two files, each under 1 MiB:

g18_tsne.npz -- a fixed 2 000-row subset of eth train's pairwise distinct rows (`sub.idx`, seed `sub.seed`, `sub.X`):
  kNN (k = 91), per row: crc32 of the sorted fp32 squared distances (`sub.knn_dcrc`), crc32 of the sorted int32
  neighbour set (`sub.knn_icrc`), a tie at the k-th distance (`sub.knn_tie`, from a k+1 query), crc32 of the fp64
  conditional P in sklearn's column order (`sub.pcond_crc`); full values for 256 seeded rows (`sub.s_rows`,
  `sub.s_knn_i`, `sub.s_knn_d`, `sub.s_pcond`).  Symmetric P: `sub.P_indptr`, per-row crc32 of the int32 column
  indices (`sub.P_icrc`), per-row fp64 sums (`sub.P_rowsum`), the total before normalisation (`sub.P_total`), all
  entries of the 256 sample rows (`sub.s_P_off`, `sub.s_P_idx`, `sub.s_P_val`).
  `sub.Y0`: sklearn's init="pca" (random_state=42).  `emb.{y50,y400,yrand}`: the theta = 0 iterate after 50 and after
  400 iterations from Y0 and a unit-variance random embedding, with `_kl_divergence_bh(angle=0)`'s error and gradient
  at each (`kl.*`, `grad.*`) on the unexaggerated P, and the smallest pair distance (`emb.mind.*`).
  `run.*`: theta = 0 whole runs (max_iter 1000) from Y0 on sub.X and on sub.X moved by 1 ulp (two seeded sign
  patterns): final KL, n_iter, trustworthiness@10 (`run.kl`, `run.n_iter`, `run.tw`).
  `default.<scene>.{kl,n_iter,N}`: sklearn's default TSNE(n_components=2, random_state=42) on each split's train C_obs.
g18b_tsne_eth.npz -- full eth train: `X` (29 809 x 6 C_obs), 1 024 seeded sample rows `rows` with the same per-row
  crc32 / tie fields as the subset, and full values for the first 128 of them (`s_knn_i`, `s_knn_d`, `s_pcond`).

g18c_tsne_edges.npz (--edges) -- what sklearn's theta = 0 gradient does where embedding points coincide or nearly do, on
  seeded inputs: `X` (300 x 6, unit normal, seed `seed`), whose P (perplexity 30, k = 91) the restatement
  tests/_tsne_np.py reproduces bit for bit (asserted here; `P_crc`, `P_nnz`), and the embeddings of
  tests/_tsne_np.edge_embeddings(300, seed + 1) (`emb.<name>`): for each, `_kl_divergence_bh(angle=0)`'s error and
  gradient (`kl.<name>`, `grad.<name>` fp32).  `n2.*`: N = 2 with P = [[0, .5], [.5, 0]], the two points distinct
  (`n2.emb.far`) and equal (`n2.emb.eq`).  `zero.embedding`, `zero.n_iter`, `zero.kl`: TSNE(angle=0,
  init=zeros).fit on X.  MANIFEST.json gets the entry `g18c_tsne_edges` (sklearn / numpy versions, the KLs).

Only data is written; nothing of the reference is copied."""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

from tests import _golden as G  # noqa: E402

K = 91
SUB_SEED, SUB_N = 18, 2000


def c_obs_ref(TrajNorm, scene):
    import torch
    obs, _, _ = G.dataset(scene, "train")
    obs = torch.from_numpy(obs)
    n, t, d = obs.shape
    tn = TrajNorm(ori=True, rot=True, sca=False)
    tn.calculate_params(obs)
    A = tn.normalize(obs).reshape(n, t * d).T
    U, _, _ = torch.linalg.svd(A, full_matrices=False)
    return np.ascontiguousarray((U[:, :6].T @ A).T.numpy())


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def knn_rows(X, rows):
    """sklearn's kNN graph + conditional P, and per-row fields for `rows`."""
    from sklearn.manifold import _utils
    from sklearn.neighbors import NearestNeighbors
    nn = NearestNeighbors(n_neighbors=K).fit(X)
    g = nn.kneighbors_graph(mode="distance")
    g.data **= 2
    g.sort_indices()
    d32 = g.data.reshape(X.shape[0], -1).astype(np.float32)
    idx = g.indices.reshape(X.shape[0], -1).astype(np.int32)
    pc = _utils._binary_search_perplexity(d32, 30.0, 0)
    dk, _ = nn.kneighbors(X[rows], n_neighbors=K + 2)  # the query rows are in the fitted set: column 0 is self
    tie = dk[:, K] == dk[:, K + 1]
    f = {"knn_dcrc": np.array([crc(np.sort(d32[r])) for r in rows], np.uint32),
         "knn_icrc": np.array([crc(np.sort(idx[r])) for r in rows], np.uint32),
         "knn_tie": tie, "pcond_crc": np.array([crc(pc[r]) for r in rows], np.uint32)}
    return g, d32, idx, pc, f


EDGE_SEED, EDGE_N = 180, 300


def edges(out_dir, threads):
    """g18c: sklearn's compiled behaviour at coincident and nearly coincident embedding points"""
    import sklearn
    from scipy.sparse import csr_matrix
    from sklearn.manifold import TSNE
    from sklearn.manifold._t_sne import _joint_probabilities_nn, _kl_divergence_bh
    from sklearn.neighbors import NearestNeighbors
    from tests import _tsne_np as T
    n = EDGE_N
    X = np.random.default_rng(EDGE_SEED).standard_normal((n, 6)).astype(np.float32)
    k = T.n_neighbors(n)
    g = NearestNeighbors(n_neighbors=k).fit(X).kneighbors_graph(mode="distance")
    g.data **= 2
    P = _joint_probabilities_nn(g, 30.0, 0)
    idx, d32 = T.knn(X, k)
    ip, ix, Pn, _ = T.symmetrize(idx, T.binary_search_perplexity(d32, 30.0, exp=T.libm_exp))
    assert np.array_equal(ip, P.indptr) and np.array_equal(ix, P.indices) and np.array_equal(Pn, P.data)
    out = {"seed": np.int64(EDGE_SEED), "X": X, "P_crc": np.uint32(crc(P.data)), "P_nnz": np.int64(P.nnz)}
    kw = dict(angle=0.0, skip_num_points=0, verbose=0, num_threads=threads)
    embs = T.edge_embeddings(n, EDGE_SEED + 1)
    for name in ("dup", "d1e-7", "d9e-7", "d2e-6"):  # what the cases are meant to be
        hi, lo = T.pair_offsets(embs[name])
        want = {"dup": (0.0, 0.0), "d2e-6": (1e-6, 3e-6)}.get(name, (0.0, 1e-6))
        assert np.all(lo >= want[0]) and np.all(hi <= want[1]) and (name == "dup" or np.all(lo > 0.0)), name
    man = {"sklearn": sklearn.__version__, "numpy": np.__version__, "N": n, "kl": {}}
    for name, Y in embs.items():
        err, grad = _kl_divergence_bh(Y.ravel().copy(), P, 1, n, 2, compute_error=True, **kw)
        out[f"emb.{name}"], out[f"kl.{name}"] = Y, np.float64(err)
        out[f"grad.{name}"] = grad.reshape(n, 2).astype(np.float32)
        man["kl"][name] = repr(float(err))
        print(f"{name}: KL {err!r} max |grad| {np.abs(grad).max():.6g}", flush=True)
    P2 = csr_matrix(np.array([[0.0, 0.5], [0.5, 0.0]]))
    for name, Y in (("far", np.float32([[0.25, -0.5], [-1.0, 0.75]])), ("eq", np.float32([[0.3, -0.7], [0.3, -0.7]]))):
        err, grad = _kl_divergence_bh(Y.ravel().copy(), P2, 1, 2, 2, compute_error=True, **kw)
        out[f"n2.emb.{name}"], out[f"n2.kl.{name}"] = Y, np.float64(err)
        out[f"n2.grad.{name}"] = grad.reshape(2, 2).astype(np.float32)
        man["kl"]["n2." + name] = repr(float(err))
        print(f"n2.{name}: KL {err!r} grad {grad}", flush=True)
    ts = TSNE(n_components=2, random_state=42, angle=0.0, init=np.zeros((n, 2), np.float32))
    out["zero.embedding"] = ts.fit_transform(X).astype(np.float32)
    out["zero.n_iter"], out["zero.kl"] = np.int64(ts.n_iter_), np.float64(ts.kl_divergence_)
    print(f"init=zeros: n_iter {ts.n_iter_} KL {ts.kl_divergence_!r} max |embedding| {np.abs(ts.embedding_).max()}")
    path = os.path.join(out_dir, "g18c_tsne_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path))
    mpath = os.path.join(out_dir, "MANIFEST.json")
    with open(mpath) as f:
        m = json.load(f)
    m["g18c_tsne_edges"] = man
    with open(mpath, "w") as f:
        json.dump(m, f, indent=1, sort_keys=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref")
    ap.add_argument("--edges", action="store_true", help="write g18c_tsne_edges.npz only (numpy and sklearn, no --ref)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--skip-default", action="store_true", help="leave out the five default-TSNE runs (about 6 min)")
    args = ap.parse_args()
    if args.edges:
        return edges(args.out, args.threads)
    if not args.ref:
        ap.error("--ref is required without --edges")
    import torch
    torch.set_num_threads(args.threads)
    sys.path.insert(0, os.path.abspath(args.ref))
    from EigenTrajectory.normalizer import TrajNorm
    from sklearn.decomposition import PCA
    from sklearn.manifold import TSNE, trustworthiness
    from sklearn.manifold._t_sne import _gradient_descent, _joint_probabilities_nn, _kl_divergence_bh
    from sklearn.utils import check_random_state

    Xe = c_obs_ref(TrajNorm, "eth")
    # rows with pairwise distinct C_obs only (the first of each group of identical rows): without the stationary
    # duplicates no two points coincide along the run, where sklearn's tree and the exact sum differ
    _, first = np.unique(Xe, axis=0, return_index=True)
    rng = np.random.default_rng(SUB_SEED)
    sub_idx = np.sort(rng.choice(np.sort(first), SUB_N, replace=False)).astype(np.int32)
    X = np.ascontiguousarray(Xe[sub_idx])
    n = X.shape[0]
    out = {"sub.seed": np.int64(SUB_SEED), "sub.idx": sub_idx, "sub.X": X}

    # (1) affinities on the subset
    g, d32, idx, pc, f = knn_rows(X, np.arange(n))
    out.update({"sub." + k: v for k, v in f.items()})
    srows = np.sort(np.random.default_rng(SUB_SEED + 1).choice(n, 256, replace=False)).astype(np.int32)
    out.update({"sub.s_rows": srows, "sub.s_knn_i": idx[srows], "sub.s_knn_d": d32[srows], "sub.s_pcond": pc[srows]})
    from scipy.sparse import csr_matrix
    Pc = csr_matrix((pc.ravel(), g.indices, g.indptr), shape=(n, n))
    Ps = Pc + Pc.T
    out["sub.P_total"] = np.float64(Ps.sum())
    P = _joint_probabilities_nn(g, 30.0, 0)
    out["sub.P_indptr"] = P.indptr.astype(np.int32)
    out["sub.P_icrc"] = np.array([crc(P.indices[P.indptr[i]:P.indptr[i + 1]].astype(np.int32)) for i in range(n)],
                                 np.uint32)
    out["sub.P_rowsum"] = np.asarray(P.sum(axis=1)).ravel()
    offs = [0]
    si, sv = [], []
    for r in srows:
        a, b = P.indptr[r], P.indptr[r + 1]
        si.append(P.indices[a:b].astype(np.int32))
        sv.append(P.data[a:b])
        offs.append(offs[-1] + b - a)
    out.update({"sub.s_P_off": np.array(offs, np.int64), "sub.s_P_idx": np.concatenate(si),
                "sub.s_P_val": np.concatenate(sv)})
    print("(1) subset affinities done", flush=True)

    # (2) PCA init and the recorded embeddings
    rs = check_random_state(42)
    pca = PCA(n_components=2, svd_solver="randomized", random_state=rs)
    pca.set_output(transform="default")
    Y0 = pca.fit_transform(X).astype(np.float32, copy=False)
    Y0 = Y0 / np.std(Y0[:, 0]) * 1e-4
    out["sub.Y0"] = Y0
    lr = np.maximum(n / 12.0 / 4, 50)
    kw = dict(angle=0.0, skip_num_points=0, verbose=0, num_threads=args.threads)
    y50, _, _ = _gradient_descent(_kl_divergence_bh, Y0.ravel(), it=0, max_iter=50, n_iter_check=50, momentum=0.5,
                                  learning_rate=lr, n_iter_without_progress=250, min_grad_norm=1e-7,
                                  args=[P * 12.0, 1, n, 2], kwargs=dict(kw))
    t400 = TSNE(n_components=2, random_state=42, angle=0.0, max_iter=400, init=Y0.copy())
    y400 = t400.fit_transform(X).astype(np.float32)
    yr = np.random.default_rng(SUB_SEED + 2).standard_normal((n, 2)).astype(np.float32)
    for name, Y in (("y50", y50.reshape(n, 2)), ("y400", y400), ("yrand", yr)):
        Y = np.ascontiguousarray(Y, dtype=np.float32)
        d = np.sqrt(((Y[:, None, :].astype(np.float64) - Y[None, :, :]) ** 2).sum(-1))
        np.fill_diagonal(d, np.inf)
        err, grad = _kl_divergence_bh(Y.ravel(), P, 1, n, 2, compute_error=True, **kw)
        out[f"emb.{name}"], out[f"emb.mind.{name}"] = Y, np.float64(d.min())
        out[f"kl.{name}"], out[f"grad.{name}"] = np.float64(err), grad.reshape(n, 2).astype(np.float32)
        print(f"(2) {name}: KL {err:.6f} min pair distance {d.min():.3g}", flush=True)

    # (3) theta = 0 whole runs from Y0, on X and on X moved by 1 ulp
    kls, its, tws = [], [], []
    for s in range(3):
        Xs = X
        if s:
            sign = np.random.default_rng(SUB_SEED + 10 + s).integers(0, 2, X.shape).astype(bool)
            Xs = np.where(sign, np.nextafter(X, np.float32(np.inf)), np.nextafter(X, np.float32(-np.inf)))
        t0 = time.time()
        ts = TSNE(n_components=2, random_state=42, angle=0.0, init=Y0.copy())
        Y = ts.fit_transform(Xs)
        kls.append(ts.kl_divergence_)
        its.append(ts.n_iter_)
        tws.append(trustworthiness(X, Y, n_neighbors=10))
        print(f"(3) run {s}: KL {kls[-1]:.5f} n_iter {its[-1]} trustworthiness@10 {tws[-1]:.5f} "
              f"({time.time() - t0:.0f} s)", flush=True)
    out["run.kl"], out["run.n_iter"], out["run.tw"] = np.array(kls), np.array(its), np.array(tws)

    # (4) sklearn's default run on each split's train C_obs
    if not args.skip_default:
        for scene in G.SCENES:
            Xs = Xe if scene == "eth" else c_obs_ref(TrajNorm, scene)
            t0 = time.time()
            ts = TSNE(n_components=2, random_state=42)
            ts.fit_transform(Xs)
            out[f"default.{scene}.kl"], out[f"default.{scene}.n_iter"] = np.float64(ts.kl_divergence_), np.int64(ts.n_iter_)
            out[f"default.{scene}.N"] = np.int64(Xs.shape[0])
            print(f"(4) {scene}: N {Xs.shape[0]} KL {ts.kl_divergence_:.4f} n_iter {ts.n_iter_} "
                  f"({time.time() - t0:.0f} s)", flush=True)

    path = os.path.join(args.out, "g18_tsne.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path))

    # g18b: full eth train
    rows = np.sort(np.random.default_rng(SUB_SEED + 3).choice(Xe.shape[0], 1024, replace=False)).astype(np.int32)
    _, d32, idx, pc, f = knn_rows(Xe, rows)
    outb = {"X": Xe, "rows": rows, **f, "s_knn_i": idx[rows[:128]], "s_knn_d": d32[rows[:128]], "s_pcond": pc[rows[:128]]}
    path = os.path.join(args.out, "g18b_tsne_eth.npz")
    np.savez_compressed(path, **outb)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
