"""numpy restatement of csrc/et_dmrgcn.hip: the dmrgcn bridge's adjacency (baseline/dmrgcn/bridge.py:4-19), the disentangled
bins (dmrgcn.py:12-35), social_dmrgcn's eval-mode forward (dmrgcn.py, predictor.py) and the post-hook's permute, in fp64 from
a state_dict of numpy arrays.

The bins are taken ON THE fp32 DISTANCES: v_rel and |.| are formed in numpy fp32 as the bridge (and the device) forms them
and then compared with the split values; everything after the decision is fp64.  A time row's (n, n) distances are
handled in blocks of rows, and a bin's Laplacian is never formed (its action on the rows is a masked sum), so synthetic
scenes of thousands of pedestrians -- which no fixture can hold -- have something to compare with."""
import numpy as np

SPLIT = ((0.0, 0.25, 0.5, 0.75, 1.0), (0.0, 0.5, 1.0, 2.0, 4.0))  # predictor.py:68-69: [A_disp, A_dist]
LAST = 1e10                                                        # dmrgcn.py:29
ROWS = 512                                                         # rows of a time row's (n, n) block handled at once


def v_rel(v):
    """v (K, N) fp32 -> the displacement rows (bridge.py:8-9), fp32"""
    v = np.asarray(v, np.float32)
    rel = np.zeros_like(v)
    rel[1:] = v[1:] - v[:-1]
    return rel


def adjacency(v):
    """v (K, N) -> a (2, K, N, N) fp32 = [A_disp, A_dist], what the bridge's pre-hook hands the network (small scenes)"""
    v = np.asarray(v, np.float32)
    rel = v_rel(v)
    return np.stack([np.abs(rel[:, :, None] - rel[:, None, :]), np.abs(v[:, :, None] - v[:, None, :])])


def bins(dist, split, closed=False):
    """dist (..., fp32), split (5,) -> (5, ...) bool: bin b is lo < dist < hi (``closed``: lo <= dist <= hi -- NOT the
    reference's semantics, kept to show that the fixtures tell the two apart); the comparison is made in fp32."""
    dist = np.asarray(dist, np.float32)
    edges = np.asarray(list(split) + [LAST], np.float32)
    if closed:
        return np.stack([(dist >= edges[b]) & (dist <= edges[b + 1]) & (dist > 0) for b in range(len(split))])
    return np.stack([(dist > edges[b]) & (dist < edges[b + 1]) & (dist > 0) for b in range(len(split))])


def _prelu(x, a):
    return np.where(x > 0, x, float(np.asarray(a).reshape(-1)[0]) * x)


def _conv33(x, w, b):
    """x (Cin, H, W), w (Cout, Cin, 3, 3) zero-padded 'same' convolution"""
    cin, h, wd = x.shape
    xp = np.zeros((cin, h + 2, wd + 2))
    xp[:, 1:-1, 1:-1] = x
    out = np.zeros((w.shape[0], h, wd)) + np.asarray(b, np.float64)[:, None, None]
    for dh in range(3):
        for dw in range(3):
            out += np.einsum("oi,ihw->ohw", w[:, :, dh, dw], xp[:, dh:dh + h, dw:dw + wd])
    return out


def _contract(X, dist_rows, split, closed):
    """One relation, one time row.  X (J, n) fp64 rows to contract, dist_rows(lo, hi) -> (hi - lo, n) fp32 distances of
    rows [lo, hi) -> P (5, J, n): P[b, j, w] = sum_v L_b[w, v] X[j, v], L_b = I - D^-1/2 (A_b + I) D^-1/2."""
    J, n = X.shape
    nb = len(split)
    cnt = np.zeros((nb, n))
    for lo in range(0, n, ROWS):
        cnt[:, lo:lo + ROWS] = bins(dist_rows(lo, min(n, lo + ROWS)), split, closed).sum(axis=2)
    dinv = (1.0 + cnt) ** -0.5                      # A_b + I: every degree is >= 1
    P = np.empty((nb, J, n))
    for lo in range(0, n, ROWS):
        hi = min(n, lo + ROWS)
        M = bins(dist_rows(lo, hi), split, closed)  # (5, rows, n); the diagonal (distance 0) is in no bin
        for b in range(nb):
            # (D (A + I) D X)[w] = d_w (sum_v A[w,v] d_v X[v] + d_w X[w])
            ax = (X * dinv[b]) @ M[b].T.astype(np.float64)
            P[b, :, lo:hi] = X[:, lo:hi] - dinv[b, lo:hi] * (ax + dinv[b, lo:hi] * X[:, lo:hi])
    return P


def forward(sd, v, a=None, n_stgcn=1, n_tpcnn=4, split=SPLIT, closed=False):
    """sd: state_dict (numpy), v (K, N) fp32 -> raw output (S, k, N) (the network's (1, S, k, N) without the batch axis).
    a (2, K, N, N) given (read as it is) or None (formed from v in fp32, block by block)."""
    sd = {k: np.asarray(val, np.float64) for k, val in sd.items()}
    v32 = np.asarray(v, np.float32)
    rel32 = v_rel(v32)
    x = v32.astype(np.float64)[None]  # (C = 1, K, N)
    K, N = x.shape[1], x.shape[2]
    ones = np.ones((1, N))
    for i in range(n_stgcn):
        pre = f"st_dmrgcns.{i}"
        Cin = x.shape[0]
        S = sd[f"{pre}.tcn.1.weight"].shape[0]
        y = np.zeros((S, K, N))
        for r, src in enumerate((rel32, v32)):
            W = sd[f"{pre}.gcns.{r}.conv.weight"][:, :, 0, 0].reshape(len(split[r]), S, Cin)   # channel b S + c
            B = sd[f"{pre}.gcns.{r}.conv.bias"].reshape(len(split[r]), S)
            for t in range(K):
                if a is not None:
                    rows = lambda lo, hi, r=r, t=t: np.asarray(a[r][t][lo:hi], np.float32)
                else:
                    rows = lambda lo, hi, s=src[t]: np.abs(s[lo:hi, None] - s[None, :])
                P = _contract(np.concatenate([x[:, t], ones]), rows, split[r], closed)          # (5, Cin + 1, N)
                y[:, t] += np.einsum("bsc,bcw->sw", W, P[:, :Cin]) + np.einsum("bs,bw->sw", B, P[:, Cin])
        y = _prelu(y, sd[f"{pre}.tcn.0.weight"])
        tw, tb = sd[f"{pre}.tcn.1.weight"][:, :, :, 0], sd[f"{pre}.tcn.1.bias"]
        yp = np.zeros((S, K + 2, N))
        yp[:, 1:-1] = y
        z = tb[:, None, None] + sum(np.einsum("oc,ctv->otv", tw[:, :, dt], yp[:, dt:dt + K]) for dt in range(3))
        if f"{pre}.residual.0.weight" in sd:
            res = np.einsum("oc,ctv->otv", sd[f"{pre}.residual.0.weight"][:, :, 0, 0], x) + \
                sd[f"{pre}.residual.0.bias"][:, None, None]
        else:
            res = x
        x = _prelu(z + res, sd[f"{pre}.prelu.weight"])
    t = np.transpose(x, (1, 0, 2))                                         # a real permute: (K, S, N)
    for j in range(n_tpcnn):
        pre = f"tpcnns.{j}"
        if f"{pre}.residual.0.weight" in sd:
            res = np.einsum("oc,chw->ohw", sd[f"{pre}.residual.0.weight"][:, :, 0, 0], t) + \
                sd[f"{pre}.residual.0.bias"][:, None, None]
        else:
            res = t
        t = _prelu(_conv33(t, sd[f"{pre}.tpcn.0.0.weight"], sd[f"{pre}.tpcn.0.0.bias"]), sd[f"{pre}.tpcn.0.1.weight"]) + res
        t = _prelu(_conv33(t, sd[f"{pre}.tpcn.1.0.weight"], sd[f"{pre}.tpcn.1.0.bias"]), sd[f"{pre}.tpcn.1.1.weight"]) + t
        g = np.einsum("ost,tsw->ow", sd[f"{pre}.gtacn.0.0.weight"][:, :, :, 0], t) + sd[f"{pre}.gtacn.0.0.bias"][:, None]
        t = _prelu(g, sd[f"{pre}.gtacn.0.1.weight"])[None] + t              # the one row broadcast over the k rows
    return np.ascontiguousarray(np.transpose(t, (1, 0, 2)))                # (S, k, N)


def c_pred_refine(raw):
    """raw (S, k, N) -> (k, N, S) (bridge.py:40)"""
    return np.ascontiguousarray(np.transpose(raw, (1, 2, 0)))


def scene_input(C_obs, nrm, lo, hi):
    """v (k+2, n) of the rows [lo, hi) of a split: [C_obs; last observed position - its mean over the scene]"""
    ori = np.asarray(nrm[:2, lo:hi], np.float32)
    ori = ori - ori.mean(axis=1, keepdims=True, dtype=np.float32)
    return np.concatenate([np.asarray(C_obs[:, lo:hi], np.float32), ori]).astype(np.float32)
