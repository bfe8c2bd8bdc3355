"""numpy restatement of csrc/et_stgcnn.hip: the stgcnn bridge's adjacency (baseline/stgcnn/bridge.py:4-21), social_stgcnn's
eval-mode forward (model.py) and the post-hook's permute, in fp64 from a state_dict of numpy arrays.

The Laplacian of a time row is formed from v one row at a time (never (K, N, N) at once), so synthetic scenes of thousands
of pedestrians -- which no fixture can hold -- have something to compare with."""
import numpy as np


def laplacian_row(u):
    """u (N,) one time row of v -> L (N, N) = I - D a_hat D, a_hat = 1/|u_i - u_j| (0 where equal) + I"""
    u = np.asarray(u, np.float64)
    dist = np.abs(u[:, None] - u[None, :])
    with np.errstate(divide="ignore"):
        a_hat = np.where(dist == 0, 0.0, 1.0 / dist)
    a_hat += np.eye(len(u))
    d = a_hat.sum(axis=1) ** -0.5
    return np.eye(len(u)) - d[:, None] * a_hat * d[None, :]


def adjacency(v):
    """v (K, N) -> (K, N, N), what the bridge's pre-hook hands the network (for small scenes)"""
    return np.stack([laplacian_row(r) for r in np.asarray(v, np.float64)])


def _bn(x, sd, pre, axis_shape):
    w, b, m, var = (np.asarray(sd[f"{pre}.{n}"], np.float64).reshape(axis_shape)
                    for n in ("weight", "bias", "running_mean", "running_var"))
    return (x - m) / np.sqrt(var + 1e-5) * w + b


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


def forward(sd, v, a=None, n_stgcnn=1, n_txpcnn=5):
    """sd: state_dict (numpy), v (K, N) -> raw output (S, k, N) (the network's (1, S, k, N) without the batch axis).
    a (K, N, N) given or None (formed from v row by row)."""
    sd = {k: np.asarray(val, np.float64) for k, val in sd.items()}
    x = np.asarray(v, np.float64)[None]  # (C=1, K, N)
    K, N = x.shape[1], x.shape[2]
    for i in range(n_stgcnn):
        pre = f"st_gcns.{i}"
        W = sd[f"{pre}.gcn.conv.weight"][:, :, 0, 0]                   # (S K, Cin)
        S = W.shape[0] // K
        x1 = np.einsum("oc,ctv->otv", W, x) + sd[f"{pre}.gcn.conv.bias"][:, None, None]
        x1 = x1.reshape(K, S, K, N)                                       # (kk, c, t, v)
        y = np.zeros((S, K, N))
        for kk in range(K):
            L = a[kk].astype(np.float64) if a is not None else laplacian_row(v[kk])
            y += np.einsum("ctv,vw->ctw", x1[kk], L)
        y = _prelu(_bn(y, sd, f"{pre}.tcn.0", (-1, 1, 1)), sd[f"{pre}.tcn.1.weight"])
        tw, tb = sd[f"{pre}.tcn.2.weight"][:, :, :, 0], sd[f"{pre}.tcn.2.bias"]
        yp = np.zeros((S, K + 2, N))
        yp[:, 1:-1] = y
        z = tb[:, None, None] + sum(np.einsum("oc,ctv->otv", tw[:, :, dt], yp[:, dt:dt + K]) for dt in range(3))
        z = _bn(z, sd, f"{pre}.tcn.3", (-1, 1, 1))
        if f"{pre}.residual.0.weight" in sd:
            r = np.einsum("oc,ctv->otv", sd[f"{pre}.residual.0.weight"][:, :, 0, 0], x) + \
                sd[f"{pre}.residual.0.bias"][:, None, None]
            r = _bn(r, sd, f"{pre}.residual.1", (-1, 1, 1))
        else:
            r = x
        x = _prelu(z + r, sd[f"{pre}.prelu.weight"])
    S = x.shape[0]
    t = x.reshape(K, S, N)                                                 # the reference's view, not a permute
    t = _prelu(_conv33(t, sd["tpcnns.0.weight"], sd["tpcnns.0.bias"]), sd["prelus.0.weight"])
    for j in range(1, n_txpcnn - 1):
        t = _prelu(_conv33(t, sd[f"tpcnns.{j}.weight"], sd[f"tpcnns.{j}.bias"]), sd[f"prelus.{j}.weight"]) + t
    t = _conv33(t, sd["tpcnn_ouput.weight"], sd["tpcnn_ouput.bias"])      # (k, S, N)
    k = t.shape[0]
    return t.reshape(S, k, N)


def c_pred_refine(raw):
    """raw (S, k, N) -> (k, N, S) (bridge.py:42)"""
    return np.ascontiguousarray(np.transpose(raw, (1, 2, 0)))


def scene_input(C_obs, nrm, lo, hi):
    """v (k+2, n) of the rows [lo, hi) of a split: [C_obs; last observed position - its mean over the scene]"""
    ori = np.asarray(nrm[:2, lo:hi], np.float32)
    ori = ori - ori.mean(axis=1, keepdims=True, dtype=np.float32)
    return np.concatenate([np.asarray(C_obs[:, lo:hi], np.float32), ori]).astype(np.float32)
