"""numpy restatement of csrc/et_graphtern.hip: the graphtern bridge's S_obs = [abs, rel] (baseline/graphtern/bridge.py:4-14),
generate_adjacency_matrix's four relations (model.py:7-15), graph_tern_light's eval-mode forward (model.py:243-264 with the
blocks of stmrgcn.py and normalizer.py) and the post-hook's squeeze, in fp64 from a state_dict of numpy arrays.

The distances are taken ON THE fp32 INPUT: |x_i - x_j| is formed in numpy fp32 as the reference (and the device) forms it,
and ``A == 0 -> A_inv = 0`` is decided on that fp32 number; the inverse, the degrees and everything after them are fp64.
The number of st_mrgcn and epcnn blocks is read off the state_dict's keys, so the same code runs the ET configuration
(1 + 6) and any other member of the family."""
import numpy as np

HIDDEN = 16      # model.py:229
PAD_MODE = "edge"  # replicate padding; "constant" is NOT the reference's, kept to show that the fixtures tell them apart


def rel_of(u):
    """u (T, N) fp32 -> the displacement rows (bridge.py:9-10), fp32: rel[0] = 0, rel[t] = u[t] - u[t-1]"""
    u = np.asarray(u, np.float32)
    rel = np.zeros_like(u)
    rel[1:] = u[1:] - u[:-1]
    return rel


def s_obs_of(u):
    """u (T, N) -> S_obs (1, 2, T, N, 1) fp32 = [abs, rel], what the bridge's pre-hook hands the network"""
    u = np.asarray(u, np.float32)
    return np.stack([u, rel_of(u)])[None, :, :, :, None]


def distances(x):
    """x (T, N) fp32 -> (T, N, N) fp32 |x_i - x_j| (the reference's norm over a dimension of size 1)"""
    x = np.asarray(x, np.float32)
    return np.abs(x[:, :, None] - x[:, None, :])


def _prelu(x, a):
    return np.where(x > 0, x, float(np.asarray(a).reshape(-1)[0]) * x)


def _conv33_replicate(x, w, b):
    """x (Cin, H, W), w (Cout, Cin, 3, 3): 'same' convolution, replicate padding (stmrgcn.py:70, 80)"""
    cin, h, wd = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1)), mode=PAD_MODE)
    out = np.zeros((w.shape[0], h, wd)) + np.asarray(b, np.float64)[:, None, None]
    for dh in range(3):
        for dw in range(3):
            out += np.einsum("oi,ihw->ohw", w[:, :, dh, dw], xp[:, dh:dh + h, dw:dw + wd])
    return out


def _normalised(A):
    """A (n, n) fp64 -> D^-1/2 (A + I) D^-1/2, D the row sums of A + I, an infinite D^-1/2 set to 0 (normalizer.py:7-21)"""
    At = A + np.eye(A.shape[0])
    with np.errstate(divide="ignore"):
        d = At.sum(axis=1) ** -0.5
    d[np.isinf(d)] = 0.0
    return (d[:, None] * At) * d[None, :]


def graphs(u, rel):
    """u, rel (T, N) fp32 -> (4, T, N, N) fp64 normalised graphs of [A_abs, A_rel, 1 / A_abs, 1 / A_rel]"""
    out = []
    for src in (u, rel):
        A32 = distances(src)
        out.append(A32.astype(np.float64))
    for A in list(out):
        with np.errstate(divide="ignore"):
            inv = 1.0 / A
        inv[A == 0] = 0.0
        out.append(inv)
    return np.stack([np.stack([_normalised(A[t]) for t in range(A.shape[0])]) for A in out])


def counts(sd):
    """-> (n_epgcn, n_epcnn) of a state_dict"""
    n_gcn = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("tp_mrgcns."))
    n_cnn = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("tpcnns."))
    return n_gcn, n_cnn


def forward(sd, u, rel=None):
    """sd: state_dict (numpy), u (T, N) fp32 (S_obs[0, 0, :, :, 0]), rel (T, N) fp32 as given (S_obs[0, 1, :, :, 0]) or None
    (formed from u in fp32) -> (k, N, S) fp64: the network's (1, k, N, S) without the batch axis, which is also what the
    post-hook's squeeze returns (C_pred_refine)."""
    sd = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    u32 = np.asarray(u, np.float32)
    rel32 = rel_of(u32) if rel is None else np.asarray(rel, np.float32)
    n_gcn, n_cnn = counts(sd)
    L = graphs(u32, rel32)                                                   # (4, T, N, N)
    x = u32.astype(np.float64)[None]                                         # (C = 1, T, N): V_obs_abs
    for i in range(n_gcn):
        pre = f"tp_mrgcns.{i}"
        W, B = sd[f"{pre}.gcn.conv.weight"][:, :, 0, 0], sd[f"{pre}.gcn.conv.bias"]
        xr = (np.einsum("oc,ctv->otv", W, x) + B[:, None, None]).reshape(4, HIDDEN, x.shape[1], x.shape[2])
        y = np.einsum("rtwv,rctv->ctw", L, xr)
        y = _prelu(y, sd[f"{pre}.tcn.0.weight"])
        tw, tb = sd[f"{pre}.tcn.1.weight"][:, :, :, 0], sd[f"{pre}.tcn.1.bias"]
        T = y.shape[1]
        yp = np.zeros((HIDDEN, T + 2, y.shape[2]))
        yp[:, 1:-1] = y
        z = tb[:, None, None] + sum(np.einsum("oc,ctv->otv", tw[:, :, dt], yp[:, dt:dt + T]) for dt in range(3))
        if f"{pre}.residual.0.weight" in sd:
            res = np.einsum("oc,ctv->otv", sd[f"{pre}.residual.0.weight"][:, :, 0, 0], x) + \
                sd[f"{pre}.residual.0.bias"][:, None, None]
        else:
            res = x
        x = z + res                                                          # use_mdn: the block's own prelu is NOT applied
    t = np.transpose(x, (1, 0, 2))                                           # (T, 16, N)
    for j in range(n_cnn):
        pre = f"tpcnns.{j}"
        res = t
        if f"{pre}.restconv.0.weight" in sd:
            res = np.einsum("ot,tcv->ocv", sd[f"{pre}.restconv.0.weight"][:, :, 0, 0], res) + \
                sd[f"{pre}.restconv.0.bias"][:, None, None]
        if f"{pre}.rescconv.0.weight" in sd:
            res = np.einsum("oc,tcv->tov", sd[f"{pre}.rescconv.0.weight"][:, :, 0, 0], res) + \
                sd[f"{pre}.rescconv.0.bias"][None, :, None]
        t = _prelu(_conv33_replicate(t, sd[f"{pre}.tpcns.0.0.weight"], sd[f"{pre}.tpcns.0.0.bias"]),
                   sd[f"{pre}.tpcns.0.1.weight"])                            # (k, 16, N): time rows as channels
        c = np.transpose(t, (1, 0, 2))                                       # (16, k, N)
        c = _prelu(_conv33_replicate(c, sd[f"{pre}.cpcns.0.0.weight"], sd[f"{pre}.cpcns.0.0.bias"]),
                   sd[f"{pre}.cpcns.0.1.weight"])                            # (C_out, k, N)
        t = np.transpose(c, (1, 0, 2)) + res                                 # (k, C_out, N)
    return np.ascontiguousarray(np.transpose(t, (0, 2, 1)))                  # (k, N, S)


def scene_input(C_obs, nrm, lo, hi):
    """u (k+2, n) of the rows [lo, hi) of a split: [C_obs; last observed position - its mean over the scene]"""
    ori = np.asarray(nrm[:2, lo:hi], np.float32)
    ori = ori - ori.mean(axis=1, keepdims=True, dtype=np.float32)
    return np.concatenate([np.asarray(C_obs[:, lo:hi], np.float32), ori]).astype(np.float32)
