"""fp64 numpy restatement of GP-Graph-STGCNN's eval-mode forward (baseline/gpgraphstgcnn: model_groupwrapper.py
GPGraph.forward around model_baseline.py's social_stgcnn, ET configuration), the arithmetic csrc/et_gpgraph_stgcnn.hip is
checked against.  Not a test module itself.  The grouping (distances, merge, compact) is tests/_gpgraph_np.py's, the
network's pieces (BatchNorm, PReLU, the 3x3 convolutions) are tests/_stgcnn_np.py's.

The base is the ORIGINAL Social-STGCNN: its gcn convolves to S channels and contracts time row t with its own Laplacian
(``einsum('nctv,tvw->nctw')``), where ET-STGCNN's (baseline/stgcnn/model.py, tests/_stgcnn_np.forward) convolves to S K
channels and contracts over all rows -- so :func:`base_forward` restates the st_gcn block itself and shares the rest.

Three kinds of hard decision are taken: ``d <= th`` on every pair (handled as in tests/_gpgraph_np.py: BAND_D, TOL_D),
``a == 0`` in the inverse-distance kernel, and the conditioning of ``1 / |u_i - u_j|``.  For the last two, :func:`forward`
can be fed the fp32 inputs of passes 1 and 2 an implementation used (``inputs=``), which are checked on their own by
:func:`check_inputs` against bounds that follow from fp32 arithmetic."""
import numpy as np

from . import _gpgraph_np as GN
from . import _stgcnn_np as ST

TOL = 1e-5             # outputs: of the largest entry
TOL_D = GN.TOL_D
BAND_D = GN.BAND_D
COND = 1e-6            # a scene whose reference fp32 run is within this of its fp64 run is *well conditioned*
_f = GN._f


def laplacian_row(u, same=None):
    """u (N,) one time row -> L (N, N) = I - D a_hat D, a_hat = (1/|u_i - u_j|, 0 where equal) * same + I: the mask
    multiplies a_inv BEFORE + I, so it enters the degree as well"""
    u = np.asarray(u, np.float64)
    dist = np.abs(u[:, None] - u[None, :])
    with np.errstate(divide="ignore"):
        a_hat = np.where(dist == 0, 0.0, 1.0 / dist)
    if same is not None:
        a_hat = a_hat * np.asarray(same, np.float64)
    a_hat += np.eye(len(u))
    d = a_hat.sum(axis=1) ** -0.5
    return np.eye(len(u)) - d[:, None] * a_hat * d[None, :]


def n_layers(sd):
    n_st = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("st_gcns."))
    n_tp = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("tpcnns."))
    return n_st, n_tp


def base_forward(sd, v, same=None):
    """model_baseline.py's social_stgcnn.forward on v (K, N) with a = laplacian(v, mask = same) -> (S, k, N)"""
    sd = {k: _f(val) for k, val in sd.items()}
    n_st, n_tp = n_layers(sd)
    x = _f(v)[None]                                                        # (C = 1, K, N)
    K, N = x.shape[1], x.shape[2]
    L = np.stack([laplacian_row(r, same) for r in _f(v)])                 # (K, N, N)
    for i in range(n_st):
        pre = f"st_gcns.{i}"
        W = sd[f"{pre}.gcn.conv.weight"][:, :, 0, 0]                       # (S, Cin)
        x1 = np.einsum("oc,ctv->otv", W, x) + sd[f"{pre}.gcn.conv.bias"][:, None, None]
        y = np.einsum("ctv,tvw->ctw", x1, L)
        S = y.shape[0]
        y = ST._prelu(ST._bn(y, sd, f"{pre}.tcn.0", (-1, 1, 1)), sd[f"{pre}.tcn.1.weight"])
        tw, tb = sd[f"{pre}.tcn.2.weight"][:, :, :, 0], sd[f"{pre}.tcn.2.bias"]
        yp = np.zeros((S, K + 2, N))
        yp[:, 1:-1] = y
        z = tb[:, None, None] + sum(np.einsum("oc,ctv->otv", tw[:, :, dt], yp[:, dt:dt + K]) for dt in range(3))
        z = ST._bn(z, sd, f"{pre}.tcn.3", (-1, 1, 1))
        if f"{pre}.residual.0.weight" in sd:
            r = np.einsum("oc,ctv->otv", sd[f"{pre}.residual.0.weight"][:, :, 0, 0], x) + \
                sd[f"{pre}.residual.0.bias"][:, None, None]
            r = ST._bn(r, sd, f"{pre}.residual.1", (-1, 1, 1))
        else:
            r = x
        x = ST._prelu(z + r, sd[f"{pre}.prelu.weight"])
    S = x.shape[0]
    t = x.reshape(K, S, N)                                                 # the reference's view, not a permute
    t = ST._prelu(ST._conv33(t, sd["tpcnns.0.weight"], sd["tpcnns.0.bias"]), sd["prelus.0.weight"])
    for j in range(1, n_tp - 1):
        t = ST._prelu(ST._conv33(t, sd[f"tpcnns.{j}.weight"], sd[f"tpcnns.{j}.bias"]), sd[f"prelus.{j}.weight"]) + t
    t = ST._conv33(t, sd["tpcnn_ouput.weight"], sd["tpcnn_ouput.bias"])  # (k, S, N)
    return t.reshape(S, t.shape[0], N)


def grouping(rest, v, close=None):
    """v (T, N) -> (dist, indices, v' (T, N), group means (T, G)) in fp64; ``close`` overrides the decisions d <= th"""
    v = _f(v)
    d = GN.distances(rest, v)
    th = GN.threshold(rest)
    indices = GN.compact(GN.merge_rows(d <= th if close is None else np.asarray(close, bool)))
    sig = 1.0 / (1.0 + np.exp((d - th) / 0.1))
    v_soft = v @ (sig / sig.sum(axis=0, keepdims=True))
    v2 = (v - v_soft) + v_soft
    return d, indices, v2, group_means(v2, indices)


def group_means(v2, indices):
    G = int(indices.max()) + 1
    onehot = (np.asarray(indices)[:, None] == np.arange(G)[None]).astype(np.float64)
    return (_f(v2) @ onehot) / onehot.sum(axis=0)


def mix(rest, stack):
    S, k, N = stack[0].shape
    x = np.concatenate(stack, axis=0).reshape(3 * S * k, N)
    w = _f(rest["group_mix.st_gcns_mix.1.weight"])[:, :, 0, 0]
    a = float(np.asarray(rest["group_mix.st_gcns_mix.0.weight"]).reshape(-1)[0])
    y = w @ np.where(x > 0, x, a * x) + _f(rest["group_mix.st_gcns_mix.1.bias"])[:, None]
    return (stack[0] + stack[1] + stack[2]) / 3.0 + y.reshape(S, k, N)


def forward(sd, v, inputs=None, indices=None):
    """v (T, N) -> dict: out (S, k, N), outs [(S, k, n_m)] * 3 (pass 1 on the G group means, before the unpooling),
    indices, dist.  ``inputs`` = (group means (T, G), v' (T, N)) with ``indices``: passes 1 and 2 run on THESE values (an
    implementation's own fp32 ones) instead of this module's."""
    base, rest = GN.split_state(sd)
    d, own_idx, v2, means = grouping(rest, v)
    if inputs is not None:
        means, v2 = _f(inputs[0]), _f(inputs[1])
        own_idx = np.asarray(indices)
    same = own_idx[:, None] == own_idx[None, :]
    outs = [base_forward(base, v), base_forward(base, means), base_forward(base, v2, same)]
    out = mix(rest, [outs[0], outs[1][:, :, own_idx], outs[2]])
    return {"out": out, "outs": outs, "indices": own_idx, "dist": d, "n_groups": int(own_idx.max()) + 1}


# ---------------------------------------------------------------------------------------------- ties and input bounds
def ties(x):
    """x (T, n) fp32 -> (T, n, n) bool: the exact off-diagonal ties of every row (where a == 0 makes a_inv 0)"""
    x = np.asarray(x, np.float32)
    return (x[:, :, None] == x[:, None, :]) & ~np.eye(x.shape[1], dtype=bool)[None]


def ties_robust(v, v_group, v_intra):
    """every exact off-diagonal tie of the three graph inputs is at value 0.0 ((0 - s) + s == 0 for any s) -- or, in v and v',
    between two pedestrians whose whole columns of v are identical (their distances, sig_norm columns and v' columns are then
    computed from identical values by identical operations)"""
    v = np.asarray(v, np.float32)
    twins = (v[:, :, None] == v[:, None, :]).all(axis=0)
    for x, allowed in ((v, twins), (v_group, None), (v_intra, twins)):
        x = np.asarray(x, np.float32)
        t = ties(x) & (np.broadcast_to(x[:, :, None], (x.shape[0], x.shape[1], x.shape[1])) != 0)
        if allowed is not None:
            t &= ~allowed[None]
        if t.any():
            return False
    return True


def check_inputs(v, v2, means, indices):
    """the bounds that fp32 arithmetic gives the inputs of passes 1 and 2 (v' and the group means as an implementation
    computed them, fp32) -> the two largest ratios error / bound (both must be <= 1):
      |v'[t,j] - v[t,j]| <= 3 * 2^-23 * max_i |v[t,i]|        (v_soft is a convex combination of the row)
      |mean_g - fp64 mean of THE GIVEN v' over THE GIVEN indices| <= (count_g + 1) * 2^-24 * max |v'[t,.]|"""
    v, v2, means, indices = _f(v), _f(v2), _f(means), np.asarray(indices)
    b1 = 3 * 2.0 ** -23 * np.abs(v).max(axis=1, keepdims=True)
    r1 = float((np.abs(v2 - v) / np.maximum(b1, 1e-300)).max())
    counts = np.bincount(indices)
    b2 = (counts[None, :] + 1) * 2.0 ** -24 * np.abs(v2).max(axis=1, keepdims=True)
    r2 = float((np.abs(means - group_means(v2, indices)) / np.maximum(b2, 1e-300)).max())
    return r1, r2


def rel_err(got, ref):
    ref = _f(ref)
    return float(np.abs(_f(got) - ref).max() / max(np.abs(ref).max(), 1e-30))
