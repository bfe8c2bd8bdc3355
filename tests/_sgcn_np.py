"""fp64 numpy restatement of SGCN's eval-mode forward (baseline/sgcn/model.py: TrajectoryModel.forward with the ET
arguments in_dims = 1, num_heads = 4, embedding_dims = 64), the arithmetic csrc/et_sgcn.hip is checked against.  Not a
test module itself.

The network takes a hard decision, ``sigmoid(logit) > 0.5``, on every entry of its two interaction masks.  Two correct
implementations can disagree on it where the logit is within rounding of zero, so :func:`forward` takes ``decide=(dec_s,
dec_t, band)``: where ``|logit| < band`` the keep / drop decision is read from the boolean arrays, everywhere else it is
this module's own; the logits are returned next to the output so a test can compare them."""
import numpy as np

H, D = 4, 16  # heads, depth per head (embedding_dims 64 / num_heads 4)
SWA = "sparse_weighted_adjacency_matrices."


def _f(a):
    return np.asarray(a, np.float64)


def n_layers(sd):
    """-> (number_asymmetric_conv_layer, n_tcn) of a state dict"""
    na = len({k.split(".")[3] for k in sd if k.startswith(SWA + "interaction_mask.spatial_asymmetric_convolutions.")})
    nt = len({k.split(".")[1] for k in sd if k.startswith("tcns.")})
    return na, nt


def attention(sd, name, x):
    """SelfAttention(multi_head=True) on x (B, L) (one input channel) -> (B, H, L, L), softmax over the last axis"""
    p = SWA + name + "."
    e = x[..., None] * _f(sd[p + "embedding.weight"])[:, 0] + _f(sd[p + "embedding.bias"])  # (B, L, 64)
    q = e @ _f(sd[p + "query.weight"]).T + _f(sd[p + "query.bias"])
    k = e @ _f(sd[p + "key.weight"]).T + _f(sd[p + "key.bias"])
    B, L = x.shape
    q = q.reshape(B, L, H, D).transpose(0, 2, 1, 3)
    k = k.reshape(B, L, H, D).transpose(0, 2, 1, 3)
    a = q @ k.transpose(0, 1, 3, 2) / 8.0  # scaled_factor = sqrt(d_model = 64)
    a = np.exp(a - a.max(axis=-1, keepdims=True))
    return a / a.sum(axis=-1, keepdims=True)


def prelu(x, a):
    a = float(np.asarray(a).reshape(-1)[0])
    return np.where(x > 0, x, a * x)


def asymmetric(sd, p, x):
    """AsymmetricConvolution on x (B, 4, P, Q): PReLU(conv(1x3) + conv(3x1)) + x, zero padded, conv(3x1) without bias"""
    w1, w2, b2 = _f(sd[p + "conv1.weight"])[..., 0], _f(sd[p + "conv2.weight"])[:, :, 0], _f(sd[p + "conv2.bias"])
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    P, Q = x.shape[2], x.shape[3]
    acc = np.zeros_like(x) + b2[None, :, None, None]
    for d in range(3):
        acc += np.einsum("oc,bcpq->bopq", w2[:, :, d], xp[:, :, 1:1 + P, d:d + Q])
        acc += np.einsum("oc,bcpq->bopq", w1[:, :, d], xp[:, :, d:d + P, 1:1 + Q])
    return prelu(acc, sd[p + "activation.weight"]) + x


def conv33(x, w, b):
    """3x3 convolution, padding 1: x (B, Cin, P, Q), w (Cout, Cin, 3, 3)"""
    w, b = _f(w), _f(b)
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    P, Q = x.shape[2], x.shape[3]
    acc = np.zeros((x.shape[0], w.shape[0], P, Q)) + b[None, :, None, None]
    for dp in range(3):
        for dq in range(3):
            acc += np.einsum("oc,bcpq->bopq", w[:, :, dp, dq], xp[:, :, dp:dp + P, dq:dq + Q])
    return acc


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _mask(logit, dec, band, identity):
    keep = sigmoid(logit) > 0.5
    if dec is not None:
        keep = np.where(np.abs(logit) < band, np.asarray(dec, bool), keep)
    return np.where(keep, sigmoid(logit), 0.0) + _f(identity)[:, None]


def zero_softmax(x):
    e = (np.exp(x) - 1.0) ** 2
    return e / (e.sum(axis=-1, keepdims=True) + 1e-5)


def forward(sd, v, identity_s, identity_t, decide=None):
    """v (T, N) (the graph (1, T, N, 1) squeezed), identity_s (1 or T, N, N), identity_t (N, 1 or T, 1 or T) ->
    (out (pred_len, N, out_dims), logit_s (T, H, N, N), logit_t (N, H, T, T)), all fp64"""
    v = _f(v)
    T, N = v.shape
    na, nt = n_layers(sd)
    dec_s, dec_t, band = decide if decide is not None else (None, None, 0.0)
    dense_s = attention(sd, "spatial_attention", v)      # (T, H, N, N)
    dense_t = attention(sd, "temporal_attention", v.T)   # (N, H, T, T)
    # spa_fusion: 1x1 convolution over the T axis, PReLU, identity shortcut
    fw = _f(sd[SWA + "spa_fusion.conv.0.weight"])[:, :, 0, 0]
    fb = _f(sd[SWA + "spa_fusion.conv.0.bias"])
    xs = prelu(np.einsum("ut,thij->uhij", fw, dense_s) + fb[:, None, None, None], sd[SWA + "spa_fusion.conv.1.weight"])
    xs = xs + dense_s
    xt = dense_t
    for j in range(na):
        xs = asymmetric(sd, f"{SWA}interaction_mask.spatial_asymmetric_convolutions.{j}.", xs)
        xt = asymmetric(sd, f"{SWA}interaction_mask.temporal_asymmetric_convolutions.{j}.", xt)
    logit_s, logit_t = xs, xt
    A_s = zero_softmax(dense_s * _mask(logit_s, dec_s, band, identity_s))
    A_t = zero_softmax(dense_t * _mask(logit_t, dec_t, band, identity_t))

    def gcn(name, i):
        return _f(sd[f"stsgcn.{name}.{i}.embedding.weight"]), sd[f"stsgcn.{name}.{i}.activation.weight"]

    w, a = gcn("spatial_temporal_sparse_gcn", 0)
    f1 = prelu(np.einsum("thij,tj->thi", A_s, v)[..., None] * w[:, 0], a)                 # (T, H, N, D)
    w, a = gcn("spatial_temporal_sparse_gcn", 1)
    st = prelu(np.einsum("nhtu,uhnd->nhtd", A_t, f1) @ w.T, a)                            # (N, H, T, D)
    w, a = gcn("temporal_spatial_sparse_gcn", 0)
    f2 = prelu(np.einsum("nhtu,un->nht", A_t, v)[..., None] * w[:, 0], a)                 # (N, H, T, D)
    w, a = gcn("temporal_spatial_sparse_gcn", 1)
    ts = prelu(np.einsum("thij,jhtd->thid", A_s, f2) @ w.T, a).transpose(2, 1, 0, 3)      # (N, H, T, D)
    rep = np.einsum("gh,nhtd->ngtd", _f(sd["fusion_.weight"])[:, :, 0, 0], st) + ts
    x = rep.transpose(0, 2, 1, 3)                                                         # (N, T, H, D)
    x = prelu(conv33(x, sd["tcns.0.0.weight"], sd["tcns.0.0.bias"]), sd["tcns.0.1.weight"])
    for j in range(1, nt):
        x = prelu(conv33(x, sd[f"tcns.{j}.0.weight"], sd[f"tcns.{j}.0.bias"]), sd[f"tcns.{j}.1.weight"]) + x
    out = (x @ _f(sd["output.weight"]).T + _f(sd["output.bias"])).mean(axis=-2)           # (N, pred_len, out_dims)
    return out.transpose(1, 0, 2), logit_s, logit_t


def decisions_fp32(logit):
    """the decision as the network takes it in fp32: sigmoid_fp32(logit) > 0.5, on fp32 logits"""
    l = np.asarray(logit, np.float32)
    one = np.float32(1.0)
    return (one / (one + np.exp(-l, dtype=np.float32))) > np.float32(0.5)


def bridge_identities(T, N):
    """what the sgcn bridge hands over: eye(N) as (1, N, N) and ones as (N, 1, 1) (eye of v.size(3) = 1)"""
    return np.eye(N, dtype=np.float32)[None], np.ones((N, 1, 1), np.float32)


def scene_input(C_obs, nrm, lo, hi):
    """v (k+2, n) of the rows [lo, hi) of a split: [C_obs; last observed position - its mean over the scene]"""
    ori = np.asarray(nrm[:2, lo:hi], np.float32)
    ori = ori - ori.mean(axis=1, keepdims=True, dtype=np.float32)
    return np.concatenate([np.asarray(C_obs[:, lo:hi], np.float32), ori]).astype(np.float32)


# ---------------------------------------------------------------------------------------------- shared test inputs
DELTA = 1e-5            # |logit| below this: the decision is *undecided*
TOL = 1e-5              # outputs: of the largest entry
CAP_SCENE = 5e-3        # undecided entries of one scene
CAP_SPLIT = 1e-4        # ... of a split (or of a set of synthetic scenes)
RAGGED = (1, 2, 3, 17, 63, 64, 65, 130)   # around the wavefront size; 130 is beyond any LDS-resident form
RAGGED_SEED = 3
SPLIT_SIZES = (1, 57, 2, 64, 3, 65, 1)
SPLIT_SEED = 11


def synthetic_split(sizes, seed, k=6):
    """C_obs (k, N), nrm (4, N) of a made-up split: coefficients ~ N(0, 1), last observed positions ~ N(0, 5)"""
    rng = np.random.default_rng(seed)
    n = int(sum(sizes))
    return rng.normal(0, 1, (k, n)).astype(np.float32), rng.normal(0, 5, (4, n)).astype(np.float32)


def synthetic_v(n, seed=RAGGED_SEED):
    C_obs, nrm = synthetic_split([n], seed + 1000 * n)
    return scene_input(C_obs, nrm, 0, n)


def undecided(logit_s, logit_t, band=DELTA):
    """-> (entries with |logit| < band, entries) over both masks"""
    return int((np.abs(logit_s) < band).sum() + (np.abs(logit_t) < band).sum()), logit_s.size + logit_t.size


def check_against(sd, v, identity_s, identity_t, out, logit_s, logit_t, ref_out=None):
    """The three-part comparison of an implementation's (out, logit_s, logit_t) -- fp32, e.g. the device's or the
    reference's recorded ones -- with the restatement, across the hard threshold:
      (a) its logits are within DELTA of the restatement's;
      (b) where |logit64| >= DELTA its decisions, sigmoid_fp32(logit) > 0.5 on ITS logits, equal the restatement's;
      (c) its output equals the restatement run with ITS decisions inside the band, within TOL of the largest entry
    and the band holds at most CAP_SCENE of the scene's entries.  -> dict of the measured figures."""
    dec_s, dec_t = decisions_fp32(logit_s), decisions_fp32(logit_t)
    ref, l64_s, l64_t = forward(sd, v, identity_s, identity_t, decide=(dec_s, dec_t, DELTA))
    fig = {"logit_err": max(float(np.abs(logit_s - l64_s).max()), float(np.abs(logit_t - l64_t).max()))}
    und, total = undecided(l64_s, l64_t)
    fig["undecided"], fig["entries"] = und, total
    own_s, own_t = sigmoid(l64_s) > 0.5, sigmoid(l64_t) > 0.5
    fig["flips_outside_band"] = int(((dec_s != own_s) & (np.abs(l64_s) >= DELTA)).sum() +
                                    ((dec_t != own_t) & (np.abs(l64_t) >= DELTA)).sum())
    fig["flips_inside_band"] = int((dec_s != own_s).sum() + (dec_t != own_t).sum()) - fig["flips_outside_band"]
    fig["out_err"] = float(np.abs(np.asarray(out, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))
    if ref_out is not None:
        fig["ref_err"] = float(np.abs(np.asarray(out, np.float64) - ref_out).max() / max(np.abs(ref_out).max(), 1e-30))
    print(f"sgcn check N={v.shape[1]}: {fig}")
    assert fig["logit_err"] <= DELTA, fig                 # (a)
    assert fig["flips_outside_band"] == 0, fig            # (b)
    assert und <= CAP_SCENE * total, fig                  # the band cannot swallow a scene
    assert fig["out_err"] <= TOL, fig                     # (c)
    return fig
