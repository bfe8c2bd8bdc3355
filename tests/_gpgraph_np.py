"""fp64 numpy restatement of GP-Graph-SGCN's eval-mode forward (baseline/gpgraphsgcn: model_groupwrapper.py GPGraph.forward
around model_baseline.py's two-channel SGCN, ET configuration), the arithmetic csrc/et_gpgraph.hip is checked against.  Not
a test module itself; the SGCN pieces are tests/_sgcn_np.py's.

Two kinds of hard decision are taken: ``sigmoid(logit) > 0.5`` on every entry of the interaction masks of the three passes
(as in SGCN), and ``d <= th`` on every pair of pedestrians.  :func:`forward` takes ``decide=(passes, band, close, band_d)``:
where ``|logit| < band`` the keep / drop decision of pass m is read from ``passes[m] = (dec_s, dec_t)``, and where ``|d -
th| <= band_d * th`` the pair decision is read from ``close``; everywhere else they are this module's own."""
import numpy as np

from . import _sgcn_np as SN

SWA = SN.SWA
BAND_D = 1e-5          # |d - th| <= BAND_D * th: the pair is *undecided*
TOL_D = 1e-6           # distances: of the scene's largest distance
CAP_UNDECIDED_SCENES = 0.02
_f = SN._f


def split_state(sd):
    """state dict of the whole GPGraph -> (the base's, with its prefix removed, the rest)"""
    base = {k[len("baseline_model."):]: v for k, v in sd.items() if k.startswith("baseline_model.")}
    return base, {k: v for k, v in sd.items() if not k.startswith("baseline_model.")}


# ------------------------------------------------------------------------------------------------------- the merge
def close_pairs(close):
    """the pairs (r, c), c < r, of a boolean (N, N) matrix in row-major order"""
    r, c = np.nonzero(np.tril(np.asarray(close, bool), -1))
    return list(zip(r.tolist(), c.tolist()))


def merge_literal(close):
    """find_group_indices' loop as written: labels[labels == labels[r]] = c over the close pairs -> raw labels"""
    n = close.shape[0]
    labels = np.arange(n)
    for r, c in close_pairs(close):
        labels[labels == labels[r]] = c
    return labels


def merge_rows(close):
    """the row form: for row r with close columns c1 < .. < cm every node whose label is in {labels[r], c1, .., c(m-1)}
    gets cm -- n serial steps, each parallel over the nodes"""
    n = close.shape[0]
    labels = np.arange(n)
    for r in range(n):
        cols = np.nonzero(close[r, :r])[0]
        if cols.size:
            labels[np.isin(labels, np.concatenate([[labels[r]], cols[:-1]]))] = cols[-1]
    return labels


def merge_union_find(close):
    """connected components (what the loop is NOT): -> the smallest member of each node's component"""
    n = close.shape[0]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for r, c in close_pairs(close):
        a, b = find(r), find(c)
        parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)])


def compact(labels):
    """labels relabelled 0..G-1 in the sorted order of the surviving values"""
    return np.unique(labels, return_inverse=True)[1].reshape(-1)


# ------------------------------------------------------------------------------------------------------ the network
def distances(rest, v_abs):
    """v_abs (T, N) -> d (N, N): mean over t of the L2 norm over the 8 channels of group_cnn(v_abs)[:, t, i] - [:, t, j]"""
    w, b = _f(rest["group_gen.group_cnn.0.weight"])[:, 0, :, 0], _f(rest["group_gen.group_cnn.0.bias"])
    x = np.pad(_f(v_abs), ((1, 1), (0, 0)))
    T = v_abs.shape[0]
    f = b[:, None, None] + sum(w[:, d, None, None] * x[None, d:d + T] for d in range(3))   # (8, T, N)
    return np.sqrt(((f[:, :, :, None] - f[:, :, None, :]) ** 2).sum(axis=0)).mean(axis=0)


def threshold(rest):
    return float(np.asarray(rest["group_gen.th"], np.float32).reshape(-1)[0])


def attention_t(sd, x):
    """the temporal SelfAttention(multi_head=True) on x (N, T, 2) -> (N, H, T, T)"""
    p = SWA + "temporal_attention."
    e = x @ _f(sd[p + "embedding.weight"]).T + _f(sd[p + "embedding.bias"])
    q = e @ _f(sd[p + "query.weight"]).T + _f(sd[p + "query.bias"])
    k = e @ _f(sd[p + "key.weight"]).T + _f(sd[p + "key.bias"])
    B, L = x.shape[:2]
    q = q.reshape(B, L, SN.H, SN.D).transpose(0, 2, 1, 3)
    k = k.reshape(B, L, SN.H, SN.D).transpose(0, 2, 1, 3)
    a = q @ k.transpose(0, 1, 3, 2) / 8.0
    a = np.exp(a - a.max(axis=-1, keepdims=True))
    return a / a.sum(axis=-1, keepdims=True)


def base_forward(sd, g, same=None, decide=None):
    """model_baseline.py's TrajectoryModel.forward: g (2, T, N) = [position; coefficients], identities eye(N) and eye(T),
    ``same`` the (N, N) same-group matrix or None -> (out (S, k, N), logit_s (T, H, N, N), logit_t (N, H, T, T))"""
    g = _f(g)
    v = g[1]
    T, N = v.shape
    na, nt = SN.n_layers(sd)
    dec_s, dec_t, band = decide if decide is not None else (None, None, 0.0)
    dense_s = SN.attention(sd, "spatial_attention", v)
    dense_t = attention_t(sd, g.transpose(2, 1, 0))
    fw = _f(sd[SWA + "spa_fusion.conv.0.weight"])[:, :, 0, 0]
    fb = _f(sd[SWA + "spa_fusion.conv.0.bias"])
    xs = SN.prelu(np.einsum("ut,thij->uhij", fw, dense_s) + fb[:, None, None, None], sd[SWA + "spa_fusion.conv.1.weight"])
    xs = xs + dense_s
    xt = dense_t
    for j in range(na):
        xs = SN.asymmetric(sd, f"{SWA}interaction_mask.spatial_asymmetric_convolutions.{j}.", xs)
        xt = SN.asymmetric(sd, f"{SWA}interaction_mask.temporal_asymmetric_convolutions.{j}.", xt)
    logit_s, logit_t = xs, xt
    mask_s = SN._mask(logit_s, dec_s, band, np.eye(N)[None])
    if same is not None:
        mask_s = mask_s * _f(same)[None, None]
    A_s = SN.zero_softmax(dense_s * mask_s)
    A_t = SN.zero_softmax(dense_t * SN._mask(logit_t, dec_t, band, np.broadcast_to(np.eye(T), (N, T, T))))

    def gcn(name, i):
        return _f(sd[f"stsgcn.{name}.{i}.embedding.weight"]), sd[f"stsgcn.{name}.{i}.activation.weight"]

    w, a = gcn("spatial_temporal_sparse_gcn", 0)
    f1 = SN.prelu(np.einsum("thij,tj->thi", A_s, v)[..., None] * w[:, 0], a)
    w, a = gcn("spatial_temporal_sparse_gcn", 1)
    st = SN.prelu(np.einsum("nhtu,uhnd->nhtd", A_t, f1) @ w.T, a)
    w, a = gcn("temporal_spatial_sparse_gcn", 0)
    f2 = SN.prelu(np.einsum("nhtu,un->nht", A_t, v)[..., None] * w[:, 0], a)
    w, a = gcn("temporal_spatial_sparse_gcn", 1)
    ts = SN.prelu(np.einsum("thij,jhtd->thid", A_s, f2) @ w.T, a).transpose(2, 1, 0, 3)
    rep = np.einsum("gh,nhtd->ngtd", _f(sd["fusion_.weight"])[:, :, 0, 0], st) + ts
    x = rep.transpose(0, 2, 1, 3)
    x = SN.prelu(SN.conv33(x, sd["tcns.0.0.weight"], sd["tcns.0.0.bias"]), sd["tcns.0.1.weight"])
    for j in range(1, nt):
        x = SN.prelu(SN.conv33(x, sd[f"tcns.{j}.0.weight"], sd[f"tcns.{j}.0.bias"]), sd[f"tcns.{j}.1.weight"]) + x
    out = (x @ _f(sd["output.weight"]).T + _f(sd["output.bias"])).mean(axis=-2)            # (N, k, S)
    return out.transpose(2, 1, 0), logit_s, logit_t


def forward(sd, v_abs, v_rel, decide=None, tau=0.1):
    """v_abs (T, N), v_rel (2, T, N) -> dict: out (S, k, N), indices (N,), dist (N, N), n_groups, passes [(out_m (S, k, n_m),
    logit_s, logit_t)] * 3 (pass 1 on the G group means, before the unpooling)"""
    base, rest = split_state(sd)
    v_abs, v_rel = _f(v_abs), _f(v_rel)
    passes, band, given, band_d = decide if decide is not None else (None, 0.0, None, 0.0)
    d = distances(rest, v_abs)
    th = threshold(rest)
    close = d <= th
    if given is not None:
        close = np.where(np.abs(d - th) <= band_d * th, np.asarray(given, bool), close)
    indices = compact(merge_literal(close))
    G = int(indices.max()) + 1
    sig = SN.sigmoid(-(d - th) / tau)
    v_soft = v_rel @ (sig / sig.sum(axis=0, keepdims=True))
    v2 = (v_rel - v_soft) + v_soft
    onehot = (indices[:, None] == np.arange(G)[None]).astype(np.float64)                    # (N, G)
    pooled = (v2 @ onehot) / onehot.sum(axis=0)
    same = indices[:, None] == indices[None, :]

    def dec(m):
        return None if passes is None else (passes[m][0], passes[m][1], band)

    res = [base_forward(base, v_rel, None, dec(0)), base_forward(base, pooled, None, dec(1)),
           base_forward(base, v2, same, dec(2))]
    stack = [res[0][0], res[1][0][:, :, indices], res[2][0]]
    S, k, N = stack[0].shape
    x = np.concatenate(stack, axis=0).reshape(3 * S * k, N)
    w = _f(rest["group_mix.st_gcns_mix.1.weight"])[:, :, 0, 0]
    y = w @ SN.prelu(x, rest["group_mix.st_gcns_mix.0.weight"]) + _f(rest["group_mix.st_gcns_mix.1.bias"])[:, None]
    out = (stack[0] + stack[1] + stack[2]) / 3.0 + y.reshape(S, k, N)
    return {"out": out, "indices": indices, "dist": d, "n_groups": G, "passes": res, "close": close}


def bridge_input(v):
    """v (T, N) = [C_obs; obs_ori] -> (v_abs (T, N), v_rel (2, T, N)) as gpgraphsgcn/bridge.py builds them (fp32)"""
    v = np.asarray(v, np.float32)
    pos = np.broadcast_to(np.arange(1, v.shape[0] + 1, dtype=np.float32)[:, None], v.shape)
    return v, np.stack([pos, v]).astype(np.float32)


def pair_margin(d, th):
    """min |d - th| / th over the pairs c < r (inf without a pair)"""
    n = d.shape[0]
    low = np.tril(np.ones((n, n), bool), -1)
    return float(np.abs(d[low] - th).min() / th) if low.any() else float("inf")


def check_against(sd, v_abs, v_rel, got, ref_out=None):
    """The comparison of an implementation's results -- fp32: ``got`` = dict(out (S, k, N), indices, dist, logit_s [3],
    logit_t [3]), the device's or the reference's recorded ones -- with the restatement:
      dist within TOL_D of the largest distance; no undecided pair -> the indices are equal; then per pass SN.check_against's
      parts (a) and (b) on the logits, the caps over the three passes together, and the output within SN.TOL of the largest
      entry against the restatement run with ITS decisions inside the bands.
    A scene with an undecided pair whose indices differ is left out of the output comparison (fig["compared"] False)."""
    base, rest = split_state(sd)
    th = threshold(rest)
    d64 = distances(rest, v_abs)
    n = d64.shape[0]
    fig = {"n": n, "dist_err": float(np.abs(np.asarray(got["dist"], np.float64) - d64).max() / max(d64.max(), 1e-30)),
           "margin": pair_margin(d64, th)}
    assert fig["dist_err"] <= TOL_D, fig
    fig["pair_undecided"] = bool(fig["margin"] <= BAND_D)
    close = np.asarray(got["dist"], np.float32) <= np.float32(th)
    own = forward(sd, v_abs, v_rel)
    same_idx = np.array_equal(own["indices"], np.asarray(got["indices"]))
    if not fig["pair_undecided"]:
        assert same_idx, (fig, own["indices"], got["indices"])
    decs = [(SN.decisions_fp32(got["logit_s"][m]), SN.decisions_fp32(got["logit_t"][m])) for m in range(3)]
    ref = forward(sd, v_abs, v_rel, decide=(decs, SN.DELTA, close, BAND_D))
    fig["compared"] = bool(np.array_equal(ref["indices"], np.asarray(got["indices"])))
    if not fig["compared"]:
        assert fig["pair_undecided"], fig
        print(f"gpgraph check N={n}: {fig}")
        return fig
    und = total = flips = 0
    logit_err = 0.0
    for m in range(3):
        _, l64_s, l64_t = ref["passes"][m]
        ls, lt = np.asarray(got["logit_s"][m]), np.asarray(got["logit_t"][m])
        assert ls.shape == l64_s.shape and lt.shape == l64_t.shape, (m, ls.shape, l64_s.shape)
        logit_err = max(logit_err, float(np.abs(ls - l64_s).max()), float(np.abs(lt - l64_t).max()))
        u, t = SN.undecided(l64_s, l64_t)
        und, total = und + u, total + t
        flips += int(((decs[m][0] != (SN.sigmoid(l64_s) > 0.5)) & (np.abs(l64_s) >= SN.DELTA)).sum() +
                     ((decs[m][1] != (SN.sigmoid(l64_t) > 0.5)) & (np.abs(l64_t) >= SN.DELTA)).sum())
    fig.update(logit_err=logit_err, undecided=und, entries=total, flips_outside_band=flips, n_groups=ref["n_groups"])
    fig["out_err"] = float(np.abs(np.asarray(got["out"], np.float64) - ref["out"]).max() / max(np.abs(ref["out"]).max(), 1e-30))
    if ref_out is not None:
        fig["ref_err"] = float(np.abs(np.asarray(got["out"], np.float64) - ref_out).max() / max(np.abs(ref_out).max(), 1e-30))
    print(f"gpgraph check N={n}: {fig}")
    assert fig["logit_err"] <= SN.DELTA, fig
    assert fig["flips_outside_band"] == 0, fig
    assert und <= SN.CAP_SCENE * total, fig
    assert fig["out_err"] <= SN.TOL, fig
    return fig
