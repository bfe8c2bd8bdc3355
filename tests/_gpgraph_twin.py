"""GP-Graph-SGCN's forward (ET configuration, dropout = 0) in stock torch operators, differentiable by autograd: our own
restatement of what csrc/et_gpgraph.hip computes (tests/_gpgraph_np.py is the numpy form), with the attentions un-collapsed,
the learned distance through ``norm`` (whose backward is 0 at 0), the straight-through soft assignment written with
``detach`` and the pooling with ``index_add``.  Used by tests/test_gpgraph_train_cpu.py as the autograd reference of
tests/_gpgraph_train_np.py and by tools/time_train.py --predictor gpgraph_sgcn as the stock-torch network.  Not a test module itself."""
import numpy as np
import torch
import torch.nn.functional as F

from . import _gpgraph_np as GN
from . import _sgcn_twin as TW

H, D, SWA = TW.H, TW.D, TW.SWA
BASE = "baseline_model."


def parameters(sd, dtype=torch.float64, device="cpu"):
    return TW.parameters(sd, dtype, device)


def _attention_t(P, x):
    """the temporal attention on x (N, T, 2) = [position, coefficient] -> (N, H, T, T)"""
    p = SWA + "temporal_attention."
    e = F.linear(x, P[p + "embedding.weight"], P[p + "embedding.bias"])
    q = F.linear(e, P[p + "query.weight"], P[p + "query.bias"])
    k = F.linear(e, P[p + "key.weight"], P[p + "key.bias"])
    B, L = x.shape[:2]
    q = q.view(B, L, H, D).permute(0, 2, 1, 3)
    k = k.view(B, L, H, D).permute(0, 2, 1, 3)
    return torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)


def base_forward(P, g, same=None, decisions=None):
    """the two-channel SGCN: P the base's parameters (no prefix), g (2, T, N) = [position; coefficients] (may require grad),
    identities eye(N) and eye(T), ``same`` the (N, N) same-group matrix or None -> (S, k, N)"""
    v = g[1]
    T_, N = v.shape
    dt, dev = v.dtype, v.device
    na = len({k.split(".")[3] for k in P if k.startswith(SWA + "interaction_mask.spatial_asymmetric_convolutions.")})
    nt = len({k.split(".")[1] for k in P if k.startswith("tcns.")})
    dense_s = TW._attention(P, "spatial_attention", v)                       # (T, H, N, N)
    dense_t = _attention_t(P, g.permute(2, 1, 0))                            # (N, H, T, T)
    x = dense_s.permute(1, 0, 2, 3)
    xs = (F.prelu(F.conv2d(x, P[SWA + "spa_fusion.conv.0.weight"], P[SWA + "spa_fusion.conv.0.bias"]),
                  P[SWA + "spa_fusion.conv.1.weight"]) + x).permute(1, 0, 2, 3)
    xt = dense_t
    for j in range(na):
        xs = TW._asym(P, f"{SWA}interaction_mask.spatial_asymmetric_convolutions.{j}.", xs)
        xt = TW._asym(P, f"{SWA}interaction_mask.temporal_asymmetric_convolutions.{j}.", xt)
    dec_s, dec_t = decisions if decisions is not None else (None, None)
    mask_s = TW._mask(xs, torch.eye(N, dtype=dt, device=dev)[None, None], dec_s)
    if same is not None:
        mask_s = mask_s * same.to(dt)[None, None]
    A_s = TW._zero_softmax(dense_s * mask_s)
    A_t = TW._zero_softmax(dense_t * TW._mask(xt, torch.eye(T_, dtype=dt, device=dev)[None, None], dec_t))

    def gcn(name, i, x):
        return F.prelu(F.linear(x, P[f"stsgcn.{name}.{i}.embedding.weight"]), P[f"stsgcn.{name}.{i}.activation.weight"])

    f1 = gcn("spatial_temporal_sparse_gcn", 0, torch.einsum("thij,tj->thi", A_s, v)[..., None])
    st = gcn("spatial_temporal_sparse_gcn", 1, torch.einsum("nhtu,uhnd->nhtd", A_t, f1))
    f2 = gcn("temporal_spatial_sparse_gcn", 0, torch.einsum("nhtu,un->nht", A_t, v)[..., None])
    ts = gcn("temporal_spatial_sparse_gcn", 1, torch.einsum("thij,jhtd->thid", A_s, f2)).permute(2, 1, 0, 3)
    rep = F.conv2d(st, P["fusion_.weight"]) + ts
    x = rep.permute(0, 2, 1, 3)
    x = F.prelu(F.conv2d(x, P["tcns.0.0.weight"], P["tcns.0.0.bias"], padding=1), P["tcns.0.1.weight"])
    for j in range(1, nt):
        x = F.prelu(F.conv2d(x, P[f"tcns.{j}.0.weight"], P[f"tcns.{j}.0.bias"], padding=1), P[f"tcns.{j}.1.weight"]) + x
    out = F.linear(x, P["output.weight"], P["output.bias"]).mean(dim=-2)     # (N, k, S)
    return out.permute(2, 1, 0)


def forward(P, v_abs, v_rel, tau=0.1, decisions=None, close=None):
    """P of :func:`parameters` (the whole GPGraph's names), v_abs (T, N), v_rel (2, T, N) -> (out (S, k, N), indices (N,)
    numpy, dist (N, N)).  ``decisions`` [3] x (dec_s, dec_t): the masks' keep / drop decisions of the three passes, given;
    ``close`` (N, N) bool: the pair decisions d <= th, given."""
    ref = P["group_mix.st_gcns_mix.1.weight"]
    dt, dev = ref.dtype, ref.device
    v_abs = torch.as_tensor(v_abs).to(device=dev, dtype=dt)
    v_rel = torch.as_tensor(v_rel).to(device=dev, dtype=dt)
    base = {k[len(BASE):]: p for k, p in P.items() if k.startswith(BASE)}
    f = F.conv2d(v_abs[None, None], P["group_gen.group_cnn.0.weight"], P["group_gen.group_cnn.0.bias"], padding=(1, 0))[0]
    d = (f[:, :, :, None] - f[:, :, None, :]).norm(p=2, dim=0).mean(dim=0)                   # (N, N)
    th = P["group_gen.th"]
    if close is None:
        close = (d <= th).detach().cpu().numpy()
    indices = GN.compact(GN.merge_literal(np.asarray(close, bool)))
    idx = torch.as_tensor(indices, device=dev)
    G = int(indices.max()) + 1
    sig = torch.sigmoid(-(d - th) / tau)
    v_soft = v_rel @ (sig / sig.sum(dim=0, keepdim=True))
    v2 = (v_rel - v_soft).detach() + v_soft
    pooled = torch.zeros(v2.shape[:-1] + (G,), dtype=dt, device=dev).index_add(-1, idx, v2)
    pooled = pooled / torch.zeros((G,), dtype=dt, device=dev).index_add(0, idx, torch.ones_like(idx, dtype=dt))
    same = idx[:, None] == idx[None, :]
    dec = decisions if decisions is not None else (None, None, None)
    stack = [base_forward(base, v_rel, None, dec[0]), base_forward(base, pooled, None, dec[1])[:, :, idx],
             base_forward(base, v2, same, dec[2])]
    S, k, N = stack[0].shape
    x = torch.cat(stack, dim=0).reshape(1, 3 * S * k, 1, N)
    y = F.conv2d(F.prelu(x, P["group_mix.st_gcns_mix.0.weight"]), P["group_mix.st_gcns_mix.1.weight"],
                 P["group_mix.st_gcns_mix.1.bias"]).view(S, k, N)
    return (stack[0] + stack[1] + stack[2]) / 3.0 + y, indices, d


def gradients(sd, v_abs, v_rel, d_out, dtype=torch.float64, device="cpu", **kw):
    """-> (out (S, k, N), indices, {name: gradient of sum(out * d_out)}) as numpy; d_out (S, k, N)"""
    P = parameters(sd, dtype, device)
    out, indices, _ = forward(P, v_abs, v_rel, **kw)
    out.backward(torch.as_tensor(d_out).to(device=out.device, dtype=dtype))
    return out.detach().cpu().numpy(), indices, {k: (p.grad if p.grad is not None else torch.zeros_like(p)).cpu().numpy()
                                                 for k, p in P.items()}


class Twin(torch.nn.Module):
    """``forward(v_abs, v_rel)`` of an :class:`eigentrajectory_amd.gpgraph.GPGraph` in the stock operators above, on that
    module's own parameters (``net``), under torch autograd: what tools/time_train.py --predictor gpgraph_sgcn times the native path
    against"""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, v_abs, v_rel):
        out, indices, _ = forward(dict(self.net.named_parameters()), v_abs[0, 0], v_rel[0], tau=self.net.TAU)
        return out[None], torch.as_tensor(indices, device=out.device)
