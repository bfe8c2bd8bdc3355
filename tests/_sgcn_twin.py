"""SGCN's forward (in_dims = 1, dropout = 0) in stock torch operators, differentiable by autograd: our own restatement of
what csrc/et_sgcn.hip computes (tests/_sgcn_np.py is the numpy form), with the attention un-collapsed (embedding, query, key
as three linear layers).  Used by tests/test_sgcn_train_cpu.py as the autograd reference of tests/_sgcn_train_np.py and by
tools/time_train.py --predictor sgcn as the stock-torch network.  Not a test module itself."""
import torch
import torch.nn.functional as F

H, D = 4, 16
SWA = "sparse_weighted_adjacency_matrices."


def parameters(sd, dtype=torch.float64, device="cpu"):
    """state dict (numpy or tensors) -> {name: leaf tensor that requires grad}"""
    return {k: torch.as_tensor(v).detach().to(device=device, dtype=dtype).clone().requires_grad_(True) for k, v in sd.items()}


def _attention(P, name, x):
    p = SWA + name + "."
    e = F.linear(x[..., None], P[p + "embedding.weight"], P[p + "embedding.bias"])       # (B, L, 64)
    q = F.linear(e, P[p + "query.weight"], P[p + "query.bias"])
    k = F.linear(e, P[p + "key.weight"], P[p + "key.bias"])
    B, L = x.shape
    q = q.view(B, L, H, D).permute(0, 2, 1, 3)
    k = k.view(B, L, H, D).permute(0, 2, 1, 3)
    return torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)


def _asym(P, p, x):
    y = F.conv2d(x, P[p + "conv2.weight"], P[p + "conv2.bias"], padding=(0, 1)) + F.conv2d(x, P[p + "conv1.weight"], None,
                                                                                            padding=(1, 0))
    return F.prelu(y, P[p + "activation.weight"]) + x


def _zero_softmax(x):
    e = (torch.exp(x) - 1.0) ** 2
    return e / (e.sum(dim=-1, keepdim=True) + 1e-5)


def _mask(logit, identity, dec=None):
    sg = torch.sigmoid(logit)
    keep = sg > 0.5 if dec is None else torch.as_tensor(dec, device=logit.device)
    return torch.where(keep, sg, torch.zeros_like(sg)) + identity


def forward(P, v, identity_s, identity_t, decisions=None):
    """P of :func:`parameters`, v (T, N), identity_s (1 or T, N, N), identity_t (N, 1 or T, 1 or T) -> out (pred_len, N,
    out_dims).  ``decisions`` (dec_s (T, H, N, N), dec_t (N, H, T, T)): the masks' keep / drop decisions, given."""
    dt, dev = P["fusion_.weight"].dtype, P["fusion_.weight"].device
    v = torch.as_tensor(v).to(device=dev, dtype=dt)
    ids = torch.as_tensor(identity_s).to(device=dev, dtype=dt)[:, None]
    idt = torch.as_tensor(identity_t).to(device=dev, dtype=dt)[:, None]
    na = len({k.split(".")[3] for k in P if k.startswith(SWA + "interaction_mask.spatial_asymmetric_convolutions.")})
    nt = len({k.split(".")[1] for k in P if k.startswith("tcns.")})
    dense_s = _attention(P, "spatial_attention", v)        # (T, H, N, N)
    dense_t = _attention(P, "temporal_attention", v.T)     # (N, H, T, T)
    x = dense_s.permute(1, 0, 2, 3)                        # (H, T, N, N): spa_fusion mixes T
    xs = (F.prelu(F.conv2d(x, P[SWA + "spa_fusion.conv.0.weight"], P[SWA + "spa_fusion.conv.0.bias"]),
                  P[SWA + "spa_fusion.conv.1.weight"]) + x).permute(1, 0, 2, 3)
    xt = dense_t
    for j in range(na):
        xs = _asym(P, f"{SWA}interaction_mask.spatial_asymmetric_convolutions.{j}.", xs)
        xt = _asym(P, f"{SWA}interaction_mask.temporal_asymmetric_convolutions.{j}.", xt)
    dec_s, dec_t = decisions if decisions is not None else (None, None)
    A_s = _zero_softmax(dense_s * _mask(xs, ids, dec_s))
    A_t = _zero_softmax(dense_t * _mask(xt, idt, dec_t))

    def gcn(name, i, x):
        return F.prelu(F.linear(x, P[f"stsgcn.{name}.{i}.embedding.weight"]), P[f"stsgcn.{name}.{i}.activation.weight"])

    f1 = gcn("spatial_temporal_sparse_gcn", 0, torch.einsum("thij,tj->thi", A_s, v)[..., None])     # (T, H, N, D)
    st = gcn("spatial_temporal_sparse_gcn", 1, torch.einsum("nhtu,uhnd->nhtd", A_t, f1))            # (N, H, T, D)
    f2 = gcn("temporal_spatial_sparse_gcn", 0, torch.einsum("nhtu,un->nht", A_t, v)[..., None])     # (N, H, T, D)
    ts = gcn("temporal_spatial_sparse_gcn", 1, torch.einsum("thij,jhtd->thid", A_s, f2)).permute(2, 1, 0, 3)
    rep = F.conv2d(st, P["fusion_.weight"]) + ts
    x = rep.permute(0, 2, 1, 3)                                                                     # (N, T, H, D)
    x = F.prelu(F.conv2d(x, P["tcns.0.0.weight"], P["tcns.0.0.bias"], padding=1), P["tcns.0.1.weight"])
    for j in range(1, nt):
        x = F.prelu(F.conv2d(x, P[f"tcns.{j}.0.weight"], P[f"tcns.{j}.0.bias"], padding=1), P[f"tcns.{j}.1.weight"]) + x
    out = F.linear(x, P["output.weight"], P["output.bias"]).mean(dim=-2)                            # (N, pred_len, S)
    return out.permute(1, 0, 2)


def gradients(sd, v, identity_s, identity_t, d_out, dtype=torch.float64, decisions=None, device="cpu"):
    """-> (out, {name: gradient of sum(out * d_out)}) as numpy"""
    P = parameters(sd, dtype, device)
    out = forward(P, v, identity_s, identity_t, decisions)
    out.backward(torch.as_tensor(d_out).to(device=out.device, dtype=dtype))
    return out.detach().cpu().numpy(), {k: (p.grad if p.grad is not None else torch.zeros_like(p)).cpu().numpy()
                                        for k, p in P.items()}


class Twin(torch.nn.Module):
    """``forward(graph, identity)`` of an :class:`eigentrajectory_amd.sgcn.SGCN` in the stock operators above, on that
    module's own parameters (``net``), under torch autograd: what tools/time_train.py --predictor sgcn times the native path against"""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, graph, identity, mask=None):
        P = dict(self.net.named_parameters())
        return forward(P, graph[0, :, :, 0], identity[0], identity[1])
