"""A stock-torch twin of GraphTERNLight's training-mode forward, built from the reference's formulas (baseline/graphtern:
model.py's generate_adjacency_matrix and graph_tern_light.forward, stmrgcn.py's st_mrgcn and epcnn blocks, dropedge.py,
normalizer.py's D (A + I) D) with the DropEdge draw as an explicit keep mask.  It shares the wrapped module's sub-modules, so
its parameters carry the same names and autograd differentiates it; any dtype (``.double()`` on a copy).  The distances
and the ``A == 0`` decision are taken on S_obs in S_obs's own dtype (fp32, as the reference and the kernels decide),
everything after that in the parameters' dtype.  Not a test module itself."""
import torch
import torch.nn as nn


class Twin(nn.Module):
    """``Twin(m)(S_obs, keep=None)`` -> out (1, k, N, S).  In training mode without ``keep`` it draws as the reference does
    (one ``rand((1, 4, T, N, N))``, kept where ``~(rand > 0.8)``), or takes the next mask of ``replay``; every mask used is
    appended to ``log``."""

    def __init__(self, base, percent=0.8, out_dtype=None):
        super().__init__()
        self.out_dtype = out_dtype   # a float64 twin inside an fp32 wrapper hands its output back in fp32
        self.tp_mrgcns, self.tpcnns = base.tp_mrgcns, base.tpcnns
        self.percent = percent
        self.log, self.replay = [], None

    def draw_keep(self, T, n, device):
        return (~(torch.rand((1, 4, T, n, n), device=device) > self.percent))[0].to(torch.uint8)

    def forward(self, S_obs, keep=None):
        dtype = self.tp_mrgcns[0].prelu.weight.dtype
        T, n = S_obs.shape[2], S_obs.shape[3]
        if keep is None and self.training:
            keep = next(self.replay) if self.replay is not None else self.draw_keep(T, n, S_obs.device)
        if keep is not None:
            self.log.append(keep)
        S_obs = S_obs.detach()
        temp = S_obs.unsqueeze(dim=3).repeat_interleave(repeats=n, dim=3)
        A = (temp - temp.transpose(3, 4)).norm(p=2, dim=5)                           # (1, 2, T, N, N), S_obs's dtype
        zero = A == 0
        A = A.to(dtype)
        A_inv = 1.0 / A
        A_inv[zero] = 0
        A = torch.cat([A, A_inv], dim=1)                                              # (1, 4, T, N, N)
        eye = torch.eye(n, dtype=dtype, device=S_obs.device)
        x = S_obs[:, 0].permute(0, 3, 1, 2).contiguous().to(dtype)                   # NTVC -> NCTV
        for blk in self.tp_mrgcns:
            res = x if blk.residual is None else blk.residual(x)
            A_drop = A if keep is None else A * (keep != 0).to(dtype)[None]           # drop_edge: A_drop[rand > percent] = 0
            A_t = A_drop + eye
            d = A_t.sum(-1).unsqueeze(-1).pow(-0.5)
            d = torch.where(torch.isinf(d), torch.zeros_like(d), d)
            L = (d * A_t) * d.transpose(-1, -2)                                       # D (A + I) D
            xc = blk.gcn.conv(x)
            xc = xc.view(xc.size(0), blk.gcn.relation, blk.gcn.out_channels, xc.size(-2), xc.size(-1))
            x = blk.tcn(torch.einsum("nrtwv,nrctv->nctw", L, xc).contiguous()) + res  # use_mdn: blk.prelu is not applied
        x = x.permute(0, 2, 1, 3).contiguous()                                        # NCTV -> NTCV
        for ep in self.tpcnns:
            res = x
            if hasattr(ep, "restconv"):
                res = ep.restconv(res)
            if hasattr(ep, "rescconv"):
                res = ep.rescconv(res.permute(0, 2, 1, 3).contiguous()).permute(0, 2, 1, 3).contiguous()
            x = ep.tpcns[0](x)
            x = ep.cpcns[0](x.permute(0, 2, 1, 3).contiguous())
            x = x.permute(0, 2, 1, 3).contiguous() + res
        out = x.transpose(2, 3).contiguous()                                          # NTCV -> NTVC
        return out if self.out_dtype is None else out.to(self.out_dtype)
