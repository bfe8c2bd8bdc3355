"""A stock-torch twin of SocialDMRGCN's training-mode forward, built from the reference's formulas (baseline/dmrgcn:
dmrgcn.py's clipped bins and st_dmrgcn block, dropedge.py, normalizer.py's D (A + I) D, predictor.py's tpcnn) with the
DropEdge draw as an explicit keep mask.  It shares the wrapped module's sub-modules, so its parameters carry the same
names and autograd differentiates it; any dtype (``.double()`` on a copy).  The bins are decided on ``a`` in ``a``'s own
dtype (fp32 distances, as the reference and the kernels decide), everything after that in the parameters' dtype.
Not a test module itself."""
import torch
import torch.nn as nn

LAST = 1e10


class Twin(nn.Module):
    """``Twin(m)(v, a, keep=None)`` -> (out (1, S, k, N), a).  In training mode without ``keep`` it draws as the reference
    does (one ``rand_like(A_)`` per relation, kept where ``~(rand > 0.8)``), or takes the next mask of ``replay``; every mask
    used is appended to ``log``."""

    def __init__(self, base, percent=0.8, out_dtype=None):
        super().__init__()
        self.out_dtype = out_dtype   # a float64 twin inside an fp32 wrapper hands its output back in fp32
        self.st_dmrgcns, self.tpcnns = base.st_dmrgcns, base.tpcnns
        self.split, self.percent = [list(s) for s in base.split], percent
        self.log, self.replay = [], None

    def draw_keep(self, K, n, device):
        return torch.cat([~(torch.rand((1, 5, K, n, n), device=device) > self.percent) for _ in range(2)]).to(torch.uint8)

    def forward(self, v, a, keep=None):
        dtype = self.st_dmrgcns[0].prelu.weight.dtype
        n, K = v.shape[-1], v.shape[-2]
        if keep is None and self.training:
            keep = next(self.replay) if self.replay is not None else self.draw_keep(K, n, v.device)
        if keep is not None:
            self.log.append(keep)
        x = v.to(dtype)
        eye = torch.eye(n, dtype=dtype, device=v.device)
        for blk in self.st_dmrgcns:
            res = x if blk.residual is None else blk.residual(x)
            x_r = None
            for r, g in enumerate(blk.gcns):
                A = a[:, r]                                                            # (1, K, N, N), a's own dtype
                edges = [torch.tensor(e, dtype=A.dtype) for e in self.split[r] + [LAST]]
                A_ = torch.stack([((A > edges[b]) & (A < edges[b + 1])) for b in range(len(self.split[r]))], dim=1).to(dtype)
                if keep is not None:                                                   # drop_edge: A_drop[rand > percent] = 0
                    A_ = A_ * (keep[r] != 0).to(dtype)[None]
                A_t = A_ + eye
                d = A_t.sum(-1).unsqueeze(-1).pow(-0.5)                                # (1, 5, K, N, 1)
                L = eye - (d * A_t) * d.transpose(-1, -2)                              # I - D (A + I) D
                xc = g.conv(x)
                xc = xc.view(xc.size(0), g.relation, g.out_channels, xc.size(-2), xc.size(-1))
                x_a = torch.einsum("nrtwv,nrctv->nctw", L, xc)
                x_r = x_a if x_r is None else x_r + x_a
            x = blk.prelu(blk.tcn(x_r) + res)
        x = x.permute(0, 2, 1, 3)
        for tp in self.tpcnns:
            res = x if tp.residual is None else tp.residual(x)
            x = tp.tpcn[0](x) + res
            x = tp.tpcn[1](x) + x
            x = x.permute(0, 2, 1, 3).contiguous()
            x = tp.gtacn[0](x) + x
            x = x.permute(0, 2, 1, 3)
        out = x.permute(0, 2, 1, 3)
        return (out if self.out_dtype is None else out.to(self.out_dtype)), a
