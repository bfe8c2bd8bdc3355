"""A stock-torch twin of eigentrajectory_amd.implicit.SocialImplicitLight under autograd: the same parameters (it reads them
from the module it is given, or from any mapping of state_dict keys to tensors), per-zone compaction with boolean gathers,
``conv2d`` / ``conv1d``, and the local stream's raw reshape.  What the native training path is cross-checked and timed
against; nothing native runs here, so it works on the CPU and in float64."""
import torch
import torch.nn.functional as F


def cell(p, xs):
    """p: name -> tensor of one cell (``feat.weight`` ... ``ped.tpcnn.bias``, ``global_w``, ``local_w``), xs (T, n) the
    zone's pedestrians compacted -> (S, T_out, n)"""
    a = xs[None, None]                                                              # (1, 1, T, n)
    u = F.relu(F.conv2d(a, p["feat.weight"], p["feat.bias"], padding=1)) \
        + F.conv2d(a, p["highway_input.weight"], p["highway_input.bias"])           # (1, S, T, n)
    ut = u.permute(0, 2, 1, 3)                                                      # T as channels
    g = F.conv2d(ut, p["tpcnn.weight"], p["tpcnn.bias"], padding=1) + F.conv2d(ut, p["highway.weight"], p["highway.bias"])
    b = xs.t()[:, None, :]                                                          # (n, 1, T)
    ul = F.relu(F.conv1d(b, p["ped.feat.weight"], p["ped.feat.bias"], padding=1)) \
        + F.conv1d(b, p["ped.highway_input.weight"], p["ped.highway_input.bias"])   # (n, S, T)
    ult = ul.permute(0, 2, 1)
    l = F.conv1d(ult, p["ped.tpcnn.weight"], p["ped.tpcnn.bias"], padding=1) \
        + F.conv1d(ult, p["ped.highway.weight"], p["ped.highway.bias"])             # (n, T_out, S)
    n, To, S = l.shape
    return p["global_w"] * g[0].permute(1, 0, 2) + p["local_w"] * l.reshape(n, S, To).permute(1, 2, 0)


def forward(params, v, bins):
    """params: state_dict key -> tensor (``implicit_cells.{i}....``), v (1, 1, T, N), bins a list -> (1, S, T_out, N).
    Every zone costs one ``bool(any)`` host synchronisation, as in the network this mirrors."""
    x = v[0, 0]
    edges = torch.tensor([float(b) for b in bins], dtype=torch.float32, device=x.device).to(x.dtype)  # fp32 bounds
    zone = torch.bucketize(x[0].abs(), edges, right=True) - 1
    first = params["implicit_cells.0.tpcnn.weight"]
    S, To = params["implicit_cells.0.feat.weight"].shape[0], first.shape[0]
    out = torch.zeros((S, To, x.shape[1]), dtype=first.dtype, device=x.device)
    for i in range(len(bins)):
        sel = zone == i
        if bool(sel.any()):
            pre = f"implicit_cells.{i}."
            p = {k[len(pre):]: t for k, t in params.items() if k.startswith(pre)}
            out[:, :, sel] = cell(p, x[:, sel].to(first.dtype))
    return out[None]


class Twin(torch.nn.Module):
    """the twin as a module over the parameters of ``net`` (shared, not copied): plugs into EigenTrajectory under the
    ``implicit`` hooks like the native module"""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, v):
        return forward(dict(self.net.named_parameters()), v, self.net.bins)
