"""numpy restatement of csrc/et_implicit.hip: SocialImplicitLight's eval-mode forward (baseline/implicit/model.py:9-88,
126-159) and the implicit bridge's post-hook, in fp64 from a state_dict of numpy arrays.

The Social-Zone of a pedestrian is decided ON THE fp32 NUMBERS (|first coefficient| against the fp32 bin values, as
torch.bucketize(right=True) decides it); everything after the decision is fp64.  Each zone's cell runs on the zone's
pedestrians compacted in scene order, as the reference's ``v[..., select]`` hands them over, with plain zero-padded
convolutions written as shifted einsum sums -- no per-pedestrian neighbour table, which is the kernel's own device."""
import numpy as np

BINS = (0.0, 0.01, 0.1, 1.2)  # utils/trainer.py:555


def zones(u, bins=BINS):
    """u (T, N) fp32 -> (N,) int32: the bins that are not greater than |u[0]|, minus one (bucketize(right=True) - 1; a NaN
    is greater than no bin, so it lands in the last zone); -1 below bins[0]"""
    first = np.abs(np.asarray(u, np.float32)[0])
    b = np.asarray(bins, np.float32)
    with np.errstate(invalid="ignore"):
        return (~(b[:, None] > first[None, :])).sum(axis=0).astype(np.int32) - 1


def _relu(x):
    return np.where(x < 0, 0.0, x)  # a NaN stays a NaN


def _conv33(x, w, b):
    """x (Cin, H, W), w (Cout, Cin, 3, 3), b (Cout,): zero-padded 'same' convolution"""
    cin, h, wd = x.shape
    xp = np.zeros((cin, h + 2, wd + 2))
    xp[:, 1:-1, 1:-1] = x
    out = np.zeros((w.shape[0], h, wd)) + b[:, None, None]
    for dh in range(3):
        for dw in range(3):
            out += np.einsum("oi,ihw->ohw", w[:, :, dh, dw], xp[:, dh:dh + h, dw:dw + wd])
    return out


def _conv3(x, w, b):
    """x (Cin, L, n) a batch of n rows, w (Cout, Cin, 3), b (Cout,): zero-padded 1-d convolution over L"""
    cin, ln, n = x.shape
    xp = np.zeros((cin, ln + 2, n))
    xp[:, 1:-1] = x
    return b[:, None, None] + sum(np.einsum("oi,iln->oln", w[:, :, d], xp[:, d:d + ln]) for d in range(3))


def cell(sd, pre, x, transpose=False):
    """One zone's SocialCellGlobal on its compacted pedestrians: x (T, n) fp64 -> (S, T_out, n).  ``transpose``: the local
    stream's (T_out, S) block transposed to (S, T_out) -- NOT what the reference does (it reshapes), kept to show that the
    fixtures tell the two apart."""
    g = lambda name: sd[pre + name]
    T, n = x.shape
    # global stream, spatial section: one input channel, S output channels over the (T, n) plane
    u = _relu(_conv33(x[None], g("feat.weight"), g("feat.bias"))) \
        + g("highway_input.weight")[:, 0, 0, 0][:, None, None] * x[None] + g("highway_input.bias")[:, None, None]
    # temporal section: T becomes the channels, the plane is (S, n); the zero padding pads u
    ut = np.transpose(u, (1, 0, 2))
    glob = _conv33(ut, g("tpcnn.weight"), g("tpcnn.bias")) \
        + np.einsum("ot,tsn->osn", g("highway.weight")[:, :, 0, 0], ut) + g("highway.bias")[:, None, None]
    glob = np.transpose(glob, (1, 0, 2))                                    # (S, T_out, n)
    # local stream: every pedestrian on its own, 1-d convolutions over T, then over S with T as channels
    ul = _relu(_conv3(x[None], g("ped.feat.weight"), g("ped.feat.bias"))) \
        + g("ped.highway_input.weight")[:, 0, 0][:, None, None] * x[None] + g("ped.highway_input.bias")[:, None, None]
    ult = np.transpose(ul, (1, 0, 2))                                       # (T, S, n)
    loc = _conv3(ult, g("ped.tpcnn.weight"), g("ped.tpcnn.bias")) \
        + np.einsum("ot,tsn->osn", g("ped.highway.weight")[:, :, 0], ult) + g("ped.highway.bias")[:, None, None]
    To, S = loc.shape[:2]                                                   # (T_out, S, n)
    loc = np.transpose(loc, (1, 0, 2)) if transpose else loc.reshape(To * S, n).reshape(S, To, n)
    return float(g("global_w")[0]) * glob + float(g("local_w")[0]) * loc


def forward(sd, u, bins=BINS, transpose=False):
    """sd: state_dict (numpy), u (T, N) fp32 of ONE scene -> raw output (S, T_out, N) (the network's (1, S, T_out, N)
    without the batch axis); a pedestrian in no zone keeps 0.  The noise term is identically zero and is left out."""
    sd = {k: np.asarray(val, np.float64) for k, val in sd.items()}
    u32 = np.asarray(u, np.float32)
    z = zones(u32, bins)
    S, To = sd["implicit_cells.0.feat.weight"].shape[0], sd["implicit_cells.0.tpcnn.weight"].shape[0]
    out = np.zeros((S, To, u32.shape[1]))
    for i in range(len(bins)):
        sel = z == i
        if sel.any():
            out[:, :, sel] = cell(sd, f"implicit_cells.{i}.", u32[:, sel].astype(np.float64), transpose)
    return out


def c_pred_refine(raw):
    """raw (S, T_out, N) -> (T_out, N, S) (bridge.py:22)"""
    return np.ascontiguousarray(np.transpose(raw, (1, 2, 0)))


def scene_input(C_obs, nrm, lo, hi):
    """v (k+2, n) of the rows [lo, hi) of a split: [C_obs; last observed position - its mean over the scene]"""
    ori = np.asarray(nrm[:2, lo:hi], np.float32)
    ori = ori - ori.mean(axis=1, keepdims=True, dtype=np.float32)
    return np.concatenate([np.asarray(C_obs[:, lo:hi], np.float32), ori]).astype(np.float32)
