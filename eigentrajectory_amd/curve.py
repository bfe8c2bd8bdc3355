"""Curve-fitting baselines of the paper's Table 1 (reference: CurveModel/curve_basis.py, CurveModel/curve_fitting.py,
script/descriptor_evaluation.py:38-85): Linear, Bezier and B-spline descriptors of trajectories, fitted on the GPU by
:func:`eigentrajectory_amd.ops.curve_fit_batch` (csrc/et_curve.hip).

The bases are computed here in fp64 and rounded once to fp32 (no scipy): Bernstein polynomials with exact binomials, and
B-splines by the Cox-de Boor recursion on clamped uniform knots.  They equal the reference's bases to within the ulp bound
stated in tests/test_curve_fit_cpu.py (the reference's binomials come from lgamma / exp in fp32)."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import ops

__all__ = ["linear_basis", "bezier_basis", "bspline_basis", "table_bases", "curve_fitting", "curve_fitting_batch"]


def _grid(step):
    """The reference's sample points: torch.linspace(0, 1, step) in fp32, as fp64."""
    return torch.linspace(0, 1, steps=step, dtype=torch.float32).double().numpy()


def linear_basis(step):
    """(step, 2): columns t and 1 - t on linspace(0, 1, step) (script/descriptor_evaluation.py:41)."""
    return torch.stack([torch.linspace(0, 1, step), torch.linspace(1, 0, step)], dim=1)


def bezier_basis(degree=3, step=13):
    """(step, degree + 1) Bernstein basis: column i = C(degree, i) t^i (1 - t)^(degree - i)."""
    t = _grid(step)[:, None]
    i = np.arange(degree + 1, dtype=np.float64)[None, :]
    binom = np.asarray([math.comb(degree, k) for k in range(degree + 1)], dtype=np.float64)[None, :]
    return torch.from_numpy((binom * t ** i * (1.0 - t) ** (degree - i)).astype(np.float32))


def _cox_de_boor(knots, p, n_basis, x):
    """Values of the n_basis B-splines of degree p on `knots` at x (fp64); x = the last knot takes the last span."""
    m = p
    while m < n_basis - 1 and knots[m + 1] <= x:
        m += 1
    out = np.zeros(n_basis)
    if x < knots[p] or x > knots[n_basis]:
        return out
    nv, left, right = [1.0] + [0.0] * p, [0.0] * (p + 1), [0.0] * (p + 1)
    for j in range(1, p + 1):
        left[j], right[j] = x - knots[m + 1 - j], knots[m + j] - x
        saved = 0.0
        for r in range(j):
            tmp = nv[r] / (right[r + 1] + left[j - r])
            nv[r] = saved + right[r + 1] * tmp
            saved = left[j - r] * tmp
        nv[j] = saved
    out[m - p:m + 1] = nv
    return out


def bspline_basis(cpoint=7, degree=2, step=13):
    """(step, cpoint + 1) clamped uniform B-spline basis of the given degree (cpoint + 1 control points, knots
    0 x degree, linspace(0, 1, cpoint + 2 - degree), 1 x degree), sampled at linspace(0, 1, step); the row at t = 1 is
    the last basis function's 1."""
    n_basis = cpoint + 1
    knots = np.concatenate([np.zeros(degree), np.linspace(0.0, 1.0, n_basis - degree + 1), np.ones(degree)])
    xs = np.linspace(0.0, 1.0, step)
    return torch.from_numpy(np.stack([_cox_de_boor(knots, degree, n_basis, x) for x in xs]).astype(np.float32))


def table_bases(step):
    """The 14 bases of one Table-1 column in the reference's order: [(kind, params, basis)] with kind 'linear' (params
    ()), 'bezier' ((degree,)) for degree 2..5 and 'bspline' ((n_curve, degree)) for degree 1..3, n_curve 2..5 > degree."""
    out = [("linear", (), linear_basis(step))]
    out += [("bezier", (d,), bezier_basis(degree=d, step=step)) for d in range(2, 6)]
    out += [("bspline", (c, d), bspline_basis(cpoint=c, degree=d, step=step))
            for d in range(1, 4) for c in range(2, 6) if c > d]
    return out


def curve_fitting_batch(trajs, bases, steps=100000, lr=1e-4, want_loss=False, want_cp=False):
    """curve_fitting for many (trajectory set, basis) pairs in one launch per pass -> (recons, best_steps, losses):
    recons a list of (N_f, T_f, 2) tensors on the trajectories' device, best_steps (B,) int64 (the step whose recon is
    returned, 0 = the initial guess), losses (B, steps) float64 per-step mean losses or None."""
    device = next((t.device for t in trajs if t.is_cuda), torch.device("cuda", torch.cuda.current_device()))
    res = ops.curve_fit_batch([t.to(device) for t in trajs], [b.to(device) for b in bases], steps=steps, lr=lr,
                              want_cp=want_cp, want_loss=want_loss)
    if want_cp:
        return res["recon"], res["best"], res["loss"], res["cp"]
    return res["recon"], res["best"], res["loss"]


def curve_fitting(traj, basis, steps=100000, lr=1e-4):
    """CurveModel/curve_fitting.py: control points of `basis` (T, ncp) fitted to traj (N, T, 2) by Adam(lr) on the mean
    L2 error; returns recon_best (N, T, 2), the recon of the step with the lowest loss (on the GPU)."""
    return curve_fitting_batch([traj], [basis], steps=steps, lr=lr)[0][0]
