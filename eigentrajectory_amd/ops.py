"""Functional front-end of the HIP kernels (thin: argument marshalling + autograd glue).

Each function enqueues one or two kernels of libetamd.so on the current HIP
stream and returns device tensors; none of them synchronises except
``kmeans_fit`` (the reference synchronises every iteration there,
EigenTrajectory/kmeans.py:239).  Inputs on the CPU are moved to the current HIP
device first; without a HIP device every function raises (no CPU fallback).
"""
from __future__ import annotations

import ctypes as C
import math
from types import SimpleNamespace
from typing import NamedTuple

import torch

from . import _lib as L
from ._native_train import family_name
from ._lib import MODE_IDENTITY, MODE_MOVING, MODE_SPLIT, MODE_STATIC  # noqa: F401  (re-exported)


def _dev_args(device, *tensors):
    return [L.on_device(t, device) for t in tensors]


# ------------------------------------------------------------------------------- TrajNorm
def norm_params(obs, want_ori=True, want_rot=True, want_sca=True):
    """normalizer.py:17-29 -> traj_ori (N,1,2), traj_rot (N,2,2), traj_sca (N,1,1) (None where not wanted)."""
    dev = L.require_device(obs)
    (obs,) = _dev_args(dev, obs)
    n, t, _ = obs.shape
    ori = torch.empty((n, 1, 2), device=dev) if want_ori else None
    rot = torch.empty((n, 2, 2), device=dev) if want_rot else None
    sca = torch.empty((n, 1, 1), device=dev) if want_sca else None
    L.call("et_norm_params", L.ptr(obs), n, t, L.ptr(ori), L.ptr(rot), L.ptr(sca), L.stream(dev))
    return ori, rot, sca


def norm_params_from_nrm(nrm, want_ori=True, want_rot=True, want_sca=True):
    """Same tensors from the compact state nrm (4,N) cached by :func:`norm_project`."""
    dev = L.require_device(nrm)
    (nrm,) = _dev_args(dev, nrm)
    n = nrm.shape[1]
    ori = torch.empty((n, 1, 2), device=dev) if want_ori else None
    rot = torch.empty((n, 2, 2), device=dev) if want_rot else None
    sca = torch.empty((n, 1, 1), device=dev) if want_sca else None
    L.call("et_norm_params_from_nrm", L.ptr(nrm), n, L.ptr(ori), L.ptr(rot), L.ptr(sca), L.stream(dev))
    return ori, rot, sca


def _traj_transform(which, traj, ori, rot, sca):
    """which: "normalize" | "denormalize" -> et_normalize / et_denormalize on contiguous device tensors."""
    n, t, _ = traj.shape
    out = torch.empty_like(traj)
    L.call("et_" + which, L.ptr(traj), n, t, L.ptr(ori), L.ptr(rot), L.ptr(sca), L.ptr(out), L.stream(traj.device))
    return out


class _TrajTransform(torch.autograd.Function):
    """normalizer.py:42-62 are ordinary differentiable torch ops in the reference; here the transform is a kernel,
    so its backward is spelled out.  Differentiable w.r.t. the trajectory only (the parameters come from
    ``calculate_params`` on the observations and carry no gradient path to a predictor):
        normalize    y = ((x - o) @ R) * s      dx = (g * s) @ R^T   = denormalize(g; no origin, R, 1/s)
        denormalize  y = (x / s) @ R^T + o      dx = (g @ R) / s     = normalize(g; no origin, R, 1/s)"""

    @staticmethod
    def forward(ctx, traj, ori, rot, sca, which):
        ctx.saved = (rot, sca, which)
        return _traj_transform(which, traj, ori, rot, sca)

    @staticmethod
    def backward(ctx, grad_out):
        rot, sca, which = ctx.saved
        inv = None if sca is None else (1.0 / sca).contiguous()
        other = "denormalize" if which == "normalize" else "normalize"
        return _traj_transform(other, grad_out.contiguous().float(), None, rot, inv), None, None, None, None


def _traj_op(which, traj, ori, rot, sca):
    dev = L.require_device(traj, ori, rot, sca)
    if traj.device != dev or traj.dtype != torch.float32 or not traj.is_contiguous():
        traj = traj.to(device=dev, dtype=torch.float32).contiguous()  # differentiable
    ori, rot, sca = _dev_args(dev, ori, rot, sca)
    return _TrajTransform.apply(traj, ori, rot, sca, which)


def normalize(traj, ori=None, rot=None, sca=None):
    """normalizer.py:42-51 with explicit parameter tensors (None = that step is off); autograd w.r.t. ``traj``."""
    return _traj_op("normalize", traj, ori, rot, sca)


def denormalize(traj, ori=None, rot=None, sca=None):
    """normalizer.py:53-62; autograd w.r.t. ``traj``."""
    return _traj_op("denormalize", traj, ori, rot, sca)


# ---------------------------------------------------------------------------- projection
def norm_project(obs, pred, U_obs_m, U_pred_m, U_obs_s, U_pred_s, mode, static_dist=0.0,
                 want_nrm=True, want_flag=True, want_obs=True, want_pose=False):
    """descriptor.py:144-160 fused with model.py:73-90.

    Returns (C_obs (k,N) | None, C_pred (k,N) | None, nrm (4,N) | None, flag (N,) uint8 | None) and, with ``want_pose``, a
    fifth element pose (5,N): the normaliser as :func:`anchor_reconstruct_metrics` consumes it (origin, rotation x scale,
    1 / scale with the moving / static decision in its sign).
    """
    dev = L.require_device(obs)
    obs, pred, U_obs_m, U_pred_m, U_obs_s, U_pred_s = _dev_args(dev, obs, pred, U_obs_m, U_pred_m, U_obs_s, U_pred_s)
    n, t_obs, _ = obs.shape
    us_obs = U_obs_m if U_obs_m is not None else U_obs_s
    us_pred = U_pred_m if U_pred_m is not None else U_pred_s
    k = (us_obs if us_obs is not None else us_pred).shape[1]
    t_pred = pred.shape[1] if pred is not None else (us_pred.shape[0] // 2 if us_pred is not None else 1)
    c_obs = torch.empty((k, n), device=dev) if (want_obs and us_obs is not None) else None
    c_pred = torch.empty((k, n), device=dev) if pred is not None else None
    nrm = torch.empty((4, n), device=dev) if want_nrm else None
    flag = torch.empty((n,), device=dev, dtype=torch.uint8) if want_flag else None
    if want_pose:
        pose = torch.empty((5, n), device=dev)
        L.call("et_norm_project_pose", L.ptr(obs), L.ptr(pred), n, t_obs, t_pred, k, L.ptr(U_obs_m), L.ptr(U_pred_m),
               L.ptr(U_obs_s), L.ptr(U_pred_s), int(mode), float(static_dist), L.ptr(c_obs), L.ptr(c_pred), L.ptr(nrm),
               L.ptr(flag), L.ptr(pose), L.stream(dev))
        return c_obs, c_pred, nrm, flag, pose
    L.call("et_norm_project", L.ptr(obs), L.ptr(pred), n, t_obs, t_pred, k, L.ptr(U_obs_m), L.ptr(U_pred_m), L.ptr(U_obs_s),
           L.ptr(U_pred_s), int(mode), float(static_dist), L.ptr(c_obs), L.ptr(c_pred), L.ptr(nrm), L.ptr(flag),
           L.stream(dev))
    return c_obs, c_pred, nrm, flag


# ------------------------------------------------------------------------- reconstruction
def _reconstruct_fwd(Cc, obs, nrm, A_m, A_s, U_m, U_s, mode, static_dist, t_obs):
    dev = Cc.device
    k, n, s = Cc.shape
    u = U_m if U_m is not None else U_s
    t_pred = u.shape[0] // 2
    out = torch.empty((s, n, t_pred, 2), device=dev)
    L.call("et_anchor_reconstruct_fwd", L.ptr(Cc), n, s, k, t_obs, t_pred, L.ptr(obs), L.ptr(nrm), L.ptr(A_m), L.ptr(A_s),
           L.ptr(U_m), L.ptr(U_s), int(mode), float(static_dist), L.ptr(out), L.stream(dev))
    return out


def _reconstruct_bwd(dtraj, obs, nrm, U_m, U_s, mode, static_dist, t_obs):
    dev = dtraj.device
    s, n, t_pred, _ = dtraj.shape
    u = U_m if U_m is not None else U_s
    k = u.shape[1]
    dC = torch.empty((k, n, s), device=dev)
    L.call("et_anchor_reconstruct_bwd", L.ptr(dtraj), n, s, k, t_obs, t_pred, L.ptr(obs), L.ptr(nrm), L.ptr(U_m), L.ptr(U_s),
           int(mode), float(static_dist), L.ptr(dC), L.stream(dev))
    return dC


class _AnchorReconstruct(torch.autograd.Function):
    """Differentiable w.r.t. C only: U, anchors and the normaliser state are detached in the
    reference too (descriptor.py:72,87; anchor.py:87)."""

    @staticmethod
    def forward(ctx, Cc, obs, nrm, A_m, A_s, U_m, U_s, mode, static_dist, t_obs):
        ctx.saved = (obs, nrm, U_m, U_s, mode, static_dist, t_obs)
        return _reconstruct_fwd(Cc, obs, nrm, A_m, A_s, U_m, U_s, mode, static_dist, t_obs)

    @staticmethod
    def backward(ctx, grad_out):
        obs, nrm, U_m, U_s, mode, static_dist, t_obs = ctx.saved
        dC = _reconstruct_bwd(grad_out.contiguous().float(), obs, nrm, U_m, U_s, mode, static_dist, t_obs)
        return (dC,) + (None,) * 9


def anchor_reconstruct(Cc, A_m, A_s, U_m, U_s, mode, static_dist=0.0, *, obs=None, nrm=None, t_obs=8):
    """anchor.py:76-88 + descriptor.py:162-176: C (k,N,S) -> (S,N,T_pred,2); autograd w.r.t. C.

    The normaliser state comes from ``nrm`` (4,N) (as returned by :func:`norm_project`) or is
    recomputed from ``obs`` (N,T_obs,2).
    """
    dev = L.require_device(Cc)
    if Cc.device != dev or Cc.dtype != torch.float32 or not Cc.is_contiguous():
        Cc = Cc.to(device=dev, dtype=torch.float32).contiguous()  # differentiable
    obs, nrm, A_m, A_s, U_m, U_s = _dev_args(dev, obs, nrm, A_m, A_s, U_m, U_s)
    if obs is not None:
        t_obs = obs.shape[1]
    return _AnchorReconstruct.apply(Cc, obs, nrm, A_m, A_s, U_m, U_s, int(mode), float(static_dist), int(t_obs))


def anchor_reconstruct_metrics(Cc, gt, A_m, A_s, U_m, U_s, mode, static_dist=0.0, *, obs=None, nrm=None, pose=None, t_obs=8):
    """Best-of-S ADE / FDE per pedestrian (utils/metrics.py:73-102) fused into the reconstruction:
    C (k,N,S), gt (N,T_pred,2) -> ade (N,), fde (N,).  No autograd (evaluation form).

    ``pose`` (5,N) from ``norm_project(..., want_pose=True)`` (same mode and static_dist): the matrix-core kernel
    (T_pred = 12, k = 6, 12 <= S <= 64) takes the normaliser from it; any other shape needs ``nrm`` or ``obs`` as well."""
    dev = L.require_device(Cc)
    Cc, gt, obs, nrm, A_m, A_s, U_m, U_s, pose = _dev_args(dev, Cc, gt, obs, nrm, A_m, A_s, U_m, U_s, pose)
    k, n, s = Cc.shape
    if obs is not None:
        t_obs = obs.shape[1]
    t_pred = gt.shape[1]
    ade = torch.empty((n,), device=dev)
    fde = torch.empty((n,), device=dev)
    L.call("et_anchor_reconstruct_metrics_pose", L.ptr(Cc), n, s, k, int(t_obs), t_pred, L.ptr(obs), L.ptr(nrm), L.ptr(pose),
           L.ptr(A_m), L.ptr(A_s), L.ptr(U_m), L.ptr(U_s), int(mode), float(static_dist), L.ptr(gt), L.ptr(ade), L.ptr(fde),
           L.stream(dev))
    return ade, fde



# ------------------------------------------------------------------------------------ test metrics (TCC / COL)
METRIC_KEYS = ("ADE", "FDE", "TCC", "COL", "best")


def scene_offsets(sizes, n, device):
    """Scene sizes (pedestrians per scene, in row order) -> int32 offsets (n_scenes + 1,) on ``device``; None -> None
    (the whole batch is one scene).  Checked on the host: non-negative, summing to ``n``."""
    if sizes is None:
        return None
    if torch.is_tensor(sizes):
        sizes = sizes.detach().cpu().tolist()
    sizes = [int(v) for v in sizes]
    if not sizes or min(sizes) < 0 or sum(sizes) != n:
        raise ValueError(f"scene_sizes must be non-negative and sum to the {n} rows (got {len(sizes)} sizes summing to "
                         f"{sum(sizes)})")
    if n > 2**31 - 1:
        raise ValueError("scene_sizes: more than 2^31 - 1 rows")
    off = [0]
    for v in sizes:
        off.append(off[-1] + v)
    return torch.tensor(off, dtype=torch.int32).to(device, non_blocking=True)


def _metric_outputs(n, dev, metrics):
    unknown = set(metrics) - set(METRIC_KEYS)
    if unknown:
        raise ValueError(f"unknown metrics {sorted(unknown)}; choose from {METRIC_KEYS}")
    return {key: torch.empty((n,), device=dev, dtype=torch.int32 if key == "best" else torch.float32)
            for key in METRIC_KEYS if key in metrics}


def _gt3(gt):
    return gt.squeeze(0) if gt.dim() == 4 else gt


def traj_metrics(pred, gt, scene_sizes=None, metrics=METRIC_KEYS):
    """utils/metrics.py:30-155 per pedestrian in one launch: pred (S,N,T,2), gt (N,T,2) or (1,N,T,2) ->
    dict of (N,) tensors: ADE, FDE, TCC, COL (float32) and best (int32, the arg-min sample of the final error).

    ``scene_sizes``: pedestrians per scene in row order (COL compares pairs within a scene only, as the reference's test
    loop calls the metric once per scene); None = one scene of N.  ``metrics`` selects the outputs (leaving out COL skips
    the pair pass)."""
    dev = L.require_device(pred)
    pred, gt = _dev_args(dev, pred, _gt3(gt))
    s, n, t, _ = pred.shape
    if gt.shape != (n, t, 2):
        raise ValueError(f"gt {tuple(gt.shape)} does not match pred {tuple(pred.shape)}")
    off = scene_offsets(scene_sizes, n, dev)
    out = _metric_outputs(n, dev, metrics)
    L.call("et_traj_metrics", L.ptr(pred), n, s, t, L.ptr(gt), L.ptr(off), 0 if off is None else off.numel() - 1,
           L.ptr(out.get("ADE")), L.ptr(out.get("FDE")), L.ptr(out.get("TCC")), L.ptr(out.get("COL")),
           L.ptr(out.get("best")), L.stream(dev))
    return out


def anchor_reconstruct_metrics_scenes(Cc, gt, A_m, A_s, U_m, U_s, mode, static_dist=0.0, *, obs=None, nrm=None, pose=None,
                                      t_obs=8, scene_sizes=None, metrics=METRIC_KEYS):
    """:func:`traj_metrics` of :func:`anchor_reconstruct`'s output without writing it: C (k,N,S), gt (N,T_pred,2) ->
    dict of (N,) tensors (ADE, FDE, TCC, COL, best), every sample reconstructed in registers with the reconstruction's
    own arithmetic.  The normaliser comes from ``nrm`` or ``obs``, else from ``pose`` (within an ulp or two for moving
    rows)."""
    dev = L.require_device(Cc)
    Cc, gt, obs, nrm, A_m, A_s, U_m, U_s, pose = _dev_args(dev, Cc, _gt3(gt), obs, nrm, A_m, A_s, U_m, U_s, pose)
    k, n, s = Cc.shape
    if obs is not None:
        t_obs = obs.shape[1]
    t_pred = gt.shape[1]
    if gt.shape != (n, t_pred, 2):
        raise ValueError(f"gt {tuple(gt.shape)} does not match C {tuple(Cc.shape)}")
    off = scene_offsets(scene_sizes, n, dev)
    out = _metric_outputs(n, dev, metrics)
    L.call("et_anchor_reconstruct_metrics_scenes", L.ptr(Cc), n, s, k, int(t_obs), t_pred, L.ptr(obs), L.ptr(nrm),
           L.ptr(pose), L.ptr(A_m), L.ptr(A_s), L.ptr(U_m), L.ptr(U_s), int(mode), float(static_dist), L.ptr(gt), L.ptr(off),
           0 if off is None else off.numel() - 1, L.ptr(out.get("ADE")), L.ptr(out.get("FDE")), L.ptr(out.get("TCC")),
           L.ptr(out.get("COL")), L.ptr(out.get("best")), L.stream(dev))
    return out


# ------------------------------------------------------------------------ what the ten predictors' wrappers share
class _SceneBatch(NamedTuple):
    """A split as an ``et_*_forward_scenes`` entry point takes it (:func:`_scene_batch`)."""
    C_obs: torch.Tensor       # (k, n) float32 on the device
    nrm: torch.Tensor         # (>= 2, n) float32 on the device
    n: int
    sizes: list               # pedestrians per scene; [n] without scene_sizes
    off: torch.Tensor | None  # int32 offsets (len(sizes) + 1,) on the device; None without scene_sizes
    n_scenes: int             # the entry point's n_scenes: len(sizes), 0 without scene_sizes
    max_n: int                # the largest scene


def _scene_batch(who, dev, C_obs, nrm, k, scene_sizes):
    """The preamble of every ``*_forward_scenes`` wrapper (``who``: its name, for the messages): C_obs (k, N) and nrm
    (2 or more rows, N) moved to ``dev`` and checked, ``scene_sizes`` (list, integer tensor or None) turned into the
    offsets and counts the C entry point takes.  None is one scene of all N rows and passes no offsets; an empty list takes
    N = 0.  What a predictor allows beyond that (a scene limit, a pooling range) is its wrapper's business."""
    C_obs, nrm = _dev_args(dev, C_obs, nrm)
    cs, ns = C_obs.shape, nrm.shape
    if len(cs) != 2 or cs[0] != k or len(ns) != 2 or ns[0] < 2 or ns[1] != cs[1]:
        raise ValueError(f"{who}: C_obs {tuple(cs)} / nrm {tuple(ns)} are not (k, N) / (2 or more, N) with k = {k}")
    n = cs[1]
    sizes, off, n_scenes = _scene_sizes(scene_sizes, n, dev)
    if not sizes and n:
        raise ValueError(f"{who}: no scenes for {n} rows")
    return _SceneBatch(C_obs, nrm, n, sizes, off, n_scenes, max(sizes, default=0))


def _scene_sizes(scene_sizes, n, dev):
    """``scene_sizes`` (list, integer tensor or None) for ``n`` rows -> (sizes, int32 offsets on ``dev``, n_scenes) as a
    ``*_scenes`` entry point takes them: the one place that makes them.  None is one scene of all ``n`` rows and passes no
    offsets: ([n], None, 0); an empty list passes the offsets [0]."""
    if scene_sizes is None:
        return [n], None, 0
    sizes = [int(s) for s in (scene_sizes.tolist() if torch.is_tensor(scene_sizes) else scene_sizes)]
    off = scene_offsets(sizes, n, dev) if sizes else torch.zeros((1,), device=dev, dtype=torch.int32)
    return sizes, off, len(sizes)


def _workspace(entry_name, dev, params, *args, required=False):
    """(uint8 tensor on ``dev`` | None, its size) as ``entry_name``, an ``et_*_workspace_bytes``, sizes it for ``params`` and
    ``args``.  ``required``: the predictor needs a workspace for any input, so a zero answer means that the library
    refuses ``params`` (status 3)."""
    nbytes = getattr(L.lib(), entry_name)(C.byref(params), *args)
    if required and not nbytes:
        L.check(3, entry_name)  # outside the native family
    return (torch.empty((nbytes,), device=dev, dtype=torch.uint8) if nbytes else None), nbytes


def _read_in_place(who, dev, tensors):
    """``tensors`` {name: tensor}: ``*_forward_graph`` inputs that the kernels read where they are (nothing is moved or copied
    for the caller)"""
    for name, t in tensors.items():
        if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous float32 tensor on {dev} (got {t.dtype}, {t.device}, "
                             f"contiguous={t.is_contiguous()})")


# ------------------------------------------------------ what the five scene-graph predictors' training wrappers share
# (SocialSTGCNN, SGCN, GPGraph around SGCN, SocialDMRGCN, GraphTERNLight: ``prefix`` below is stgcnn, sgcn, gpgraph_sgcn,
# dmrgcn or graphtern, the middle of their entry points' and wrappers' names)
def _numel(t):
    return 0 if t is None else t.numel()


def _check_train_ws(who, dev, workspace, maker):
    if workspace is None or workspace.device != dev or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise ValueError(f"{who}: workspace is not a contiguous uint8 tensor on {dev} ({maker} makes one)")


def _backward_args(who, grad_floats_entry, params, dev, d_out, shape):
    """The preamble of a ``*_backward_graph`` / ``_scenes`` wrapper: ``d_out`` checked against ``shape`` and made a contiguous
    float32 tensor on ``dev`` -> (d_out, the empty flat gradient buffer, sized by ``grad_floats_entry``)."""
    if tuple(d_out.shape) != shape:
        raise ValueError(f"{who}: d_out {tuple(d_out.shape)} is not {shape}")
    d_out = d_out.detach()
    if d_out.device != dev or d_out.dtype != torch.float32 or not d_out.is_contiguous():
        d_out = d_out.to(device=dev, dtype=torch.float32).contiguous()
    size = int(getattr(L.lib(), grad_floats_entry)(C.byref(params)))
    if not size:
        L.check(3, grad_floats_entry)
    return d_out, torch.empty((size,), device=dev)


def _grad_views(who, model, grads):
    out, at, size = {}, 0, grads.numel()
    for name, t in model.named_parameters():
        k = t.numel()
        if at + k <= size:   # (a short buffer is refused below, with the count it should have)
            out[name] = grads[at:at + k].view(t.shape)
        at += k
    if at != size:
        raise ValueError(f"{who}: {size} floats for parameters of {at}")
    return out


def _layout(entry, names, params, *args):
    """-> the offsets of a training workspace as ``entry``, an ``et_*_train_layout``, gives them for ``args``, by the
    ``names`` of ``_lib.*_TRAIN_LAYOUT_NAMES`` (the C enum's order)"""
    o = (C.c_int64 * len(names))()
    L.call(entry, C.byref(params), *args, o, len(names))
    return SimpleNamespace(**{name: int(x) for name, x in zip(names, o)})


def _train_params(who, model, et_params):
    """-> (params, device) of ``model`` for the training wrapper ``who``; ``et_params``: what the caller holds already"""
    if et_params is not None:   # the training Function's calls: its forward() has looked at the family already
        return et_params
    why = model.outside_native_training()
    if why is not None:
        raise NotImplementedError(f"{who}: {family_name(model)} has no native backward pass outside its native family: {why}")
    return model.et_params()


def _train_workspace(prefix, model, et_params, n, *sizes):
    """the body of ``{prefix}_train_workspace``: ``sizes`` are the entry point's arguments after ``n``"""
    params, dev = _train_params(f"{prefix}_train_workspace", model, et_params)
    return _workspace(f"et_{prefix}_train_workspace_bytes", dev, params, n, *sizes, required=n > 0)[0]


def _backward_graph(prefix, model, workspace, d_out, et_params, n_axis, shape):
    """the body of ``{prefix}_backward_graph``: ``d_out`` is 4-d with N on ``n_axis``, ``shape(params, n)`` what it must be"""
    who = f"{prefix}_backward_graph"
    params, dev = _train_params(who, model, et_params)
    n = d_out.shape[n_axis] if d_out.dim() == 4 else -1
    d_out, grads = _backward_args(who, f"et_{prefix}_grad_floats", params, dev, d_out, shape(params, n))
    if n:
        _check_train_ws(who, dev, workspace, f"{prefix}_train_workspace")
    L.call(f"et_{prefix}_backward_graph", C.byref(params), n, L.ptr(d_out), L.ptr(grads), grads.numel(), L.ptr(workspace),
           _numel(workspace), L.stream(dev))
    return grads


def _backward_scenes(prefix, model, workspace, d_out, scene_sizes, k_S, packed=False, cap=None):
    """the body of ``{prefix}_backward_scenes``: ``d_out`` is (k, N, S) with ``k_S(params)`` = (k, S).  ``packed``: the entry
    point also takes the sum of n^2 over the scenes (of at most ``cap`` pedestrians, if given) and the largest scene"""
    who = f"{prefix}_backward_scenes"
    params, dev = _train_params(who, model, None)
    n = d_out.shape[1] if d_out.dim() == 3 else -1
    k, S = k_S(params)
    d_out, grads = _backward_args(who, f"et_{prefix}_grad_floats", params, dev, d_out, (k, n, S))
    sizes, off, n_scenes = _scene_sizes(scene_sizes, n, dev)
    if n:
        _check_train_ws(who, dev, workspace, f"{prefix}_train_workspace")
    sums = (sum(s * s for s in sizes if cap is None or s <= cap), max(sizes, default=0)) if packed else ()
    L.call(f"et_{prefix}_backward_scenes", C.byref(params), n, L.ptr(off), n_scenes, *sums, L.ptr(d_out), L.ptr(grads),
           grads.numel(), L.ptr(workspace), _numel(workspace), L.stream(dev))
    return grads


def _keep_mask(who, dev, keep, shape=None, numel=None):
    """the keep mask as the kernel reads it: contiguous uint8 on ``dev`` of ``shape`` (or of ``numel`` entries); None stays"""
    if keep is None:
        return None
    if keep.dtype != torch.uint8 or (shape is not None and tuple(keep.shape) != shape) or \
            (numel is not None and keep.numel() != numel):
        raise ValueError(f"{who}: keep {tuple(keep.shape)} {keep.dtype} is not uint8 "
                         f"{shape if shape is not None else f'of {numel} entries'}")
    return keep.to(dev).contiguous()


def _keep_offsets(scene_sizes, cap, device):
    """-> (int64 tensor (n_scenes + 1,): the running sum of n^2, a scene of more than ``cap`` pedestrians taking no room; the
    total)"""
    off = [0]
    for s in scene_sizes:
        off.append(off[-1] + (int(s) ** 2 if int(s) <= cap else 0))
    t = torch.tensor(off, dtype=torch.int64)
    return (t if device is None else t.to(device)), off[-1]


# ------------------------------------------------------------------------ Social-STGCNN predictor (inference)
def _stgcnn_graph_args(who, params, dev, v, a):
    """v (1, 1, K, N) and a (K, N, N) of a graph-form call, checked and on ``dev`` -> (v, a, N)"""
    K, n = params.seq_len, v.shape[-1]
    if tuple(v.shape) != (1, 1, K, n) or tuple(a.shape) != (K, n, n):
        raise ValueError(f"{who}: v {tuple(v.shape)} / a {tuple(a.shape)} are not (1,1,{K},N) / ({K},N,N)")
    return (*_dev_args(dev, v.detach(), a.detach()), n)


def stgcnn_forward_graph(model, v, a):
    """``model`` (:class:`eigentrajectory_amd.stgcnn.SocialSTGCNN`, eval mode) on one scene as the stgcnn bridge hands it
    over: v (1, 1, K, N), a (K, N, N) -> the raw output (1, S, k, N).  One launch."""
    if getattr(model, "graph_per_time_row", False):
        raise NotImplementedError("stgcnn_forward_graph: a per-time-row SocialSTGCNN (graph_per_time_row=True) runs only inside "
                                  "GPGraphSTGCNN")
    params, dev = model.et_params()
    v, a, n = _stgcnn_graph_args("stgcnn_forward_graph", params, dev, v, a)
    out = torch.empty((1, params.output_feat, params.pred_seq_len, n), device=dev)
    ws, nbytes = _workspace("et_stgcnn_workspace_bytes", dev, params, n, n)
    L.call("et_stgcnn_forward_graph", C.byref(params), L.ptr(v), L.ptr(a), n, L.ptr(out), L.ptr(ws), nbytes, L.stream(dev))
    return out


def stgcnn_forward_scenes(model, C_obs, nrm, scene_sizes=None):
    """The stgcnn bridge + ``model`` (eval mode) + the post-hook for every scene of a split in ONE launch: C_obs (k, N) and
    nrm (4, N) of :func:`norm_project` (rows 0-1: the last observed positions, centred here per scene), ``scene_sizes``
    pedestrians per scene in row order as a list or an integer tensor (None = one scene; an empty list takes N = 0) ->
    C_pred_refine (k, N, S).  The other nine ``*_forward_scenes`` take these three arguments the same way."""
    if getattr(model, "graph_per_time_row", False):
        raise NotImplementedError("stgcnn_forward_scenes: a per-time-row SocialSTGCNN (graph_per_time_row=True) runs only inside "
                                  "GPGraphSTGCNN")
    params, dev = model.et_params()
    b = _scene_batch("stgcnn_forward_scenes", dev, C_obs, nrm, params.pred_seq_len, scene_sizes)
    out = torch.empty((params.pred_seq_len, b.n, params.output_feat), device=dev)
    ws, nbytes = _workspace("et_stgcnn_workspace_bytes", dev, params, b.n, b.max_n)
    L.call("et_stgcnn_forward_scenes", C.byref(params), L.ptr(b.C_obs), L.ptr(b.nrm), b.n, L.ptr(b.off), b.n_scenes,
           L.ptr(out), L.ptr(ws), nbytes, L.stream(dev))
    return out


# ------------------------------------------------------------------------ Social-STGCNN predictor (training)
def stgcnn_train_workspace(model, n, n_scenes=1, et_params=None):
    """A training workspace for ``n`` pedestrians in ``n_scenes`` scenes: :func:`stgcnn_train_forward_graph` / ``_scenes``
    fill it, :func:`stgcnn_backward_graph` / ``_scenes`` read it."""
    return _train_workspace("stgcnn", model, et_params, n, max(n_scenes, 1))


def stgcnn_train_forward_graph(model, v, a, workspace, et_params=None):
    """``model`` in training mode on one scene as the stgcnn bridge hands it over: v (1, 1, K, N), a (K, N, N) -> the raw
    output (1, S, k, N).  The three BatchNorms use the scene's batch statistics, and their running statistics and
    ``num_batches_tracked`` are updated in place; every intermediate stays in ``workspace`` (of
    :func:`stgcnn_train_workspace`) for :func:`stgcnn_backward_graph`.  Two launches."""
    params, dev = _train_params("stgcnn_train_forward_graph", model, et_params)
    v, a, n = _stgcnn_graph_args("stgcnn_train_forward_graph", params, dev, v, a)
    out = torch.empty((1, params.output_feat, params.pred_seq_len, n), device=dev)
    if n:
        _check_train_ws("stgcnn_train_forward_graph", dev, workspace, "stgcnn_train_workspace")
    train = model.et_train_state()
    L.call("et_stgcnn_train_forward_graph", C.byref(params), C.byref(train), L.ptr(v), L.ptr(a), n, L.ptr(out),
           L.ptr(workspace), _numel(workspace), L.stream(dev))
    return out


def stgcnn_train_forward_scenes(model, C_obs, nrm, scene_sizes=None, workspace=None):
    """The stgcnn bridge + ``model`` in training mode + the post-hook for every scene of a batch in two launches, one
    workgroup per scene: each scene is normalised with its own batch statistics, and the running statistics end as after
    consecutive single-scene calls in row order (an empty scene is no batch).  C_obs, nrm and ``scene_sizes`` as
    :func:`stgcnn_forward_scenes` -> (C_pred_refine (k, N, S), workspace); the workspace (made here unless given) goes to
    :func:`stgcnn_backward_scenes` with the same ``scene_sizes``."""
    params, dev = _train_params("stgcnn_train_forward_scenes", model, None)
    b = _scene_batch("stgcnn_train_forward_scenes", dev, C_obs, nrm, params.pred_seq_len, scene_sizes)
    if workspace is None:
        workspace = stgcnn_train_workspace(model, b.n, len(b.sizes), et_params=(params, dev))
    if b.n:
        _check_train_ws("stgcnn_train_forward_scenes", dev, workspace, "stgcnn_train_workspace")
    out = torch.empty((params.pred_seq_len, b.n, params.output_feat), device=dev)
    train = model.et_train_state()
    L.call("et_stgcnn_train_forward_scenes", C.byref(params), C.byref(train), L.ptr(b.C_obs), L.ptr(b.nrm), b.n, L.ptr(b.off),
           b.n_scenes, L.ptr(out), L.ptr(workspace), _numel(workspace), L.stream(dev))
    return out, workspace


def stgcnn_grad_views(model, grads):
    """``grads``, the flat buffer of :func:`stgcnn_backward_graph` / ``_scenes`` -> {state_dict key: a view of it shaped like
    the parameter}, every parameter of ``model`` (state_dict order; the unused tail ``tpcnns[n_txpcnn-1]`` /
    ``prelus[n_txpcnn-1]`` holds exact zeros)."""
    return _grad_views("stgcnn_grad_views", model, grads)


def stgcnn_backward_graph(model, workspace, d_out, et_params=None):
    """The backward pass of :func:`stgcnn_train_forward_graph` in two launches: ``workspace`` as that call filled it (same
    weights), ``d_out`` (1, S, k, N) the gradient at its output -> the flat float32 gradient buffer
    (:func:`stgcnn_grad_views` names its parts)."""
    return _backward_graph("stgcnn", model, workspace, d_out, et_params, -1,
                           lambda p, n: (1, p.output_feat, p.pred_seq_len, n))


def stgcnn_backward_scenes(model, workspace, d_out, scene_sizes=None):
    """The backward pass of :func:`stgcnn_train_forward_scenes` in two launches whatever the number of scenes:
    ``workspace`` as that call filled it, ``scene_sizes`` as given to it, ``d_out`` (k, N, S) -> the flat gradient buffer,
    summed over the scenes in ascending order."""
    return _backward_scenes("stgcnn", model, workspace, d_out, scene_sizes, lambda p: (p.pred_seq_len, p.output_feat))


def stgcnn_train_views(model, workspace, n, n_scenes=1, lo=0, scene=0, scene_n=None):
    """The values kept in ``workspace`` by name, as views, for scene number ``scene`` of ``scene_n`` pedestrians that starts
    at row ``lo`` (one scene: the defaults).  Forward: ``u`` (K, n), ``d`` (K, n) (scenes form), ``P`` (K, K + 1, n) (the
    contraction rows, the ones row last), ``g`` (the gcn output), ``a1`` / ``y`` (tcn.1's input and output), ``t`` (tcn.2's
    output), ``r`` (residual.0's output), ``s`` (the pre-residual sum, the block PReLU's input), ``x`` -- (S, K, n) each --
    ``tp_pre`` / ``tp_out`` [applied tpcnns] x (k, S, n), and ``stats`` (3, 5, S): per BatchNorm (tcn.0, tcn.3, residual.1)
    mean, biased variance, 1/sqrt(var + eps) and, after a backward call, mean(dy), mean(dy x^).  After a backward call also
    ``d_fin`` (k, S, n), ``d_tp_pre`` / ``d_tp_out``, ``d_x``, ``d_s``, ``d_t``, ``d_r``, ``d_y``, ``d_a1``, ``d_g`` and
    ``partial``, the scene's own flat gradient.  The offsets are the library's (``et_stgcnn_train_layout``)."""
    params, _ = model.et_params()
    K, k, S = params.seq_len, params.pred_seq_len, params.output_feat
    m = n if scene_n is None else scene_n
    f = workspace.view(torch.float32)
    lay = _layout("et_stgcnn_train_layout", L.STGCNN_TRAIN_LAYOUT_NAMES, params, n, n_scenes)
    base = lo * lay.per
    fld = lambda off, *shape: f[base + off * m:base + off * m + math.prod(shape) * m].view(*shape, m)
    A = max(1, params.n_txpcnn - 1)
    views = {"u": fld(lay.u, K), "d": fld(lay.d, K), "P": fld(lay.P, K, K + 1)}
    for name in ("g", "a1", "y", "t", "r", "s", "x"):
        views[name] = fld(getattr(lay, name), S, K)
    for name in ("dx", "ds", "dt", "dr", "dy", "da1", "dg"):
        views["d_" + name[1:]] = fld(getattr(lay, name), S, K)
    views["tp_pre"] = [fld(lay.tp + 2 * j * k * S, k, S) for j in range(A)]
    views["tp_out"] = [fld(lay.tp + (2 * j + 1) * k * S, k, S) for j in range(A)]
    views["d_tp_pre"] = [fld(lay.dtp + 2 * j * k * S, k, S) for j in range(A)]
    views["d_tp_out"] = [fld(lay.dtp + (2 * j + 1) * k * S, k, S) for j in range(A)]
    views["d_fin"] = fld(lay.dfin, k, S)
    views["stats"] = f[lay.stats + scene * lay.stat_stride:lay.stats + (scene + 1) * lay.stat_stride].view(3, 5, S)
    views["partial"] = f[lay.partials + scene * lay.grads:lay.partials + (scene + 1) * lay.grads]
    return views


# ------------------------------------------------------------------------------ SGCN predictor (inference)
def _sgcn_logits(want, T, n, sum_n2, dev):
    if not want:
        return None, None
    return torch.empty((4 * T * sum_n2,), device=dev), torch.empty((n * 4 * T * T,), device=dev)


def _sgcn_graph_args(who, params, dev, v, identity):
    """v (1, T, N, 1) and the two identities of a graph-form call, checked (they are read in place) -> (id_s, id_t, N)"""
    T = params.obs_len
    id_s, id_t = identity
    n = v.shape[2] if v.dim() == 4 else -1
    if (tuple(v.shape) != (1, T, n, 1) or tuple(id_s.shape) not in ((1, n, n), (T, n, n))
            or tuple(id_t.shape) not in ((n, 1, 1), (n, T, T))):
        raise ValueError(f"{who}: v {tuple(v.shape)} / identity {tuple(id_s.shape)}, {tuple(id_t.shape)} are not "
                         f"(1,{T},N,1) / (1 or {T},N,N), (N,1,1) or (N,{T},{T})")
    _read_in_place(who, dev, {"v": v, "identity[0]": id_s, "identity[1]": id_t})
    if n > L.SGCN_MAX_N:
        raise ValueError(f"{who}: N = {n} exceeds the {L.SGCN_MAX_N} pedestrians a scene may have")
    return id_s, id_t, n


def sgcn_forward_graph(model, v, identity, want_logits=False):
    """``model`` (:class:`eigentrajectory_amd.sgcn.SGCN`, eval mode) on one scene as the sgcn bridge hands it over: v
    (1, T, N, 1), identity = [spatial (1 or T, N, N), temporal (N, 1, 1) or (N, T, T)] -> (pred_len, N, out_dims); with
    ``want_logits`` also the values that enter the interaction mask's sigmoids, logit_s (T, 4, N, N) and logit_t
    (N, 4, T, T).  The inputs must be contiguous float32 tensors on the model's device (they are read in place)."""
    model._check_mode()
    if getattr(model, "position_channel", False):
        raise NotImplementedError("sgcn_forward_graph: a two-channel SGCN (position_channel=True) runs only inside GPGraphSGCN")
    params, dev = model.et_params()
    T, k, S = params.obs_len, params.pred_len, params.out_dims
    id_s, id_t, n = _sgcn_graph_args("sgcn_forward_graph", params, dev, v, identity)
    out = torch.empty((k, n, S), device=dev)
    ls, lt = _sgcn_logits(want_logits, T, n, n * n, dev)
    ws, nbytes = _workspace("et_sgcn_workspace_bytes", dev, params, n, n * n, 1)
    L.call("et_sgcn_forward_graph", C.byref(params), L.ptr(v.detach()), L.ptr(id_s.detach()), int(id_s.shape[0]),
           L.ptr(id_t.detach()), int(id_t.shape[1]), n, L.ptr(out), L.ptr(ls), L.ptr(lt), L.ptr(ws), nbytes, L.stream(dev))
    if want_logits:
        return out, ls.view(T, 4, n, n), lt.view(n, 4, T, T)
    return out


def sgcn_forward_scenes(model, C_obs, nrm, scene_sizes=None, want_logits=False):
    """The sgcn bridge + ``model`` (eval mode) + the post-hook for every scene of a split in a fixed number of launches:
    C_obs, nrm and ``scene_sizes`` as :func:`stgcnn_forward_scenes` -> C_pred_refine (k, N, S).  A scene of more than 512
    pedestrians raises ValueError.  With ``want_logits`` also the packed logits: scene s's (T, 4, n, n) block at
    4 T (n_0^2 + ... + n_{s-1}^2) of the first and its (n, 4, T, T) block at 4 T T (n_0 + ... + n_{s-1}) of the second."""
    model._check_mode()
    if getattr(model, "position_channel", False):
        raise NotImplementedError("sgcn_forward_scenes: a two-channel SGCN (position_channel=True) runs only inside GPGraphSGCN")
    params, dev = model.et_params()
    b = _scene_batch("sgcn_forward_scenes", dev, C_obs, nrm, params.pred_len, scene_sizes)
    n = b.n
    if b.max_n > L.SGCN_MAX_N:
        raise ValueError(f"sgcn_forward_scenes: a scene of {b.max_n} pedestrians exceeds the {L.SGCN_MAX_N} a scene may have")
    sum_n2 = sum(s * s for s in b.sizes)
    out = torch.empty((params.pred_len, n, params.out_dims), device=dev)
    ls, lt = _sgcn_logits(want_logits, params.obs_len, n, sum_n2, dev)
    ws, nbytes = _workspace("et_sgcn_workspace_bytes", dev, params, n, sum_n2, len(b.sizes))
    L.call("et_sgcn_forward_scenes", C.byref(params), L.ptr(b.C_obs), L.ptr(b.nrm), n, L.ptr(b.off), b.n_scenes, sum_n2,
           b.max_n, L.ptr(out), L.ptr(ls), L.ptr(lt), L.ptr(ws), nbytes, L.stream(dev))
    return (out, ls, lt) if want_logits else out


# ------------------------------------------------------------------------------ SGCN predictor (training)
def sgcn_train_workspace(model, n, sum_n2=None, n_scenes=1, et_params=None):
    """A training workspace for ``n`` pedestrians in ``n_scenes`` scenes whose squared sizes sum to ``sum_n2`` (one scene:
    n * n): :func:`sgcn_train_forward_graph` / ``_scenes`` fill it, :func:`sgcn_backward_graph` / ``_scenes`` read it."""
    return _train_workspace("sgcn", model, et_params, n, n * n if sum_n2 is None else sum_n2, n_scenes)


def sgcn_train_forward_graph(model, v, identity, workspace, want_logits=False, et_params=None):
    """:func:`sgcn_forward_graph` with the kept layout (the same kernels; the output is bit-equal): every asymmetric layer's
    input, the softmax row records, A_t, f1, f2, ts and the tail's activations stay in ``workspace`` (of
    :func:`sgcn_train_workspace`) for :func:`sgcn_backward_graph`."""
    params, dev = _train_params("sgcn_train_forward_graph", model, et_params)
    T, k, S = params.obs_len, params.pred_len, params.out_dims
    id_s, id_t, n = _sgcn_graph_args("sgcn_train_forward_graph", params, dev, v, identity)
    _check_train_ws("sgcn_train_forward_graph", dev, workspace, "sgcn_train_workspace")
    out = torch.empty((k, n, S), device=dev)
    ls, lt = _sgcn_logits(want_logits, T, n, n * n, dev)
    L.call("et_sgcn_train_forward_graph", C.byref(params), L.ptr(v.detach()), L.ptr(id_s.detach()), int(id_s.shape[0]),
           L.ptr(id_t.detach()), int(id_t.shape[1]), n, L.ptr(out), L.ptr(ls), L.ptr(lt), L.ptr(workspace), workspace.numel(),
           L.stream(dev))
    if want_logits:
        return out, ls.view(T, 4, n, n), lt.view(n, 4, T, T)
    return out


def sgcn_train_forward_scenes(model, C_obs, nrm, scene_sizes=None, want_logits=False, workspace=None):
    """:func:`sgcn_forward_scenes` with the kept layout -> (C_pred_refine (k, N, S)[, logit_s, logit_t], workspace); the
    workspace (made here unless given) goes to :func:`sgcn_backward_scenes` with the same ``scene_sizes``."""
    params, dev = _train_params("sgcn_train_forward_scenes", model, None)
    b = _scene_batch("sgcn_train_forward_scenes", dev, C_obs, nrm, params.pred_len, scene_sizes)
    n = b.n
    if b.max_n > L.SGCN_MAX_N:
        raise ValueError(f"sgcn_train_forward_scenes: a scene of {b.max_n} pedestrians exceeds the {L.SGCN_MAX_N} a scene may "
                         "have")
    sum_n2 = sum(s * s for s in b.sizes)
    if workspace is None:
        workspace = sgcn_train_workspace(model, n, sum_n2, len(b.sizes), et_params=(params, dev))
    if n:
        _check_train_ws("sgcn_train_forward_scenes", dev, workspace, "sgcn_train_workspace")
    out = torch.empty((params.pred_len, n, params.out_dims), device=dev)
    ls, lt = _sgcn_logits(want_logits, params.obs_len, n, sum_n2, dev)
    L.call("et_sgcn_train_forward_scenes", C.byref(params), L.ptr(b.C_obs), L.ptr(b.nrm), n, L.ptr(b.off), b.n_scenes, sum_n2,
           b.max_n, L.ptr(out), L.ptr(ls), L.ptr(lt), L.ptr(workspace), _numel(workspace), L.stream(dev))
    return (out, ls, lt, workspace) if want_logits else (out, workspace)


def sgcn_grad_views(model, grads):
    """``grads``, the flat buffer of :func:`sgcn_backward_graph` / ``_scenes`` -> {state_dict key: a view of it shaped like
    the parameter}, every parameter of ``model`` (state_dict order)."""
    return _grad_views("sgcn_grad_views", model, grads)


def sgcn_backward_graph(model, identity, workspace, d_out, et_params=None):
    """The backward pass of :func:`sgcn_train_forward_graph` in ``number_asymmetric_conv_layer + 8`` launches: ``identity``
    and ``workspace`` as that call read / filled them (same weights), ``d_out`` (pred_len, N, out_dims) the gradient at its
    output -> the flat float32 gradient buffer (:func:`sgcn_grad_views` names its parts)."""
    params, dev = _train_params("sgcn_backward_graph", model, et_params)
    id_s, id_t = identity
    n = id_s.shape[-1]
    _read_in_place("sgcn_backward_graph", dev, {"identity[0]": id_s, "identity[1]": id_t})
    _check_train_ws("sgcn_backward_graph", dev, workspace, "sgcn_train_workspace")
    d_out, grads = _backward_args("sgcn_backward_graph", "et_sgcn_grad_floats", params, dev, d_out,
                                  (params.pred_len, n, params.out_dims))
    L.call("et_sgcn_backward_graph", C.byref(params), L.ptr(id_s.detach()), int(id_s.shape[0]), L.ptr(id_t.detach()),
           int(id_t.shape[1]), n, L.ptr(d_out), L.ptr(grads), grads.numel(), L.ptr(workspace), workspace.numel(),
           L.stream(dev))
    return grads


def sgcn_backward_scenes(model, workspace, d_out, scene_sizes=None):
    """The backward pass of :func:`sgcn_train_forward_scenes`, the same number of launches whatever the number of scenes:
    ``workspace`` as that call filled it, ``scene_sizes`` as given to it, ``d_out`` (k, N, S) -> the flat gradient buffer,
    summed over the scenes in ascending order."""
    return _backward_scenes("sgcn", model, workspace, d_out, scene_sizes, lambda p: (p.pred_len, p.out_dims), packed=True)


def sgcn_train_views(model, workspace, n, sum_n2=None, n_scenes=1, lo=0, sq=0, scene_n=None):
    """The values kept in ``workspace`` by name, as views, for the scene of ``scene_n`` pedestrians that starts at row ``lo``
    and at ``sq`` in the packed n^2 stacks (one scene: the defaults).  Forward: ``v`` (T, n), ``stack_s`` [n_asym + 1] x
    (T, 4, n, n) and ``stack_t`` [n_asym + 1] x (n, 4, T, T) (every asymmetric layer's input; the last ones are the logits,
    ``stack_t[0]`` is the temporal attention), ``rows_s`` (T, 4, n, 2) / ``rows_t`` (n, 4, T, 2) (softmax maximum and sum),
    ``at`` (n, 4, T, T), ``f1`` (T, 4, n, 16), ``f2`` / ``ts`` (n, 4, T, 16), and of the tail per pedestrian ``st_pre``
    (n, T, 64) (spatial_temporal gcn 1 before its PReLU), ``rep`` (n, T, 64) (the tcns' input), ``tcn_pre`` / ``tcn_out``
    [n_tcn] x (n, k, 64).  After a backward call also what it left: ``d_ts``, ``d_f2`` (n, 4, T, 16), ``d_f1`` (T, 4, n, 16),
    ``d_at`` (the tail's part), ``d_accn`` (T, 4, n, 16) (d (A_s f2) per spatial row), ``g_s`` / ``g_t`` (the gradient of every
    kept stack), ``dir_s`` / ``dir_t`` (the direct parts of d dense) and ``dd_s`` (d dense_s).  The offsets are the library's
    (``et_sgcn_train_layout``)."""
    params, _ = model.et_params()
    T, k, na, nt = params.obs_len, params.pred_len, params.n_asym, params.n_tcn
    N, n2 = n, n * n if sum_n2 is None else sum_n2
    m = N if scene_n is None else scene_n
    f = workspace.view(torch.float32)
    lay = _layout("et_sgcn_train_layout", L.SGCN_TRAIN_LAYOUT_NAMES, params, N, n2, n_scenes)
    sl = lambda off, cnt, *shape: f[off:off + cnt].view(*shape)
    rows = lambda off: sl(off + lo * 4 * T * T, m * 4 * T * T, m, 4, T, T)          # (n, 4, T, T) blocks
    feat = lambda off, *shape: sl(off + lo * 4 * T * 16, m * 4 * T * 16, *shape)     # 64 T floats per pedestrian
    dense = lambda off: sl(off + 4 * T * sq, 4 * T * m * m, T, 4, m, m)              # (T, 4, n, n) blocks
    keep = sl(lay.keep + lo * lay.keep_stride, m * lay.keep_stride, m, 2 * T + 2 * nt * k, 64)
    return {
        "v": sl(lay.v + T * lo, T * m, T, m),
        "stack_s": [dense(lay.stack_s + j * lay.stack_s_stride) for j in range(na + 1)],
        "stack_t": [rows(lay.stack_t + j * lay.stack_t_stride) for j in range(na + 1)],
        "rows_s": sl(lay.rows_s + 2 * T * 4 * lo, 2 * T * 4 * m, T, 4, m, 2),
        "rows_t": sl(lay.rows_t + 2 * T * 4 * lo, 2 * T * 4 * m, m, 4, T, 2),
        "at": rows(lay.at), "f1": feat(lay.f1, T, 4, m, 16), "f2": feat(lay.f2, m, 4, T, 16), "ts": feat(lay.ts, m, 4, T, 16),
        "st_pre": keep[:, :T], "rep": keep[:, T:2 * T],
        "tcn_pre": [keep[:, 2 * T + 2 * j * k:2 * T + (2 * j + 1) * k] for j in range(nt)],
        "tcn_out": [keep[:, 2 * T + (2 * j + 1) * k:2 * T + (2 * j + 2) * k] for j in range(nt)],
        "d_ts": feat(lay.d_ts, m, 4, T, 16), "d_f2": feat(lay.d_f2, m, 4, T, 16), "d_f1": feat(lay.d_f1, T, 4, m, 16),
        "d_at": rows(lay.d_at), "d_accn": sl(lay.rrec + 4 * T * lo * 17, 4 * T * m * 17, T, 4, m, 17)[..., 1:],
        "g_s": [dense(lay.g_s + j * lay.stack_s_stride) for j in range(na + 1)],
        "g_t": [rows(lay.g_t + j * lay.stack_t_stride) for j in range(na + 1)],
        "dir_s": dense(lay.dir_s), "dir_t": rows(lay.dir_t), "dd_s": dense(lay.dd_s),
    }


# ------------------------------------------------------------------------ GP-Graph-SGCN predictor (inference)
def _gpgraph_buffers(params, want, T, n, sum_n2, n_scenes, dev):
    ws, nbytes = _workspace("et_gpgraph_sgcn_workspace_bytes", dev, params, n, sum_n2, n_scenes, required=True)
    gi = torch.empty((n,), device=dev, dtype=torch.int32)
    if not want:
        return ws, nbytes, gi, None, None, None
    return (ws, nbytes, gi, torch.empty((sum_n2,), device=dev), torch.empty((3 * 4 * T * sum_n2,), device=dev),
            torch.empty((3 * n * 4 * T * T,), device=dev))


def gpgraph_sgcn_forward_graph(model, v_abs, v_rel, want_details=False):
    """``model`` (:class:`eigentrajectory_amd.gpgraph.GPGraph`, eval mode) on one scene as the gpgraphsgcn bridge hands it
    over: v_abs (1, 1, T, N), v_rel (1, 2, T, N) (channel 0 the position) -> ``(v (1, S, k, N), indices (N,) int64)``; with
    ``want_details`` a dict is returned as third item: ``dist`` (N, N), ``n_groups``, and per pass m (0 pedestrian graph, 1
    group means, 2 intra-group) ``logit_s[m]`` (T, 4, n_m, n_m) and ``logit_t[m]`` (n_m, 4, T, T), n_1 = the number of
    groups.  The inputs must be contiguous float32 tensors on the model's device (they are read in place)."""
    model._check_mode()
    params, dev = model.et_params()
    T, k, S = params.base.obs_len, params.base.pred_len, params.base.out_dims
    n = v_abs.shape[3] if v_abs.dim() == 4 else -1
    if tuple(v_abs.shape) != (1, 1, T, n) or tuple(v_rel.shape) != (1, 2, T, n):
        raise ValueError(f"gpgraph_sgcn_forward_graph: v_abs {tuple(v_abs.shape)} / v_rel {tuple(v_rel.shape)} are not "
                         f"(1,1,{T},N) / (1,2,{T},N)")
    _read_in_place("gpgraph_sgcn_forward_graph", dev, {"v_abs": v_abs, "v_rel": v_rel})
    if n > L.SGCN_MAX_N:
        raise ValueError(f"gpgraph_sgcn_forward_graph: N = {n} exceeds the {L.SGCN_MAX_N} pedestrians a scene may have")
    out = torch.empty((1, S, k, n), device=dev)
    if n == 0:
        L.call("et_gpgraph_sgcn_forward_graph", C.byref(params), None, None, 0, None, None, None, None, None, None, 0,
               L.stream(dev))
        res = (out, torch.empty((0,), device=dev, dtype=torch.int64))
        return res + ({"dist": torch.empty((0, 0), device=dev), "n_groups": 0, "logit_s": [], "logit_t": []},) \
            if want_details else res
    ws, nbytes, gi, dist, ls, lt = _gpgraph_buffers(params, want_details, T, n, n * n, 1, dev)
    L.call("et_gpgraph_sgcn_forward_graph", C.byref(params), L.ptr(v_abs.detach()), L.ptr(v_rel.detach()), n, L.ptr(out),
           L.ptr(gi), L.ptr(dist), L.ptr(ls), L.ptr(lt), L.ptr(ws), nbytes, L.stream(dev))
    idx = gi.long()
    if not want_details:
        return out, idx
    g = int(idx.max()) + 1
    sizes = (n, g, n)
    det = {"dist": dist.view(n, n), "n_groups": g,
           "logit_s": [ls[4 * T * m * n * n:4 * T * (m * n * n + sizes[m] ** 2)].view(T, 4, sizes[m], sizes[m]) for m in range(3)],
           "logit_t": [lt[4 * T * T * m * n:4 * T * T * (m * n + sizes[m])].view(sizes[m], 4, T, T) for m in range(3)]}
    return out, idx, det


def gpgraph_sgcn_forward_scenes(model, C_obs, nrm, scene_sizes=None, want_details=False):
    """The gpgraphsgcn bridge + ``model`` (eval mode) + the post-hook for every scene of a split in a fixed number of
    launches (8 + the number of asymmetric convolution layers): C_obs, nrm and ``scene_sizes`` as
    :func:`stgcnn_forward_scenes` -> C_pred_refine (k, N, S).  One unlisted scene of more than 512 pedestrians raises
    ValueError; a listed one is not computed: its rows are NaN.  With ``want_details`` also a dict:
    ``group_index`` (N,) int32 scene-local, ``dist`` packed (scene s's (n, n) block at n_0^2 + ... + n_{s-1}^2), ``logit_s``
    / ``logit_t`` packed as include/eigentraj.h describes (pass m of scene s at 4 T (m sum_n2 + sum_{s'<s} n_s'^2) and at
    4 T T (m N + off[s]))."""
    model._check_mode()
    params, dev = model.et_params()
    b = _scene_batch("gpgraph_sgcn_forward_scenes", dev, C_obs, nrm, params.base.pred_len, scene_sizes)
    n = b.n
    if b.off is None and n > L.SGCN_MAX_N:
        raise ValueError(f"gpgraph_sgcn_forward_scenes: a scene of {n} pedestrians exceeds the {L.SGCN_MAX_N} a scene may have")
    # (a listed scene above the limit is not refused: its rows come back NaN, the other scenes are computed)
    sum_n2 = sum(s * s for s in b.sizes if s <= L.SGCN_MAX_N)
    out = torch.empty((params.base.pred_len, n, params.base.out_dims), device=dev)
    if n == 0:
        L.call("et_gpgraph_sgcn_forward_scenes", C.byref(params), None, None, 0, L.ptr(b.off), b.n_scenes, 0, 0, None, None,
               None, None, None, None, 0, L.stream(dev))
        return (out, {"group_index": torch.empty((0,), device=dev, dtype=torch.int32)}) if want_details else out
    ws, nbytes, gi, dist, ls, lt = _gpgraph_buffers(params, want_details, params.base.obs_len, n, sum_n2, len(b.sizes), dev)
    L.call("et_gpgraph_sgcn_forward_scenes", C.byref(params), L.ptr(b.C_obs), L.ptr(b.nrm), n, L.ptr(b.off), b.n_scenes,
           sum_n2, b.max_n, L.ptr(out), L.ptr(gi), L.ptr(dist), L.ptr(ls), L.ptr(lt), L.ptr(ws), nbytes, L.stream(dev))
    if want_details:
        return out, {"group_index": gi, "dist": dist, "logit_s": ls, "logit_t": lt}
    return out


# ------------------------------------------------------------------------ GP-Graph-SGCN predictor (training)
def gpgraph_sgcn_train_workspace(model, n, sum_n2=None, n_scenes=1, et_params=None):
    """A training workspace for ``n`` pedestrians in ``n_scenes`` scenes whose squared sizes sum to ``sum_n2`` (one scene:
    n * n): :func:`gpgraph_sgcn_train_forward_graph` / ``_scenes`` fill it, :func:`gpgraph_sgcn_backward_graph` / ``_scenes``
    read it."""
    return _train_workspace("gpgraph_sgcn", model, et_params, n, n * n if sum_n2 is None else sum_n2, n_scenes)


def _gpgraph_details(want, T, n, sum_n2, dev):
    gi = torch.empty((n,), device=dev, dtype=torch.int32)
    if not want:
        return gi, None, None, None
    return (gi, torch.empty((sum_n2,), device=dev), torch.empty((3 * 4 * T * sum_n2,), device=dev),
            torch.empty((3 * n * 4 * T * T,), device=dev))


def gpgraph_sgcn_train_forward_graph(model, v_abs, v_rel, workspace, want_details=False, et_params=None):
    """:func:`gpgraph_sgcn_forward_graph` with the kept layout (the same kernels; ``v`` and ``indices`` are bit-equal): what the
    backward pass reads stays in ``workspace`` (of :func:`gpgraph_sgcn_train_workspace`) for
    :func:`gpgraph_sgcn_backward_graph`."""
    who = "gpgraph_sgcn_train_forward_graph"
    params, dev = _train_params(who, model, et_params)
    T, k, S = params.base.obs_len, params.base.pred_len, params.base.out_dims
    n = v_abs.shape[3] if v_abs.dim() == 4 else -1
    if tuple(v_abs.shape) != (1, 1, T, n) or tuple(v_rel.shape) != (1, 2, T, n) or n < 1:
        raise ValueError(f"{who}: v_abs {tuple(v_abs.shape)} / v_rel {tuple(v_rel.shape)} are not (1,1,{T},N) / (1,2,{T},N), "
                         "N >= 1")
    _read_in_place(who, dev, {"v_abs": v_abs, "v_rel": v_rel})
    if n > L.SGCN_MAX_N:
        raise ValueError(f"{who}: N = {n} exceeds the {L.SGCN_MAX_N} pedestrians a scene may have")
    _check_train_ws(who, dev, workspace, "gpgraph_sgcn_train_workspace")
    out = torch.empty((1, S, k, n), device=dev)
    gi, dist, ls, lt = _gpgraph_details(want_details, T, n, n * n, dev)
    L.call("et_gpgraph_sgcn_train_forward_graph", C.byref(params), L.ptr(v_abs.detach()), L.ptr(v_rel.detach()), n, L.ptr(out),
           L.ptr(gi), L.ptr(dist), L.ptr(ls), L.ptr(lt), L.ptr(workspace), workspace.numel(), L.stream(dev))
    idx = gi.long()
    if not want_details:
        return out, idx
    g = int(idx.max()) + 1
    sizes = (n, g, n)
    det = {"dist": dist.view(n, n), "n_groups": g,
           "logit_s": [ls[4 * T * m * n * n:4 * T * (m * n * n + sizes[m] ** 2)].view(T, 4, sizes[m], sizes[m]) for m in range(3)],
           "logit_t": [lt[4 * T * T * m * n:4 * T * T * (m * n + sizes[m])].view(sizes[m], 4, T, T) for m in range(3)]}
    return out, idx, det


def gpgraph_sgcn_train_forward_scenes(model, C_obs, nrm, scene_sizes=None, want_details=False, workspace=None):
    """:func:`gpgraph_sgcn_forward_scenes` with the kept layout -> (C_pred_refine (k, N, S)[, details], workspace); the
    workspace (made here unless given) goes to :func:`gpgraph_sgcn_backward_scenes` with the same ``scene_sizes``."""
    who = "gpgraph_sgcn_train_forward_scenes"
    params, dev = _train_params(who, model, None)
    b = _scene_batch(who, dev, C_obs, nrm, params.base.pred_len, scene_sizes)
    n = b.n
    if b.off is None and n > L.SGCN_MAX_N:
        raise ValueError(f"{who}: a scene of {n} pedestrians exceeds the {L.SGCN_MAX_N} a scene may have")
    sum_n2 = sum(s * s for s in b.sizes if s <= L.SGCN_MAX_N)
    out = torch.empty((params.base.pred_len, n, params.base.out_dims), device=dev)
    if workspace is None:
        workspace = gpgraph_sgcn_train_workspace(model, n, sum_n2, len(b.sizes), et_params=(params, dev))
    if n:
        _check_train_ws(who, dev, workspace, "gpgraph_sgcn_train_workspace")
    gi, dist, ls, lt = _gpgraph_details(want_details, params.base.obs_len, n, sum_n2, dev)
    L.call("et_gpgraph_sgcn_train_forward_scenes", C.byref(params), L.ptr(b.C_obs), L.ptr(b.nrm), n, L.ptr(b.off), b.n_scenes,
           sum_n2, b.max_n, L.ptr(out), L.ptr(gi), L.ptr(dist), L.ptr(ls), L.ptr(lt), L.ptr(workspace), _numel(workspace),
           L.stream(dev))
    if want_details:
        return out, {"group_index": gi, "dist": dist, "logit_s": ls, "logit_t": lt}, workspace
    return out, workspace


def gpgraph_sgcn_grad_views(model, grads):
    """``grads``, the flat buffer of :func:`gpgraph_sgcn_backward_graph` / ``_scenes`` -> {state_dict key: a view of it shaped
    like the parameter}, every parameter of the whole ``GPGraph`` (state_dict order: ``baseline_model.*``, ``group_gen.th``,
    ``group_gen.group_cnn.0.*``, ``group_mix.st_gcns_mix.{0,1}.*``)."""
    return _grad_views("gpgraph_sgcn_grad_views", model, grads)


def gpgraph_sgcn_backward_graph(model, workspace, d_out, et_params=None):
    """The backward pass of :func:`gpgraph_sgcn_train_forward_graph` in ``number_asymmetric_conv_layer + 13`` launches:
    ``workspace`` as that call filled it (same weights), ``d_out`` (1, S, k, N) the gradient at its output -> the flat float32
    gradient buffer (:func:`gpgraph_sgcn_grad_views` names its parts)."""
    who = "gpgraph_sgcn_backward_graph"
    params, dev = _train_params(who, model, et_params)
    n = d_out.shape[3] if d_out.dim() == 4 else -1
    _check_train_ws(who, dev, workspace, "gpgraph_sgcn_train_workspace")
    d_out, grads = _backward_args(who, "et_gpgraph_sgcn_grad_floats", params, dev, d_out,
                                  (1, params.base.out_dims, params.base.pred_len, n))
    L.call("et_gpgraph_sgcn_backward_graph", C.byref(params), n, L.ptr(d_out), L.ptr(grads), grads.numel(), L.ptr(workspace),
           workspace.numel(), L.stream(dev))
    return grads


def gpgraph_sgcn_backward_scenes(model, workspace, d_out, scene_sizes=None):
    """The backward pass of :func:`gpgraph_sgcn_train_forward_scenes`, the same number of launches whatever the number of
    scenes: ``workspace`` as that call filled it, ``scene_sizes`` as given to it, ``d_out`` (k, N, S) -> the flat gradient
    buffer, summed over the scenes in ascending order."""
    return _backward_scenes("gpgraph_sgcn", model, workspace, d_out, scene_sizes,
                            lambda p: (p.base.pred_len, p.base.out_dims), packed=True, cap=L.SGCN_MAX_N)


def gpgraph_sgcn_train_views(model, workspace, n, sum_n2=None, n_scenes=1, lo=0, sq=0, scene_n=None, scene=0):
    """The values kept in ``workspace`` by name, as views, for scene number ``scene`` of ``scene_n`` pedestrians that starts at
    row ``lo`` and at ``sq`` in the packed n^2 stacks (one scene: the defaults).  ``n_groups``; ``passes`` [3]: per pass (0
    pedestrian graph, 1 group means, 2 intra-group, n_m = n, G, n) the names of :func:`sgcn_train_views` and ``vp`` (T, n_m)
    (the position channel; ``v`` is the coefficient channel), ``out`` (k, n_m, S), and after a backward call ``d_out`` (the
    base's upstream gradient), ``d_ax`` (T, 4, n_m), ``srec`` (T, 4, n_m, 2), ``trec`` (n_m, 4, T, 3), ``d_acc_t`` (n_m, 4, T),
    ``dx_as`` (n_m, 4, T), ``dx`` (2, T, n_m) (passes 1 and 2).  The wrapper's: ``v_abs`` (T, n), ``f`` (8, T, n), ``dist``,
    ``sig``, ``sn`` (sig / colsum) (n, n), ``colsum`` (n,), ``group_index`` (n,), ``group_size`` (G,), and after a backward call
    ``d_o`` [3] x (k, n, S) (d o_m per pedestrian), ``d_vp`` (2, T, n), ``d_P``, ``d_sig``, ``d_d`` (n, n), ``d_f`` (8, T, n).  The
    offsets are the library's (``et_gpgraph_sgcn_train_layout``)."""
    params, _ = model.et_params()
    bp = params.base
    T, k, S, na, nt = bp.obs_len, bp.pred_len, bp.out_dims, bp.n_asym, bp.n_tcn
    N, n2 = n, n * n if sum_n2 is None else sum_n2
    m0 = N if scene_n is None else scene_n
    f = workspace.view(torch.float32)
    i32 = workspace.view(torch.int32)
    lay = _layout("et_gpgraph_sgcn_train_layout", L.GPGRAPH_SGCN_TRAIN_LAYOUT_NAMES, params, N, n2, n_scenes)
    sl = lambda off, cnt, *shape: f[off:off + cnt].view(*shape)
    G = int(i32[lay.vn + n_scenes + scene])
    passes = []
    for p_, m in enumerate((m0, G, m0)):
        r0, q0 = p_ * N + lo, p_ * n2 + sq     # the virtual scene's first row and packed offset
        rows = lambda off: sl(off + r0 * 4 * T * T, m * 4 * T * T, m, 4, T, T)
        feat = lambda off, *shape: sl(off + r0 * 4 * T * 16, m * 4 * T * 16, *shape)
        dense = lambda off: sl(off + 4 * T * q0, 4 * T * m * m, T, 4, m, m)
        keep = sl(lay.keep + r0 * lay.keep_stride, m * lay.keep_stride, m, 2 * T + 2 * nt * k, 64)
        po = lambda off: f[off:off + k * 3 * N * S].view(k, 3 * N, S)[:, r0:r0 + m]
        passes.append({
            "v": sl(lay.v + T * r0, T * m, T, m), "vp": sl(lay.vp + T * r0, T * m, T, m),
            "stack_s": [dense(lay.stack_s + j * lay.stack_s_stride) for j in range(na + 1)],
            "stack_t": [rows(lay.stack_t + j * lay.stack_t_stride) for j in range(na + 1)],
            "rows_s": sl(lay.rows_s + 2 * T * 4 * r0, 2 * T * 4 * m, T, 4, m, 2),
            "rows_t": sl(lay.rows_t + 2 * T * 4 * r0, 2 * T * 4 * m, m, 4, T, 2),
            "at": rows(lay.at), "f1": feat(lay.f1, T, 4, m, 16), "f2": feat(lay.f2, m, 4, T, 16), "ts": feat(lay.ts, m, 4, T, 16),
            "st_pre": keep[:, :T], "rep": keep[:, T:2 * T],
            "tcn_pre": [keep[:, 2 * T + 2 * j * k:2 * T + (2 * j + 1) * k] for j in range(nt)],
            "tcn_out": [keep[:, 2 * T + (2 * j + 1) * k:2 * T + (2 * j + 2) * k] for j in range(nt)],
            "out": po(lay.po), "d_out": po(lay.dpo),
            "d_ts": feat(lay.d_ts, m, 4, T, 16), "d_f2": feat(lay.d_f2, m, 4, T, 16), "d_f1": feat(lay.d_f1, T, 4, m, 16),
            "d_at": rows(lay.d_at), "d_accn": sl(lay.rrec + 4 * T * r0 * 17, 4 * T * m * 17, T, 4, m, 17)[..., 1:],
            "g_s": [dense(lay.g_s + j * lay.stack_s_stride) for j in range(na + 1)],
            "g_t": [rows(lay.g_t + j * lay.stack_t_stride) for j in range(na + 1)],
            "dir_s": dense(lay.dir_s), "dir_t": rows(lay.dir_t), "dd_s": dense(lay.dd_s),
            "d_ax": sl(lay.dax + 4 * T * r0, 4 * T * m, T, 4, m), "srec": sl(lay.srec + 8 * T * r0, 8 * T * m, T, 4, m, 2),
            "trec": sl(lay.trec + 12 * T * r0, 12 * T * m, m, 4, T, 3), "d_acc_t": sl(lay.dacct + 4 * T * r0, 4 * T * m, m, 4, T),
            "dx_as": sl(lay.dxas + 4 * T * r0, 4 * T * m, m, 4, T),
            "dx": torch.stack([sl(lay.dxp + T * r0, T * m, T, m), sl(lay.dxv + T * r0, T * m, T, m)]),
        })
    m = m0
    dmix = f[lay.dmix:lay.dmix + k * 3 * N * S].view(k, 3 * N, S)
    return {
        "n_groups": G, "passes": passes,
        "v_abs": sl(lay.va + T * lo, T * m, T, m), "f": sl(lay.feat + 8 * T * lo, 8 * T * m, 8, T, m),
        "dist": sl(lay.dist + sq, m * m, m, m), "sn": sl(lay.sn + sq, m * m, m, m), "sig": sl(lay.sig + sq, m * m, m, m),
        "colsum": sl(lay.cs + lo, m, m), "group_index": i32[lay.gidx + lo:lay.gidx + lo + m],
        "group_size": i32[lay.cnt + lo:lay.cnt + lo + G],
        "d_o": [dmix[:, p_ * N + lo:p_ * N + lo + m] for p_ in range(3)],
        "d_vp": sl(lay.dvp + 2 * T * lo, 2 * T * m, 2, T, m), "d_P": sl(lay.dP + sq, m * m, m, m),
        "d_sig": sl(lay.dsig + sq, m * m, m, m), "d_d": sl(lay.dd + sq, m * m, m, m),
        "d_f": sl(lay.df + 8 * T * lo, 8 * T * m, 8, T, m),
    }


# ---------------------------------------------------------------------- GP-Graph-STGCNN predictor (inference)
def _gpgraph_stgcnn_buffers(params, want, T, n, sum_n2, n_scenes, dev):
    ws, nbytes = _workspace("et_gpgraph_stgcnn_workspace_bytes", dev, params, n, sum_n2, n_scenes, required=True)
    gi = torch.empty((n,), device=dev, dtype=torch.int32)
    if not want:
        return ws, nbytes, gi, None, None
    return ws, nbytes, gi, torch.empty((sum_n2,), device=dev), torch.zeros((3, T * n), device=dev)


def _stgcnn_base_of(model, who):
    from .stgcnn import SocialSTGCNN
    if not isinstance(getattr(model, "baseline_model", None), SocialSTGCNN):
        raise NotImplementedError(f"{who}: the model is not a GPGraph around a SocialSTGCNN base (a GPGraph around SGCN runs "
                                  "through gpgraph_sgcn_forward_*)")


def gpgraph_stgcnn_forward_graph(model, v_abs, v_rel, want_details=False):
    """``model`` (:class:`eigentrajectory_amd.gpgraph.GPGraph` around a per-time-row SocialSTGCNN, eval mode) on one scene as
    the gpgraphstgcnn bridge hands it over: v_abs (1, 1, T, N), v_rel (1, 1, T, N) -> ``(v (1, S, k, N), indices (N,)
    int64)``; with ``want_details`` a dict is returned as third item: ``dist`` (N, N), ``group_index`` (N,) int32,
    ``n_groups``, and ``graph_inputs``, the three passes' inputs as the kernel reads them: [(T, N), (T, G), (T, N)].  The
    inputs must be contiguous float32 tensors on the model's device (they are read in place).  Three launches."""
    _stgcnn_base_of(model, "gpgraph_stgcnn_forward_graph")
    model._check_mode()
    params, dev = model.et_params()
    T, k, S = params.base.seq_len, params.base.pred_seq_len, params.base.output_feat
    n = v_abs.shape[3] if v_abs.dim() == 4 else -1
    if tuple(v_abs.shape) != (1, 1, T, n) or tuple(v_rel.shape) != (1, 1, T, n):
        raise ValueError(f"gpgraph_stgcnn_forward_graph: v_abs {tuple(v_abs.shape)} / v_rel {tuple(v_rel.shape)} are not "
                         f"(1,1,{T},N) / (1,1,{T},N)")
    _read_in_place("gpgraph_stgcnn_forward_graph", dev, {"v_abs": v_abs, "v_rel": v_rel})
    if n > L.SGCN_MAX_N:
        raise ValueError(f"gpgraph_stgcnn_forward_graph: N = {n} exceeds the {L.SGCN_MAX_N} pedestrians a scene may have")
    out = torch.empty((1, S, k, n), device=dev)
    if n == 0:
        L.call("et_gpgraph_stgcnn_forward_graph", C.byref(params), None, None, 0, None, None, None, None, None, 0,
               L.stream(dev))
        res = (out, torch.empty((0,), device=dev, dtype=torch.int64))
        return res + ({"dist": torch.empty((0, 0), device=dev), "n_groups": 0, "graph_inputs": [],
                       "group_index": torch.empty((0,), device=dev, dtype=torch.int32)},) if want_details else res
    ws, nbytes, gi, dist, gin = _gpgraph_stgcnn_buffers(params, want_details, T, n, n * n, 1, dev)
    L.call("et_gpgraph_stgcnn_forward_graph", C.byref(params), L.ptr(v_abs.detach()), L.ptr(v_rel.detach()), n, L.ptr(out),
           L.ptr(gi), L.ptr(dist), L.ptr(gin), L.ptr(ws), nbytes, L.stream(dev))
    idx = gi.long()
    if not want_details:
        return out, idx
    g = int(idx.max()) + 1
    return out, idx, {"dist": dist.view(n, n), "group_index": gi, "n_groups": g,
                      "graph_inputs": [gin[m, :T * nm].view(T, nm) for m, nm in enumerate((n, g, n))]}


def gpgraph_stgcnn_forward_scenes(model, C_obs, nrm, scene_sizes=None, want_details=False):
    """The gpgraphstgcnn bridge + ``model`` (eval mode) + the post-hook for every scene of a split in three launches: C_obs,
    nrm, ``scene_sizes`` and the scene limit as :func:`gpgraph_sgcn_forward_scenes` -> C_pred_refine (k, N, S).
    With ``want_details`` also a dict: ``group_index`` (N,) int32 scene-local, ``dist`` packed (scene s's (n, n) block at
    n_0^2 + ... + n_{s-1}^2), ``n_groups`` (per scene, int64) and ``graph_inputs`` (3, T N) as include/eigentraj.h describes
    (pass m of scene s a (T, n_m) block at T (m N + off[s]))."""
    _stgcnn_base_of(model, "gpgraph_stgcnn_forward_scenes")
    model._check_mode()
    params, dev = model.et_params()
    b = _scene_batch("gpgraph_stgcnn_forward_scenes", dev, C_obs, nrm, params.base.pred_seq_len, scene_sizes)
    n, sizes = b.n, b.sizes
    if b.off is None and n > L.SGCN_MAX_N:
        raise ValueError(f"gpgraph_stgcnn_forward_scenes: a scene of {n} pedestrians exceeds the {L.SGCN_MAX_N} a scene may "
                         "have")
    # (a listed scene above the limit is not refused: its rows come back NaN, the other scenes are computed)
    sum_n2 = sum(s * s for s in sizes if s <= L.SGCN_MAX_N)
    out = torch.empty((params.base.pred_seq_len, n, params.base.output_feat), device=dev)
    if n == 0:
        L.call("et_gpgraph_stgcnn_forward_scenes", C.byref(params), None, None, 0, L.ptr(b.off), b.n_scenes, 0, 0, None, None,
               None, None, None, 0, L.stream(dev))
        empty = {"group_index": torch.empty((0,), device=dev, dtype=torch.int32), "dist": torch.empty((0,), device=dev),
                 "graph_inputs": torch.empty((3, 0), device=dev), "n_groups": torch.zeros((len(sizes),), dtype=torch.int64)}
        return (out, empty) if want_details else out
    ws, nbytes, gi, dist, gin = _gpgraph_stgcnn_buffers(params, want_details, params.base.seq_len, n, sum_n2, len(sizes), dev)
    L.call("et_gpgraph_stgcnn_forward_scenes", C.byref(params), L.ptr(b.C_obs), L.ptr(b.nrm), n, L.ptr(b.off), b.n_scenes,
           sum_n2, b.max_n, L.ptr(out), L.ptr(gi), L.ptr(dist), L.ptr(gin), L.ptr(ws), nbytes, L.stream(dev))
    if want_details:
        lo, groups = 0, []
        host = gi.cpu()
        for s_ in sizes:
            groups.append(int(host[lo:lo + s_].max()) + 1 if 0 < s_ <= L.SGCN_MAX_N else 0)
            lo += s_
        return out, {"group_index": gi, "dist": dist, "graph_inputs": gin,
                     "n_groups": torch.tensor(groups, dtype=torch.int64)}
    return out


# ------------------------------------------------------------------------------ DMRGCN predictor (inference)
def dmrgcn_forward_graph(model, v, a):
    """``model`` (:class:`eigentrajectory_amd.dmrgcn.SocialDMRGCN`, eval mode) on one scene as the dmrgcn bridge hands it
    over: v (1, 1, K, N), a (1, 2, K, N, N) = [A_disp, A_dist], read as given -> the raw output (1, S, k, N).  One launch."""
    params, dev = model.et_params()
    K, k, S = params.seq_len, params.pred_seq_len, params.output_feat
    n = v.shape[-1]
    if tuple(v.shape) != (1, 1, K, n) or tuple(a.shape) != (1, 2, K, n, n):
        raise ValueError(f"dmrgcn_forward_graph: v {tuple(v.shape)} / a {tuple(a.shape)} are not (1,1,{K},N) / (1,2,{K},N,N)")
    v, a = _dev_args(dev, v, a)
    out = torch.empty((1, S, k, n), device=dev)
    ws, nbytes = _workspace("et_dmrgcn_workspace_bytes", dev, params, n, n)
    L.call("et_dmrgcn_forward_graph", C.byref(params), L.ptr(v), L.ptr(a), n, L.ptr(out), L.ptr(ws), nbytes, L.stream(dev))
    return out


def dmrgcn_forward_scenes(model, C_obs, nrm, scene_sizes=None, want_details=False):
    """The dmrgcn bridge + ``model`` (eval mode) + the post-hook for every scene of a split in ONE launch: C_obs, nrm and
    ``scene_sizes`` as :func:`stgcnn_forward_scenes` -> C_pred_refine (k, N, S).  With ``want_details`` also a dict:
    ``graph_inputs`` (K, N), the fp32 v = [C_obs; obs_ori] the kernel used."""
    params, dev = model.et_params()
    b = _scene_batch("dmrgcn_forward_scenes", dev, C_obs, nrm, params.pred_seq_len, scene_sizes)
    out = torch.empty((params.pred_seq_len, b.n, params.output_feat), device=dev)
    gin = torch.empty((params.seq_len, b.n), device=dev) if want_details else None
    ws, nbytes = _workspace("et_dmrgcn_workspace_bytes", dev, params, b.n, b.max_n)
    L.call("et_dmrgcn_forward_scenes", C.byref(params), L.ptr(b.C_obs), L.ptr(b.nrm), b.n, L.ptr(b.off), b.n_scenes,
           L.ptr(out), L.ptr(gin), L.ptr(ws), nbytes, L.stream(dev))
    return (out, {"graph_inputs": gin}) if want_details else out


# ------------------------------------------------------------------------------ DMRGCN predictor (training)
def dmrgcn_train_workspace(model, n, n_scenes=1, et_params=None):
    """A training workspace for ``n`` pedestrians in ``n_scenes`` scenes: :func:`dmrgcn_train_forward_graph` / ``_scenes``
    fill it, :func:`dmrgcn_backward_graph` / ``_scenes`` read it (None for ``n`` = 0)."""
    return _train_workspace("dmrgcn", model, et_params, n, max(n_scenes, 1))


def dmrgcn_train_forward_graph(model, v, a, workspace, keep=None, et_params=None):
    """``model`` in training mode on one scene as the dmrgcn bridge hands it over: v (1, 1, K, N), a (1, 2, K, N, N),
    ``keep`` uint8 (2, 5, K, N, N) indexed [r, b, t, w, v] (:meth:`SocialDMRGCN.draw_keep`; None keeps every edge) -> the
    raw output (1, S, k, N).  What the backward reads stays in ``workspace`` (of :func:`dmrgcn_train_workspace`) for
    :func:`dmrgcn_backward_graph`.  One launch."""
    params, dev = _train_params("dmrgcn_train_forward_graph", model, et_params)
    K, k, S = params.seq_len, params.pred_seq_len, params.output_feat
    n = v.shape[-1]
    if tuple(v.shape) != (1, 1, K, n) or tuple(a.shape) != (1, 2, K, n, n):
        raise ValueError(f"dmrgcn_train_forward_graph: v {tuple(v.shape)} / a {tuple(a.shape)} are not (1,1,{K},N) / "
                         f"(1,2,{K},N,N)")
    if n > L.DMRGCN_TRAIN_MAX_N:
        raise ValueError(f"dmrgcn_train_forward_graph: N = {n} exceeds the {L.DMRGCN_TRAIN_MAX_N} pedestrians a training scene "
                         "may have")
    v, a = _dev_args(dev, v.detach(), a.detach())
    keep = _keep_mask("dmrgcn_train_forward_graph", dev, keep, shape=(2, L.DMRGCN_BINS, K, n, n))
    out = torch.empty((1, S, k, n), device=dev)
    if n:
        _check_train_ws("dmrgcn_train_forward_graph", dev, workspace, "dmrgcn_train_workspace")
    L.call("et_dmrgcn_train_forward_graph", C.byref(params), L.ptr(v), L.ptr(a), n, L.ptr(keep), L.ptr(out),
           L.ptr(workspace), _numel(workspace), L.stream(dev))
    return out


def dmrgcn_keep_offsets(scene_sizes, device=None):
    """-> (int64 tensor (n_scenes + 1,): where each scene's (2, 5, K, n, n) block of a packed keep mask starts, in units of
    10 K entries (the running sum of n^2; a scene above the training cap takes no room), the total sum of n^2)"""
    return _keep_offsets(scene_sizes, L.DMRGCN_TRAIN_MAX_N, device)


def dmrgcn_train_forward_scenes(model, C_obs, nrm, scene_sizes=None, keep=None, workspace=None):
    """The dmrgcn bridge + ``model`` in training mode + the post-hook for every scene of a batch in ONE launch, one
    workgroup per scene.  C_obs, nrm and ``scene_sizes`` as :func:`dmrgcn_forward_scenes`; ``keep``: uint8, every scene's
    (2, 5, K, n, n) block one after the other (:func:`dmrgcn_keep_offsets`), None keeps every edge -> (C_pred_refine
    (k, N, S), workspace); the workspace (made here unless given) goes to :func:`dmrgcn_backward_scenes` with the same
    ``scene_sizes``.  A scene of more than 512 pedestrians is not computed (NaN rows)."""
    params, dev = _train_params("dmrgcn_train_forward_scenes", model, None)
    b = _scene_batch("dmrgcn_train_forward_scenes", dev, C_obs, nrm, params.pred_seq_len, scene_sizes)
    if scene_sizes is None and b.n > L.DMRGCN_TRAIN_MAX_N:
        raise ValueError(f"dmrgcn_train_forward_scenes: one unlisted scene of {b.n} pedestrians exceeds the "
                         f"{L.DMRGCN_TRAIN_MAX_N} a training scene may have")
    if workspace is None:
        workspace = dmrgcn_train_workspace(model, b.n, len(b.sizes), et_params=(params, dev))
    if b.n:
        _check_train_ws("dmrgcn_train_forward_scenes", dev, workspace, "dmrgcn_train_workspace")
    koff, total = dmrgcn_keep_offsets(b.sizes, dev if keep is not None else None)
    keep = _keep_mask("dmrgcn_train_forward_scenes", dev, keep, numel=2 * L.DMRGCN_BINS * params.seq_len * total)
    out = torch.empty((params.pred_seq_len, b.n, params.output_feat), device=dev)
    L.call("et_dmrgcn_train_forward_scenes", C.byref(params), L.ptr(b.C_obs), L.ptr(b.nrm), b.n, L.ptr(b.off), b.n_scenes,
           L.ptr(keep), L.ptr(koff if keep is not None else None), L.ptr(out), L.ptr(workspace), _numel(workspace),
           L.stream(dev))
    return out, workspace


def dmrgcn_grad_views(model, grads):
    """``grads``, the flat buffer of :func:`dmrgcn_backward_graph` / ``_scenes`` -> {state_dict key: a view of it shaped like
    the parameter}, every parameter of ``model`` (state_dict order)."""
    return _grad_views("dmrgcn_grad_views", model, grads)


def dmrgcn_backward_graph(model, workspace, d_out, et_params=None):
    """The backward pass of :func:`dmrgcn_train_forward_graph` in three launches: ``workspace`` as that call filled it (same
    weights), ``d_out`` (1, S, k, N) the gradient at its output -> the flat float32 gradient buffer
    (:func:`dmrgcn_grad_views` names its parts)."""
    return _backward_graph("dmrgcn", model, workspace, d_out, et_params, -1,
                           lambda p, n: (1, p.output_feat, p.pred_seq_len, n))


def dmrgcn_backward_scenes(model, workspace, d_out, scene_sizes=None):
    """The backward pass of :func:`dmrgcn_train_forward_scenes` in three launches whatever the number of scenes:
    ``workspace`` as that call filled it, ``scene_sizes`` as given to it, ``d_out`` (k, N, S) -> the flat gradient buffer,
    summed over the scenes in ascending order."""
    return _backward_scenes("dmrgcn", model, workspace, d_out, scene_sizes, lambda p: (p.pred_seq_len, p.output_feat))


def dmrgcn_train_views(model, workspace, n, n_scenes=1, lo=0, scene=0, scene_n=None):
    """The values kept in ``workspace`` by name, as views, for scene number ``scene`` of ``scene_n`` pedestrians that starts
    at row ``lo`` (one scene: the defaults).  Forward: ``u`` (K, n), ``P`` (2, 5, 2, K, n) (the contraction rows: j = 0 from
    u, j = 1 from the ones row), ``yp`` (S, K, n) the tcn PReLU's input, ``s`` (S, K, n) the block PReLU's input, ``x``
    (K, S, n) the block's output, and per tpcnn block the lists ``c0`` / ``y`` / ``c1`` / ``q`` / ``o`` (k, S, n) and ``z``
    (S, n).  After a backward call also ``d_q`` / ``d_y`` (k, S, n) and ``d_g`` (S, n) per block, ``d_x`` (K, S, n),
    ``d_yt`` (S, K, n) the gradient at PReLU(yp), and ``partial``, the scene's own flat gradient.  The offsets are the
    library's (``et_dmrgcn_train_layout``)."""
    params, _ = model.et_params()
    K, k, S = params.seq_len, params.pred_seq_len, params.output_feat
    m = n if scene_n is None else scene_n
    f = workspace.view(torch.float32)
    lay = _layout("et_dmrgcn_train_layout", L.DMRGCN_TRAIN_LAYOUT_NAMES, params, n, n_scenes)
    base = lo * lay.per
    fld = lambda off, *shape: f[base + off * m:base + off * m + math.prod(shape) * m].view(*shape, m)
    kS = k * S
    views = {"u": fld(lay.u, K), "P": fld(lay.P, 2, L.DMRGCN_BINS, 2, K), "yp": fld(lay.yp, S, K), "s": fld(lay.s, S, K),
             "x": fld(lay.x, K, S), "d_x": fld(lay.dx, K, S), "d_yt": fld(lay.dy, S, K)}
    blocks = range(params.n_tpcnn)
    for q, name in enumerate(("c0", "y", "c1", "q", "o")):
        views[name] = [fld(lay.tp + j * lay.tp_stride + q * kS, k, S) for j in blocks]
    views["z"] = [fld(lay.tp + j * lay.tp_stride + 5 * kS, S) for j in blocks]
    views["d_q"] = [fld(lay.dtp + j * lay.dtp_stride, k, S) for j in blocks]
    views["d_y"] = [fld(lay.dtp + j * lay.dtp_stride + kS, k, S) for j in blocks]
    views["d_g"] = [fld(lay.dtp + j * lay.dtp_stride + 2 * kS, S) for j in blocks]
    views["partial"] = f[lay.partials + scene * lay.grads:lay.partials + (scene + 1) * lay.grads]
    return views


# ------------------------------------------------------------------------------ Social-Implicit predictor (inference)
def implicit_workspace(model, n, et_params=None):
    """A caller-owned workspace for ``n`` pedestrians: pass it as ``workspace=`` to :func:`implicit_forward_graph` /
    :func:`implicit_forward_scenes`, which fill it with the neighbour table (the scenes form also with every scene's v), and
    then to :func:`implicit_backward_graph` / :func:`implicit_backward_scenes` (None for ``n`` = 0).  ``et_params``, here
    and in the graph-form calls: what ``model.et_params()`` returned, for a caller that makes several of these calls on
    unchanged tensors and bins (the training Function) and builds the pointer table once."""
    params, dev = et_params or model.et_params()
    return _workspace("et_implicit_workspace_bytes", dev, params, n)[0]


def _implicit_workspace(who, dev, params, n, workspace):
    """the call's own workspace, or the caller's after a look at it -> (tensor | None, its size in bytes)"""
    if workspace is None:
        return _workspace("et_implicit_workspace_bytes", dev, params, n)
    need = L.lib().et_implicit_workspace_bytes(C.byref(params), n)
    if workspace.device != dev or workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need:
        raise ValueError(f"{who}: workspace is not a contiguous uint8 tensor of at least {need} bytes on {dev} "
                         "(implicit_workspace makes one)")
    return workspace, workspace.numel()


def implicit_forward_graph(model, v, workspace=None, et_params=None):
    """``model`` (:class:`eigentrajectory_amd.implicit.SocialImplicitLight`) on one scene as the implicit bridge hands it
    over: v (1, 1, T, N) -> the raw output (1, S, T_out, N).  Two launches.  ``workspace`` (of :func:`implicit_workspace`):
    the neighbour table is left in it for :func:`implicit_backward_graph`."""
    params, dev = et_params or model.et_params()
    T, To, S = params.temporal_input, params.temporal_output, params.spatial_output
    if v.dim() != 4 or tuple(v.shape[:3]) != (1, 1, T):
        raise ValueError(f"implicit_forward_graph: v {tuple(v.shape)} is not (1,1,{T},N)")
    n = v.shape[-1]
    (v,) = _dev_args(dev, v)
    out = torch.empty((1, S, To, n), device=dev)
    ws, nbytes = _implicit_workspace("implicit_forward_graph", dev, params, n, workspace)
    L.call("et_implicit_forward_graph", C.byref(params), L.ptr(v), n, L.ptr(out), L.ptr(ws), nbytes, L.stream(dev))
    return out


def implicit_forward_scenes(model, C_obs, nrm, scene_sizes=None, want_details=False, workspace=None):
    """The implicit bridge + ``model`` + the post-hook for every scene of a split in TWO launches: C_obs, nrm and
    ``scene_sizes`` as :func:`stgcnn_forward_scenes`, k = temporal_input - 2 -> C_pred_refine (T_out, N, S).  With
    ``want_details`` also a dict: ``graph_inputs`` (k + 2, N), the fp32 v = [C_obs; obs_ori] the kernel used, and ``zone``
    (N,) int32, every pedestrian's Social-Zone.  ``workspace`` (of :func:`implicit_workspace`): the neighbour table and
    every scene's v are left in it for :func:`implicit_backward_scenes`."""
    params, dev = model.et_params()
    b = _scene_batch("implicit_forward_scenes", dev, C_obs, nrm, params.temporal_input - 2, scene_sizes)
    n = b.n
    out = torch.empty((params.temporal_output, n, params.spatial_output), device=dev)
    gin = torch.empty((params.temporal_input, n), device=dev) if want_details else None
    zone = torch.empty((n,), device=dev, dtype=torch.int32) if want_details else None
    ws, nbytes = _implicit_workspace("implicit_forward_scenes", dev, params, n, workspace)
    L.call("et_implicit_forward_scenes", C.byref(params), L.ptr(b.C_obs), L.ptr(b.nrm), n, L.ptr(b.off), b.n_scenes,
           L.ptr(out), L.ptr(gin), L.ptr(zone), L.ptr(ws), nbytes, L.stream(dev))
    return (out, {"graph_inputs": gin, "zone": zone}) if want_details else out


# ------------------------------------------------------------------------------ Social-Implicit predictor (training)
def implicit_grad_size(params):
    """floats of one cell's gradient block (csrc/et_implicit.hip: im_layout().size; noise_w is not in it)"""
    S, T, To = params.spatial_output, params.temporal_input, params.temporal_output
    return 18 * S + 14 * To * T + 4 * To + 2


def implicit_grad_views(model, grads):
    """``grads`` (n_bins, G) of :func:`implicit_backward_graph` -> {state_dict key: a view of it shaped like the
    parameter}, the 18 tensors of every cell the forward reads (``noise_w`` is not among them)."""
    out = {}
    for i, cell in enumerate(model.implicit_cells):
        at = 0
        for prefix, mod in (("", cell), ("ped.", cell.ped)):
            for name in ("feat", "highway_input", "highway", "tpcnn"):
                for kind in ("weight", "bias"):
                    t = getattr(getattr(mod, name), kind)
                    out[f"implicit_cells.{i}.{prefix}{name}.{kind}"] = grads[i, at:at + t.numel()].view(t.shape)
                    at += t.numel()
        for name in ("global_w", "local_w"):
            out[f"implicit_cells.{i}.{name}"] = grads[i, at:at + 1]
            at += 1
        assert at == grads.shape[1]
    return out


def _implicit_backward(who, entry, model, params, dev, n, workspace, lead, g, tail):
    """the shared end of the two backward calls: ``lead`` / ``tail`` are the entry's arguments before N / after g"""
    if n and (workspace is None or workspace.device != dev or workspace.dtype != torch.uint8
              or not workspace.is_contiguous()):
        raise ValueError(f"{who}: workspace is not the uint8 tensor the forward call filled")
    grads = torch.empty((params.n_bins, implicit_grad_size(params)), device=dev)
    ws, nbytes = _workspace("et_implicit_backward_workspace_bytes", dev, params, n)
    L.call(entry, C.byref(params), *lead, n, L.ptr(workspace), _numel(workspace), L.ptr(g), *tail, L.ptr(grads), L.ptr(ws),
           nbytes, L.stream(dev))
    return grads


def implicit_backward_graph(model, v, workspace, g_out, et_params=None):
    """The backward pass of :func:`implicit_forward_graph` in TWO launches: ``v`` (1, 1, T, N) and ``workspace`` as that call
    read / filled them (same weights), ``g_out`` (1, S, T_out, N) the gradient at its output -> grads (n_bins, G) float32,
    one block per cell in ``et_implicit_cell``'s field order (:func:`implicit_grad_views` names its parts); a cell without
    pedestrians holds +0.0.  A ``g_out`` that is the permuted view of a contiguous (T_out, N, S) tensor, as the implicit
    bridge's post-hook makes it, is read where it is."""
    params, dev = et_params or model.et_params()
    T, To, S = params.temporal_input, params.temporal_output, params.spatial_output
    if v.dim() != 4 or tuple(v.shape[:3]) != (1, 1, T):
        raise ValueError(f"implicit_backward_graph: v {tuple(v.shape)} is not (1,1,{T},N)")
    n = v.shape[-1]
    if tuple(g_out.shape) != (1, S, To, n):
        raise ValueError(f"implicit_backward_graph: g_out {tuple(g_out.shape)} is not (1,{S},{To},{n})")
    (v,) = _dev_args(dev, v)
    g_out = g_out.detach()
    if g_out.device != dev or g_out.dtype != torch.float32:
        g_out = g_out.to(device=dev, dtype=torch.float32)
    tns = g_out.permute(0, 2, 3, 1).is_contiguous()  # ET_IMPLICIT_G_TNS: (T_out, N, S) in memory
    if not tns:
        g_out = g_out.contiguous()
    return _implicit_backward("implicit_backward_graph", "et_implicit_backward_graph", model, params, dev, n, workspace,
                              (L.ptr(v),), g_out, (int(tns),))


def implicit_backward_scenes(model, workspace, g):
    """The backward pass of :func:`implicit_forward_scenes` in TWO launches whatever the number of scenes: ``workspace`` as
    that call filled it, ``g`` (T_out, N, S) the gradient at C_pred_refine -> grads (n_bins, G) as
    :func:`implicit_backward_graph`, summed over all scenes."""
    params, dev = model.et_params()
    if g.dim() != 3 or (g.shape[0], g.shape[2]) != (params.temporal_output, params.spatial_output):
        raise ValueError(f"implicit_backward_scenes: g {tuple(g.shape)} is not ({params.temporal_output}, N, "
                         f"{params.spatial_output})")
    (g,) = _dev_args(dev, g)
    return _implicit_backward("implicit_backward_scenes", "et_implicit_backward_scenes", model, params, dev, g.shape[1],
                              workspace, (), g, ())


# ------------------------------------------------------------------------------ AgentFormer predictor (inference)
def agentformer_forward_graph(model, pre_motion):
    """``model`` (:class:`eigentrajectory_amd.agentformer.AgentFormerLight`, eval mode) on one scene as the agentformer
    bridge hands it over: pre_motion (T, N, 1) or (T, N) -> ``_seq_out`` (k, N, S).  1 + 2 encoder layers + 4 decoder layers
    launches."""
    params, dev = model.et_params()
    T, k, S = params.past_frames, params.future_frames, params.forecast_dim
    if pre_motion.dim() == 3 and pre_motion.shape[2] == 1:
        pre_motion = pre_motion[:, :, 0]
    if pre_motion.dim() != 2 or pre_motion.shape[0] != T:
        raise ValueError(f"agentformer_forward_graph: pre_motion {tuple(pre_motion.shape)} is not ({T},N,1)")
    n = pre_motion.shape[1]
    if n > L.AGENTFORMER_MAX_SCENE_N:
        raise ValueError(f"agentformer_forward_graph: a scene of {n} pedestrians exceeds the {L.AGENTFORMER_MAX_SCENE_N} a "
                         "scene may have")
    (u,) = _dev_args(dev, pre_motion)
    out = torch.empty((k, n, S), device=dev)
    ws, nbytes = _workspace("et_agentformer_workspace_bytes", dev, params, n, n)
    L.call("et_agentformer_forward_graph", C.byref(params), L.ptr(u), n, L.ptr(out), L.ptr(ws), nbytes, L.stream(dev))
    return out


def agentformer_forward_scenes(model, C_obs, nrm, scene_sizes=None, want_details=False):
    """The agentformer bridge + ``model`` (eval mode) + the post-hook for every scene of a split in 2 + 2 encoder layers + 4
    decoder layers launches: C_obs, nrm and ``scene_sizes`` as :func:`stgcnn_forward_scenes`, k = future_frames =
    past_frames - 2 -> C_pred_refine (k, N, S).  One unlisted scene of more than 128 pedestrians raises ValueError; a listed
    one is not computed: its rows are NaN.  With ``want_details`` also a dict: ``graph_inputs`` (k + 2, N), the fp32
    pre_motion = [C_obs; obs_ori] the kernels used."""
    params, dev = model.et_params()
    k = params.future_frames
    if params.past_frames != k + 2:
        raise ValueError(f"agentformer_forward_scenes: past_frames = {params.past_frames} is not future_frames + 2 = {k + 2}, "
                         f"the rows of [C_obs; obs_ori] (C_obs {tuple(C_obs.shape)} / nrm {tuple(nrm.shape)})")
    b = _scene_batch("agentformer_forward_scenes", dev, C_obs, nrm, k, scene_sizes)
    n = b.n
    if b.off is None and n > L.AGENTFORMER_MAX_SCENE_N:
        raise ValueError(f"agentformer_forward_scenes: one scene of {n} pedestrians exceeds the "
                         f"{L.AGENTFORMER_MAX_SCENE_N} a scene may have")
    out = torch.empty((k, n, params.forecast_dim), device=dev)
    gin = torch.empty((k + 2, n), device=dev) if want_details else None
    ws, nbytes = _workspace("et_agentformer_workspace_bytes", dev, params, n, b.max_n)
    L.call("et_agentformer_forward_scenes", C.byref(params), L.ptr(b.C_obs), L.ptr(b.nrm), n, L.ptr(b.off), b.n_scenes,
           L.ptr(out), L.ptr(gin), L.ptr(ws), nbytes, L.stream(dev))
    return (out, {"graph_inputs": gin}) if want_details else out


# ------------------------------------------------------------------------------ Graph-TERN predictor (inference)
def graphtern_forward_graph(model, S_obs):
    """``model`` (:class:`eigentrajectory_amd.graphtern.GraphTERNLight`, eval mode) on one scene as the graphtern bridge
    hands it over: S_obs (1, 2, T, N, 1) = [abs, rel], both read as given -> the raw output (1, k, N, S).  One launch."""
    params, dev = model.et_params()
    T, k, S = params.seq_len, params.pred_seq_len, params.n_smpl
    n = S_obs.shape[3] if S_obs.dim() == 5 else -1
    if tuple(S_obs.shape) != (1, 2, T, n, 1):
        raise ValueError(f"graphtern_forward_graph: S_obs {tuple(S_obs.shape)} is not (1,2,{T},N,1)")
    (S_obs,) = _dev_args(dev, S_obs)
    out = torch.empty((1, k, n, S), device=dev)
    ws, nbytes = _workspace("et_graphtern_workspace_bytes", dev, params, n, n)
    L.call("et_graphtern_forward_graph", C.byref(params), L.ptr(S_obs), n, L.ptr(out), L.ptr(ws), nbytes, L.stream(dev))
    return out


def graphtern_forward_scenes(model, C_obs, nrm, scene_sizes=None, want_details=False):
    """The graphtern bridge + ``model`` (eval mode) + the post-hook for every scene of a split in ONE launch: C_obs, nrm and
    ``scene_sizes`` as :func:`stgcnn_forward_scenes` -> C_pred_refine (k, N, S).  With ``want_details`` also a dict:
    ``graph_inputs`` (T, N), the fp32 u = [C_obs; obs_ori] the kernel used."""
    params, dev = model.et_params()
    b = _scene_batch("graphtern_forward_scenes", dev, C_obs, nrm, params.pred_seq_len, scene_sizes)
    out = torch.empty((params.pred_seq_len, b.n, params.n_smpl), device=dev)
    gin = torch.empty((params.seq_len, b.n), device=dev) if want_details else None
    ws, nbytes = _workspace("et_graphtern_workspace_bytes", dev, params, b.n, b.max_n)
    L.call("et_graphtern_forward_scenes", C.byref(params), L.ptr(b.C_obs), L.ptr(b.nrm), b.n, L.ptr(b.off), b.n_scenes,
           L.ptr(out), L.ptr(gin), L.ptr(ws), nbytes, L.stream(dev))
    return (out, {"graph_inputs": gin}) if want_details else out


# ------------------------------------------------------------------------------ Graph-TERN predictor (training)
def graphtern_train_workspace(model, n, n_scenes=1, et_params=None):
    """A training workspace for ``n`` pedestrians in ``n_scenes`` scenes: :func:`graphtern_train_forward_graph` /
    ``_scenes`` fill it, :func:`graphtern_backward_graph` / ``_scenes`` read it (None for ``n`` = 0)."""
    return _train_workspace("graphtern", model, et_params, n, max(n_scenes, 1))


def graphtern_train_forward_graph(model, S_obs, workspace, keep=None, et_params=None):
    """``model`` in training mode on one scene as the graphtern bridge hands it over: S_obs (1, 2, T, N, 1) = [abs, rel],
    ``keep`` uint8 (4, T, N, N) indexed [r, t, w, v] (:meth:`GraphTERNLight.draw_keep`; None keeps every edge) -> the raw
    output (1, k, N, S).  What the backward reads stays in ``workspace`` (of :func:`graphtern_train_workspace`) for
    :func:`graphtern_backward_graph`.  One launch."""
    params, dev = _train_params("graphtern_train_forward_graph", model, et_params)
    T, k, S = params.seq_len, params.pred_seq_len, params.n_smpl
    n = S_obs.shape[3] if S_obs.dim() == 5 else -1
    if tuple(S_obs.shape) != (1, 2, T, n, 1):
        raise ValueError(f"graphtern_train_forward_graph: S_obs {tuple(S_obs.shape)} is not (1,2,{T},N,1)")
    if n > L.GRAPHTERN_TRAIN_MAX_N:
        raise ValueError(f"graphtern_train_forward_graph: N = {n} exceeds the {L.GRAPHTERN_TRAIN_MAX_N} pedestrians a "
                         "training scene may have")
    (S_obs,) = _dev_args(dev, S_obs.detach())
    keep = _keep_mask("graphtern_train_forward_graph", dev, keep, shape=(L.GRAPHTERN_REL, T, n, n))
    out = torch.empty((1, k, n, S), device=dev)
    if n:
        _check_train_ws("graphtern_train_forward_graph", dev, workspace, "graphtern_train_workspace")
    L.call("et_graphtern_train_forward_graph", C.byref(params), L.ptr(S_obs), n, L.ptr(keep), L.ptr(out), L.ptr(workspace),
           _numel(workspace), L.stream(dev))
    return out


def graphtern_keep_offsets(scene_sizes, device=None):
    """-> (int64 tensor (n_scenes + 1,): where each scene's (4, T, n, n) block of a packed keep mask starts, in units of
    4 T entries (the running sum of n^2; a scene above the training cap takes no room), the total sum of n^2)"""
    return _keep_offsets(scene_sizes, L.GRAPHTERN_TRAIN_MAX_N, device)


def graphtern_train_forward_scenes(model, C_obs, nrm, scene_sizes=None, keep=None, workspace=None):
    """The graphtern bridge + ``model`` in training mode + the post-hook for every scene of a batch in ONE launch, one
    workgroup per scene.  C_obs, nrm and ``scene_sizes`` as :func:`graphtern_forward_scenes`; ``keep``: uint8, every scene's
    (4, T, n, n) block one after the other (:func:`graphtern_keep_offsets`), None keeps every edge -> (C_pred_refine
    (k, N, S), workspace); the workspace (made here unless given) goes to :func:`graphtern_backward_scenes` with the same
    ``scene_sizes``.  A scene of more than 512 pedestrians is not computed (NaN rows)."""
    params, dev = _train_params("graphtern_train_forward_scenes", model, None)
    b = _scene_batch("graphtern_train_forward_scenes", dev, C_obs, nrm, params.pred_seq_len, scene_sizes)
    if scene_sizes is None and b.n > L.GRAPHTERN_TRAIN_MAX_N:
        raise ValueError(f"graphtern_train_forward_scenes: one unlisted scene of {b.n} pedestrians exceeds the "
                         f"{L.GRAPHTERN_TRAIN_MAX_N} a training scene may have")
    if workspace is None:
        workspace = graphtern_train_workspace(model, b.n, len(b.sizes), et_params=(params, dev))
    if b.n:
        _check_train_ws("graphtern_train_forward_scenes", dev, workspace, "graphtern_train_workspace")
    koff, total = graphtern_keep_offsets(b.sizes, dev if keep is not None else None)
    keep = _keep_mask("graphtern_train_forward_scenes", dev, keep, numel=L.GRAPHTERN_REL * params.seq_len * total)
    out = torch.empty((params.pred_seq_len, b.n, params.n_smpl), device=dev)
    L.call("et_graphtern_train_forward_scenes", C.byref(params), L.ptr(b.C_obs), L.ptr(b.nrm), b.n, L.ptr(b.off), b.n_scenes,
           L.ptr(keep), L.ptr(koff if keep is not None else None), L.ptr(out), L.ptr(workspace), _numel(workspace),
           L.stream(dev))
    return out, workspace


def graphtern_grad_views(model, grads):
    """``grads``, the flat buffer of :func:`graphtern_backward_graph` / ``_scenes`` -> {state_dict key: a view of it shaped
    like the parameter}, every parameter of ``model`` (state_dict order).  ``tp_mrgcns.0.prelu.weight``, which the forward
    never applies, is always +0."""
    return _grad_views("graphtern_grad_views", model, grads)


def graphtern_backward_graph(model, workspace, d_out, et_params=None):
    """The backward pass of :func:`graphtern_train_forward_graph` in three launches: ``workspace`` as that call filled it
    (same weights), ``d_out`` (1, k, N, S) the gradient at its output -> the flat float32 gradient buffer
    (:func:`graphtern_grad_views` names its parts)."""
    return _backward_graph("graphtern", model, workspace, d_out, et_params, 2,
                           lambda p, n: (1, p.pred_seq_len, n, p.n_smpl))


def graphtern_backward_scenes(model, workspace, d_out, scene_sizes=None):
    """The backward pass of :func:`graphtern_train_forward_scenes` in three launches whatever the number of scenes:
    ``workspace`` as that call filled it, ``scene_sizes`` as given to it, ``d_out`` (k, N, S) -> the flat gradient buffer,
    summed over the scenes in ascending order."""
    return _backward_scenes("graphtern", model, workspace, d_out, scene_sizes, lambda p: (p.pred_seq_len, p.n_smpl))


def graphtern_train_layout(model, n, n_scenes=1):
    """-> the ``ET_GRAPHTERN_TRAIN_LAYOUT_FIELDS`` offsets of a training workspace, in floats (``et_graphtern_train_layout``;
    include/eigentraj.h names the fields)"""
    return list(vars(_graphtern_layout(model.et_params()[0], n, n_scenes)).values())


def _graphtern_layout(params, n, n_scenes):
    return _layout("et_graphtern_train_layout", L.GRAPHTERN_TRAIN_LAYOUT_NAMES, params, n, n_scenes)


def graphtern_train_views(model, workspace, n, n_scenes=1, lo=0, scene=0, scene_n=None):
    """The values kept in ``workspace`` by name, as views, for scene number ``scene`` of ``scene_n`` pedestrians that starts
    at row ``lo`` (one scene: the defaults).  Forward: ``u`` (T, n), ``d`` (4, T, n), ``P`` (4, 2, T, n) (the contracted
    rows: j = 0 from u, j = 1 from the ones row), ``yp`` (16, T, n) the tcn PReLU's input, ``x0`` (T, 16, n) the st_mrgcn
    block's output, and per epcnn block the lists ``c0`` / ``y`` (k, 16, n) and ``c1`` / ``o`` (k, C_out, n).  After a
    backward call also ``d_o`` (k, C_out, n) and ``d_y`` (k, 16, n) per block, ``d_x0`` (T, 16, n), ``d_yt`` (16, T, n) the
    gradient at PReLU(yp), and ``partial``, the scene's own flat gradient.  The offsets are the library's
    (``et_graphtern_train_layout``)."""
    params, _ = model.et_params()
    T, k, S, H = params.seq_len, params.pred_seq_len, params.n_smpl, params.hidden_feat
    m = n if scene_n is None else scene_n
    f = workspace.view(torch.float32)
    lay = _graphtern_layout(params, n, n_scenes)
    base = lo * lay.per
    fld = lambda off, *shape: f[base + off * m:base + off * m + math.prod(shape) * m].view(*shape, m)
    kH, kC = k * H, k * max(H, S)
    views = {"u": fld(lay.u, T), "d": fld(lay.d, L.GRAPHTERN_REL, T), "P": fld(lay.P, L.GRAPHTERN_REL, 2, T),
             "yp": fld(lay.yp, H, T), "x0": fld(lay.x0, T, H), "d_x0": fld(lay.dx0, T, H), "d_yt": fld(lay.dy, H, T)}
    blocks = range(params.n_epcnn)
    cout = [S if j + 1 == params.n_epcnn else H for j in blocks]
    views["c0"] = [fld(lay.tp + j * lay.tp_stride, k, H) for j in blocks]
    views["y"] = [fld(lay.tp + j * lay.tp_stride + kH, k, H) for j in blocks]
    views["c1"] = [fld(lay.tp + j * lay.tp_stride + 2 * kH, k, cout[j]) for j in blocks]
    views["o"] = [fld(lay.tp + j * lay.tp_stride + 2 * kH + kC, k, cout[j]) for j in blocks]
    views["d_o"] = [fld(lay.dtp + j * lay.dtp_stride, k, cout[j]) for j in blocks]
    views["d_y"] = [fld(lay.dtp + j * lay.dtp_stride + kC, k, H) for j in blocks]
    views["partial"] = f[lay.partials + scene * lay.grads:lay.partials + (scene + 1) * lay.grads]
    return views


# ------------------------------------------------------------------------------ PECNet / LBEBM predictors (inference)
def _mlp_rows(who, dev, width, **tensors):
    """(N, width_i) float32 rows on ``dev``, all of one N"""
    out = _dev_args(dev, *tensors.values())
    n = out[0].shape[0]
    for (name, _), t, w in zip(tensors.items(), out, width):
        if t.dim() != 2 or tuple(t.shape) != (n, w):
            raise ValueError(f"{who}: {name} {tuple(t.shape)} is not ({n}, {w})")
    return n, out


def pecnet_predict(model, past, generated_dest, mask, initial_pos):
    """``model`` (:class:`eigentrajectory_amd.pecnet.PECNet`, eval mode): past (N, 2 past_length), generated_dest (N, 2),
    mask (N, N) bool or float32 (None: all ones), initial_pos (N, 2) -> (N, out_width), the reference's ``predict``.
    2 + 2 nonlocal_pools launches."""
    params, dev = model.et_params()
    n, (past, dest, pos) = _mlp_rows("pecnet_predict", dev, (params.encoder_past.widths[0], params.encoder_dest.widths[0], 2),
                                     past=past, generated_dest=generated_dest, initial_pos=initial_pos)
    if mask is not None:
        (mask,) = _dev_args(dev, mask)  # bool -> float32
        if tuple(mask.shape) != (n, n):
            raise ValueError(f"pecnet_predict: mask {tuple(mask.shape)} is not ({n}, {n})")
    out = torch.empty((n, params.out_width), device=dev)
    ws, nbytes = _workspace("et_pecnet_workspace_bytes", dev, params, n)
    L.call("et_pecnet_predict", C.byref(params), L.ptr(past), L.ptr(dest), L.ptr(mask), L.ptr(pos), n, L.ptr(out), L.ptr(ws),
           nbytes, L.stream(dev))
    return out


def lbebm_predict(model, past, generated_dest):
    """``model`` (:class:`eigentrajectory_amd.lbebm.LBEBM`, eval mode): past (N, 2 past_length), generated_dest
    (N, 2 sub-goals) -> (N, out_width), the reference's ``predict``.  2 launches."""
    params, dev = model.et_params()
    n, (past, dest) = _mlp_rows("lbebm_predict", dev, (params.encoder_past.widths[0], params.encoder_dest.widths[0]),
                                past=past, generated_dest=generated_dest)
    out = torch.empty((n, params.out_width), device=dev)
    ws, nbytes = _workspace("et_lbebm_workspace_bytes", dev, params, n)
    L.call("et_lbebm_predict", C.byref(params), L.ptr(past), L.ptr(dest), n, L.ptr(out), L.ptr(ws), nbytes, L.stream(dev))
    return out


def _mlp_forward_scenes(kind, model, C_obs, nrm, scene_sizes, want_details):
    params, dev = model.et_params()
    k = params.encoder_past.widths[0]
    b = _scene_batch(f"{kind}_forward_scenes", dev, C_obs, nrm, k, scene_sizes)
    n = b.n
    if params.nonlocal_pools > 0 and b.max_n > L.MLP_MAX_RANGE:
        raise ValueError(f"{kind}_forward_scenes: a scene of {b.max_n} pedestrians is beyond the pooling step's range of "
                         f"{L.MLP_MAX_RANGE} (ET_MLP_MAX_RANGE)")
    out = torch.empty((k, n, params.out_width // max(k, 1)), device=dev)
    gin = torch.empty((k + 2, n), device=dev) if want_details else None
    ws, nbytes = _workspace(f"et_{kind}_workspace_bytes", dev, params, n)
    L.call(f"et_{kind}_forward_scenes", C.byref(params), L.ptr(b.C_obs), L.ptr(b.nrm), n, L.ptr(b.off), b.n_scenes,
           L.ptr(out), L.ptr(gin), L.ptr(ws), nbytes, L.stream(dev))
    return (out, {"net_inputs": gin}) if want_details else out


def pecnet_forward_scenes(model, C_obs, nrm, scene_sizes=None, want_details=False):
    """The pecnet bridge + ``model.predict`` (eval mode) + the post-hook for every scene of a split in 2 + 2 nonlocal_pools
    launches: C_obs, nrm and ``scene_sizes`` as :func:`stgcnn_forward_scenes` -> C_pred_refine (k, N, S).  Every scene is its own softmax range under an all-ones mask, as in the reference's test loop
    (one scene per call); a scene of more than ET_MLP_MAX_RANGE (4096) pedestrians raises ValueError before any launch.  With
    ``want_details`` also a dict: ``net_inputs`` (k + 2, N), the fp32 [C_obs; obs_ori] used."""
    return _mlp_forward_scenes("pecnet", model, C_obs, nrm, scene_sizes, want_details)


def lbebm_forward_scenes(model, C_obs, nrm, scene_sizes=None, want_details=False):
    """The lbebm bridge + ``model.predict`` (eval mode) + the post-hook for every scene of a split in 2 launches; arguments
    and results as :func:`pecnet_forward_scenes`."""
    return _mlp_forward_scenes("lbebm", model, C_obs, nrm, scene_sizes, want_details)


# ------------------------------------------------------------------------------------- LBEBM predictor (training)
def _mlp_strided(who, dev, width, **tensors):
    """(N, width_i) float32 tensors on ``dev``, all of one N, as the kernels read them in place: a row-major tensor or the
    transposed view of one (the bridge's ``C_obs.T``) stays as it is, anything else is copied"""
    out = []
    for t in tensors.values():
        t = t.detach()
        if t.device != dev or t.dtype != torch.float32:
            t = t.to(device=dev, dtype=torch.float32)
        if t.dim() == 2 and not (t.is_contiguous() or t.t().is_contiguous()):
            t = t.contiguous()
        out.append(t)
    n = out[0].shape[0]
    for name, t, w in zip(tensors, out, width):
        if t.dim() != 2 or tuple(t.shape) != (n, w):
            raise ValueError(f"{who}: {name} {tuple(t.shape)} is not ({n}, {w})")
    return n, out


def lbebm_train_fwd(model, past, generated_dest):
    """``model`` (:class:`eigentrajectory_amd.lbebm.LBEBM`): past (N, 2 past_length), generated_dest (N, 2 sub-goals), read
    in place through their strides -> (out, saved): out (N, out_width) is :func:`lbebm_predict`'s, bit for bit, in the same
    2 launches; ``saved`` (float32, flat) holds the activations :func:`lbebm_train_bwd` needs (layout: include/eigentraj.h,
    "LBEBM predictor, training")."""
    params, dev = model.et_params()
    n, (past, dest) = _mlp_strided("lbebm_train_fwd", dev, (params.encoder_past.widths[0], params.encoder_dest.widths[0]),
                                   past=past, generated_dest=generated_dest)
    out = torch.empty((n, params.out_width), device=dev)
    saved = torch.empty((L.lib().et_lbebm_train_workspace_bytes(C.byref(params), n) // 4,), device=dev)
    L.call("et_lbebm_train_fwd", C.byref(params), L.ptr(past), past.stride(0), past.stride(1), L.ptr(dest), dest.stride(0),
           dest.stride(1), n, L.ptr(out), L.ptr(saved), None, 0, L.stream(dev))
    return out, saved


def lbebm_train_bwd(model, past, generated_dest, saved, g_out, need_input_grads=False):
    """The backward pass of :func:`lbebm_train_fwd` in 3 launches: ``saved`` as that call returned it (same ``model``
    weights, same inputs), ``g_out`` (N, out_width) the gradient at its ``out`` -> a dict keyed by the module's parameter
    names (``encoder_past.layers.0.weight``, ...) of fresh tensors holding the gradients (nothing is accumulated), plus
    ``past`` / ``dest``, laid out like the inputs, when ``need_input_grads`` (a bool, or one per input) asks for them."""
    params, dev = model.et_params()
    n, (past, dest) = _mlp_strided("lbebm_train_bwd", dev, (params.encoder_past.widths[0], params.encoder_dest.widths[0]),
                                   past=past, generated_dest=generated_dest)
    (g_out,) = _dev_args(dev, g_out)
    nbytes = L.lib().et_lbebm_train_workspace_bytes(C.byref(params), n)
    if tuple(g_out.shape) != (n, params.out_width):
        raise ValueError(f"lbebm_train_bwd: g_out {tuple(g_out.shape)} is not ({n}, {params.out_width})")
    if saved.device != dev or saved.dtype != torch.float32 or not saved.is_contiguous() or saved.numel() * 4 < nbytes:
        raise ValueError(f"lbebm_train_bwd: saved is not the {nbytes // 4} float32 values lbebm_train_fwd returned for "
                         f"{n} rows")
    want_past, want_dest = (need_input_grads if isinstance(need_input_grads, (tuple, list)) else (need_input_grads,) * 2)
    # one tensor per gradient: autograd's accumulation takes a fresh, unshared tensor over as .grad without a copy
    out = {name: torch.empty_like(t) for name, t in zip(model.chain_parameter_names(), model.chain_parameters())}
    grads = L.LBEBMGrads()
    for chain in model.CHAINS:
        g = getattr(grads, chain)
        for i in range(len(getattr(model, chain).layers)):
            g.dw[i] = out[f"{chain}.layers.{i}.weight"].data_ptr()
            g.db[i] = out[f"{chain}.layers.{i}.bias"].data_ptr()
    if want_past:
        out["past"] = torch.empty_strided(past.shape, past.stride(), device=dev)
    if want_dest:
        out["dest"] = torch.empty_strided(dest.shape, dest.stride(), device=dev)
    ws = torch.empty((nbytes // 4,), device=dev)
    L.call("et_lbebm_train_bwd", C.byref(params), L.ptr(past), past.stride(0), past.stride(1), L.ptr(dest), dest.stride(0),
           dest.stride(1), n, L.ptr(saved), L.ptr(g_out), C.byref(grads), L.ptr(out.get("past")), L.ptr(out.get("dest")),
           L.ptr(ws), nbytes, L.stream(dev))
    return out


# ------------------------------------------------------------------------------------- PECNet predictor (training)
def _pecnet_train_args(who, model, past, generated_dest, mask, initial_pos):
    params, dev = model.et_params()
    n, (past, dest, pos) = _mlp_strided(who, dev, (params.encoder_past.widths[0], params.encoder_dest.widths[0], 2),
                                        past=past, generated_dest=generated_dest, initial_pos=initial_pos)
    if mask is not None:
        (mask,) = _dev_args(dev, mask)  # bool -> float32
        if tuple(mask.shape) != (n, n):
            raise ValueError(f"{who}: mask {tuple(mask.shape)} is not ({n}, {n})")
    if params.nonlocal_pools > 0 and n > L.MLP_MAX_RANGE:
        raise ValueError(f"{who}: {n} rows are beyond the pooling step's range of {L.MLP_MAX_RANGE} (ET_MLP_MAX_RANGE)")
    strided = []
    for t in (past, dest, pos):
        strided += [L.ptr(t), t.stride(0), t.stride(1)]
    return params, dev, n, (past, dest, pos), mask, strided


def pecnet_train_fwd(model, past, generated_dest, mask, initial_pos):
    """``model`` (:class:`eigentrajectory_amd.pecnet.PECNet`): past (N, 2 past_length), generated_dest (N, 2), initial_pos
    (N, 2), read in place through their strides; mask (N, N) bool or float32 (None: all ones) -> (out, saved): out
    (N, out_width) is :func:`pecnet_predict`'s, bit for bit, in the same 2 + 2 nonlocal_pools launches; ``saved`` (float32,
    flat) holds what :func:`pecnet_train_bwd` needs (layout: csrc/et_mlp_train.hip, "PECNet")."""
    params, dev, n, _, mask, strided = _pecnet_train_args("pecnet_train_fwd", model, past, generated_dest, mask, initial_pos)
    out = torch.empty((n, params.out_width), device=dev)
    saved = torch.empty((L.lib().et_pecnet_train_saved_bytes(C.byref(params), n) // 4,), device=dev)
    L.call("et_pecnet_train_fwd", C.byref(params), *strided, L.ptr(mask), n, L.ptr(out), L.ptr(saved), None, 0, L.stream(dev))
    return out, saved


def pecnet_train_bwd(model, past, generated_dest, mask, initial_pos, saved, g_out, need_input_grads=False):
    """The backward pass of :func:`pecnet_train_fwd` in 3 + 3 nonlocal_pools launches: ``saved`` as that call returned it
    (same ``model`` weights, same inputs, same mask), ``g_out`` (N, out_width) the gradient at its ``out`` -> a dict keyed by
    the module's parameter names (``encoder_past.layers.0.weight``, ...; the six chains, or without pooling rounds the
    three that run) of fresh tensors holding the gradients (nothing is accumulated), plus ``past`` / ``dest`` / ``pos``, laid
    out like the inputs, when ``need_input_grads`` (a bool, or one per input) asks for them.  The mask gets none."""
    params, dev, n, (past, dest, pos), mask, strided = _pecnet_train_args("pecnet_train_bwd", model, past, generated_dest,
                                                                          mask, initial_pos)
    (g_out,) = _dev_args(dev, g_out)
    if tuple(g_out.shape) != (n, params.out_width):
        raise ValueError(f"pecnet_train_bwd: g_out {tuple(g_out.shape)} is not ({n}, {params.out_width})")
    sbytes = L.lib().et_pecnet_train_saved_bytes(C.byref(params), n)
    if saved.device != dev or saved.dtype != torch.float32 or not saved.is_contiguous() or saved.numel() * 4 < sbytes:
        raise ValueError(f"pecnet_train_bwd: saved is not the {sbytes // 4} float32 values pecnet_train_fwd returned for "
                         f"{n} rows")
    want = need_input_grads if isinstance(need_input_grads, (tuple, list)) else (need_input_grads,) * 3
    chains = model.CHAINS if params.nonlocal_pools > 0 else model.CHAINS_WITHOUT_POOLING
    # one tensor per gradient: autograd's accumulation takes a fresh, unshared tensor over as .grad without a copy
    out = {name: torch.empty_like(t) for name, t in zip(model.chain_parameter_names(), model.chain_parameters())
           if name.split(".")[0] in chains}
    grads = L.PECNetGrads()
    for chain in chains:
        g = getattr(grads, chain)
        for i in range(len(getattr(model, chain).layers)):
            g.dw[i] = out[f"{chain}.layers.{i}.weight"].data_ptr()
            g.db[i] = out[f"{chain}.layers.{i}.bias"].data_ptr()
    for key, t, wanted in zip(("past", "dest", "pos"), (past, dest, pos), want):
        if wanted:
            out[key] = torch.empty_strided(t.shape, t.stride(), device=dev)
    nbytes = L.lib().et_pecnet_train_workspace_bytes(C.byref(params), n)
    ws = torch.empty((nbytes // 4,), device=dev)
    L.call("et_pecnet_train_bwd", C.byref(params), *strided, L.ptr(mask), n, L.ptr(saved), L.ptr(g_out), C.byref(grads),
           L.ptr(out.get("past")), L.ptr(out.get("dest")), L.ptr(out.get("pos")), L.ptr(ws), nbytes, L.stream(dev))
    return out


# ----------------------------------------------------------------------- curve fitting
def curve_fit_batch(trajs, bases, steps=100000, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, want_cp=False, want_loss=False):
    """CurveModel/curve_fitting.py for a batch of fits: fit f fits basis ``bases[f]`` (T_f, ncp_f) to every trajectory of
    ``trajs[f]`` (N_f, T_f, 2) (already normalised) by ``steps`` Adam steps on the mean L2 error.  All fits of up to
    ET_CURVE_MAX_FITS (64) run in one launch per pass; longer lists are split.  Returns a dict:
    ``recon`` list of (N_f, T_f, 2) float32, the recon of each fit's best step; ``best`` (B,) int64 best steps;
    ``cp`` list of (N_f, ncp_f, 2) control points (want_cp); ``loss`` (B, steps) float64 per-step mean loss (want_loss)."""
    if len(trajs) != len(bases) or not trajs:
        raise ValueError("curve_fit_batch: trajs and bases must be non-empty lists of the same length")
    dev = L.require_device(*trajs, *bases)
    trajs = [t.to(dev, torch.float32).contiguous() for t in trajs]
    bases = [b.to(dev, torch.float32).contiguous() for b in bases]
    out = {"recon": [], "best": [], "cp": [] if want_cp else None, "loss": [] if want_loss else None}
    for c0 in range(0, len(trajs), L.CURVE_MAX_FITS):
        tr, bs = trajs[c0:c0 + L.CURVE_MAX_FITS], bases[c0:c0 + L.CURVE_MAX_FITS]
        fits, t_off, b_off, c_off = [], 0, 0, 0
        for t, b in zip(tr, bs):
            if t.dim() != 3 or t.shape[2] != 2 or b.dim() != 2 or b.shape[0] != t.shape[1]:
                raise ValueError(f"curve_fit_batch: traj {tuple(t.shape)} and basis {tuple(b.shape)} do not match")
            n, T, ncp = t.shape[0], t.shape[1], b.shape[1]
            fits.append([n, T, ncp, t_off, b_off, c_off])
            t_off, b_off, c_off = t_off + n * T * 2, b_off + T * ncp, c_off + n * ncp * 2
        nf = len(fits)
        table = (C.c_int64 * (6 * nf))(*[v for row in fits for v in row])
        traj = torch.cat([t.reshape(-1) for t in tr])
        basis = torch.cat([b.reshape(-1) for b in bs])
        recon = torch.empty_like(traj)
        cp = torch.empty((c_off,), device=dev, dtype=torch.float32) if want_cp else None
        loss = torch.empty((nf, int(steps)), device=dev, dtype=torch.float64) if want_loss else None
        best = torch.empty((nf,), device=dev, dtype=torch.int32)
        nbytes = L.lib().et_curve_fit_batch_workspace_bytes(nf, int(steps))
        if nbytes == 0:
            raise ValueError(f"curve_fit_batch: steps={steps} not taken")
        ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
        L.call("et_curve_fit_batch", L.ptr(traj), L.ptr(basis), table, nf, int(steps), float(lr), float(betas[0]),
               float(betas[1]), float(eps), L.ptr(recon), L.ptr(cp), L.ptr(loss), L.ptr(best), L.ptr(ws), nbytes,
               L.stream(dev))
        for (n, T, ncp, to, _, co) in fits:
            out["recon"].append(recon[to:to + n * T * 2].view(n, T, 2))
            if want_cp:
                out["cp"].append(cp[co:co + n * ncp * 2].view(n, ncp, 2))
        out["best"].append(best.long())
        if want_loss:
            out["loss"].append(loss)
    out["best"] = torch.cat(out["best"])
    if want_loss:
        out["loss"] = torch.cat(out["loss"])
    return out

# ------------------------------------------------------------------------------------ t-SNE
def _tsne_ws(nbytes, dev):
    if nbytes == 0:
        raise ValueError("t-SNE: arguments not taken")
    return torch.empty((nbytes,), device=dev, dtype=torch.uint8)


def tsne_affinities(X, perplexity=30.0):
    """sklearn's kNN + perplexity search + symmetrised P (et_tsne_affinities) for X (N,d) fp32, d <= 32.  -> dict:
    ``knn_idx`` (N,k) int32 and ``knn_dist`` (N,k) fp32 squared distances in column order, ``p_cond`` (N,k) fp64,
    ``indptr`` (N+1) int32, ``indices`` (nnz) int32, ``P`` (nnz) fp64 (canonical CSR, normalised), ``total`` (1) fp64."""
    dev = L.require_device(X)
    X = L.on_device(X, dev)
    if X.dim() != 2:
        raise ValueError("tsne_affinities: X must be (N, d)")
    n, d = X.shape
    k = L.lib().et_tsne_neighbors(n, float(perplexity))
    if k < 1:
        raise ValueError(f"tsne_affinities: N={n}, perplexity={perplexity} not taken")
    ws = _tsne_ws(L.lib().et_tsne_affinities_workspace_bytes(n, d, k), dev)
    out = {"knn_idx": torch.empty((n, k), device=dev, dtype=torch.int32),
           "knn_dist": torch.empty((n, k), device=dev),
           "p_cond": torch.empty((n, k), device=dev, dtype=torch.float64),
           "indptr": torch.empty((n + 1,), device=dev, dtype=torch.int32),
           "indices": torch.empty((2 * n * k,), device=dev, dtype=torch.int32),
           "P": torch.empty((2 * n * k,), device=dev, dtype=torch.float64),
           "total": torch.empty((1,), device=dev, dtype=torch.float64)}
    L.call("et_tsne_affinities", L.ptr(X), n, d, float(perplexity), k, L.ptr(out["knn_idx"]), L.ptr(out["knn_dist"]),
           L.ptr(out["p_cond"]), L.ptr(out["indptr"]), L.ptr(out["indices"]), L.ptr(out["P"]), L.ptr(out["total"]),
           L.ptr(ws), ws.numel(), L.stream(dev))
    nnz = int(out["indptr"][n].item())
    out["indices"], out["P"] = out["indices"][:nnz], out["P"][:nnz]
    return out


def tsne_kl_grad(Y, indptr, indices, P, want_kl=True):
    """KL divergence and gradient at Y (N,2) with exact repulsion (et_tsne_kl_grad); P fp32 (fp64 is rounded to fp32,
    as sklearn's _kl_divergence_bh does).  -> (kl fp64 device scalar | None, grad (N,2) fp32)."""
    dev = L.require_device(Y)
    Y = L.on_device(Y, dev)
    if Y.dim() != 2 or Y.shape[1] != 2:
        raise ValueError("tsne_kl_grad: Y must be (N, 2)")
    n = Y.shape[0]
    indptr, indices = L.on_device(indptr, dev, torch.int32), L.on_device(indices, dev, torch.int32)
    P = L.on_device(P, dev, torch.float32)
    grad = torch.empty_like(Y)
    kl = torch.empty((1,), device=dev, dtype=torch.float64) if want_kl else None
    ws = _tsne_ws(L.lib().et_tsne_kl_grad_workspace_bytes(n), dev)
    L.call("et_tsne_kl_grad", L.ptr(Y), n, L.ptr(indptr), L.ptr(indices), L.ptr(P), L.ptr(grad), L.ptr(kl), L.ptr(ws),
           ws.numel(), L.stream(dev))
    return (kl[0] if want_kl else None), grad


def tsne_update(p, update, gains, grad, momentum, learning_rate):
    """One step of sklearn's _gradient_descent in place (et_tsne_update): p fp32, update fp64, gains fp32, grad fp32
    (scaled by the new gains)."""
    for t, dt in ((p, torch.float32), (update, torch.float64), (gains, torch.float32), (grad, torch.float32)):
        if t.dtype != dt or not t.is_contiguous() or t.numel() != p.numel():
            raise ValueError("tsne_update: p, gains, grad fp32 and update fp64, contiguous, of one size")
    dev = L.require_device(p)
    L.call("et_tsne_update", L.ptr(p), L.ptr(update), L.ptr(gains), L.ptr(grad), p.numel(), float(momentum),
           float(learning_rate), L.stream(dev))


def tsne_optimize(Y0, indptr, indices, P, early_exaggeration=12.0, learning_rate=200.0, max_iter=1000):
    """TSNE._tsne from Y0 (N,2) with the fp64 CSR P of :func:`tsne_affinities` (et_tsne_optimize).
    -> (Y (N,2) fp32, kl float, n_iter int)."""
    dev = L.require_device(Y0)
    Y = L.on_device(Y0, dev).clone()
    n = Y.shape[0]
    indptr, indices = L.on_device(indptr, dev, torch.int32), L.on_device(indices, dev, torch.int32)
    P = L.on_device(P, dev, torch.float64)
    ws = _tsne_ws(L.lib().et_tsne_optimize_workspace_bytes(n, P.numel()), dev)
    kl, it = C.c_double(0.0), C.c_int(0)
    L.call("et_tsne_optimize", L.ptr(Y), n, L.ptr(indptr), L.ptr(indices), L.ptr(P), P.numel(), float(early_exaggeration),
           float(learning_rate), int(max_iter), C.byref(kl), C.byref(it), L.ptr(ws), ws.numel(), L.stream(dev))
    return Y, kl.value, it.value


def tsne_pca_init(X):
    """sklearn's init="pca" for t-SNE (et_tsne_pca_init): X (N,d) -> Y0 (N,2) fp32."""
    dev = L.require_device(X)
    X = L.on_device(X, dev)
    n, d = X.shape
    Y = torch.empty((n, 2), device=dev)
    ws = _tsne_ws(L.lib().et_tsne_pca_init_workspace_bytes(n, d), dev)
    L.call("et_tsne_pca_init", L.ptr(X), n, d, L.ptr(Y), L.ptr(ws), ws.numel(), L.stream(dev))
    return Y


# ------------------------------------------------------------------------------------ fit
def fit_gram(obs, pred, mode, static_dist=0.0, which=1):
    """Gram matrices (fp64) of the normalised rows routed to descriptor ``which`` + their count (int64, device)."""
    dev = L.require_device(obs)
    obs, pred = _dev_args(dev, obs, pred)
    n, t_obs, _ = obs.shape
    t_pred = pred.shape[1]
    g_obs = torch.empty((2 * t_obs, 2 * t_obs), device=dev, dtype=torch.float64)
    g_pred = torch.empty((2 * t_pred, 2 * t_pred), device=dev, dtype=torch.float64)
    count = torch.empty((1,), device=dev, dtype=torch.int64)  # (written by the finish kernel, or zeroed for n == 0: no fill)
    ws_bytes = L.lib().et_fit_gram_workspace_bytes(n, t_obs, t_pred)
    ws = torch.empty((max(ws_bytes, 8),), device=dev, dtype=torch.uint8)
    L.call("et_fit_gram", L.ptr(obs), L.ptr(pred), n, t_obs, t_pred, int(mode), float(static_dist), int(which), L.ptr(g_obs),
           L.ptr(g_pred), L.ptr(count), L.ptr(ws), ws.numel(), L.stream(dev))
    return g_obs, g_pred, count


_FIT_WS_BYTES = {}  # (N, T_obs, T_pred) -> et_fit_descriptor_workspace_bytes


def fit_descriptor(obs, pred, k, mode, static_dist=0.0, which=1, want_gram=False):
    """descriptor.py:116-142 for one descriptor in ONE call (et_fit_descriptor: the Gram kernel, its partial reduction, and
    one launch that assembles and solves both eigenproblems).  -> (U_obs (2T_obs,k), U_pred (2T_pred,k), sigma_obs (k), sigma_pred (k),
    count (int64 device tensor)) and, with ``want_gram``, + (G_obs, G_pred) -- the same bits as :func:`fit_gram` +
    :func:`eigh_topk_batch`."""
    dev = L.require_device(obs)
    # (this call opens the bench step on an idle device: every microsecond of host time in front of its first launch is a
    # microsecond of the fit stage -- tensors that are already fp32 / contiguous / on the device pass as they are, the
    # workspace size is asked once per shape, one allocation holds the small outputs, the arguments cross as plain ints)
    if not (obs.device == dev and obs.dtype == torch.float32 and obs.is_contiguous() and not obs.requires_grad):
        (obs,) = _dev_args(dev, obs)
    if not (pred.device == dev and pred.dtype == torch.float32 and pred.is_contiguous() and not pred.requires_grad):
        (pred,) = _dev_args(dev, pred)
    n, t_obs, _ = obs.shape
    t_pred = pred.shape[1]
    k = int(k)
    do, dp = 2 * t_obs, 2 * t_pred
    key = (n, t_obs, t_pred)
    ws_bytes = _FIT_WS_BYTES.get(key)
    if ws_bytes is None:
        ws_bytes = _FIT_WS_BYTES[key] = max(int(L.lib().et_fit_descriptor_workspace_bytes(n, t_obs, t_pred)), 8)
    n_small = (do + dp) * k + 2 * k
    n_small += n_small % 2  # (the int64 count behind the floats: 8-byte aligned)
    buf = torch.empty((n_small + 2,), device=dev)
    U_obs, U_pred = buf[:do * k].view(do, k), buf[do * k:(do + dp) * k].view(dp, k)
    s_obs, s_pred = buf[(do + dp) * k:(do + dp) * k + k], buf[(do + dp) * k + k:(do + dp) * k + 2 * k]
    count = buf[n_small:].view(torch.int64)
    g_obs = torch.empty((do, do), device=dev, dtype=torch.float64) if want_gram else None
    g_pred = torch.empty((dp, dp), device=dev, dtype=torch.float64) if want_gram else None
    ws = torch.empty((ws_bytes,), device=dev, dtype=torch.uint8)
    p_buf = buf.data_ptr()
    rc = L.lib().et_fit_descriptor(obs.data_ptr(), pred.data_ptr(), n, t_obs, t_pred, k, int(mode), float(static_dist), int(which),
                                   p_buf, p_buf + 4 * do * k, p_buf + 4 * (do + dp) * k, p_buf + 4 * ((do + dp) * k + k),
                                   g_obs.data_ptr() if want_gram else None, g_pred.data_ptr() if want_gram else None,
                                   p_buf + 4 * n_small, ws.data_ptr(), ws_bytes, L.raw_stream(dev.index))
    if rc:
        L.check(rc, "et_fit_descriptor")
    return (U_obs, U_pred, s_obs, s_pred, count) + ((g_obs, g_pred) if want_gram else ())


def eigh_topk(G, k):
    """Top-k eigenvectors (n,k) fp32 and sigma (k,) = sqrt(eigenvalues) of a symmetric fp64 matrix."""
    dev = L.require_device(G)
    G = L.on_device(G, dev, torch.float64)
    n = G.shape[0]
    U = torch.empty((n, k), device=dev)
    sigma = torch.empty((k,), device=dev)
    L.call("et_eigh_topk", L.ptr(G), n, int(k), L.ptr(U), L.ptr(sigma), L.stream(dev))
    return U, sigma


def eigh_topk_batch(mats, k):
    """``eigh_topk`` of several symmetric fp64 matrices in one launch (one workgroup each, side by side).

    mats: sequence of (n_i, n_i) tensors; k: int or sequence of ints.  -> list of (U_i, sigma_i)."""
    mats = list(mats)
    if not mats:
        return []
    ks = [int(k)] * len(mats) if isinstance(k, int) else [int(x) for x in k]
    dev = L.require_device(mats[0])
    mats = [L.on_device(G, dev, torch.float64) for G in mats]
    outs = [(torch.empty((G.shape[0], kk), device=dev), torch.empty((kk,), device=dev)) for G, kk in zip(mats, ks)]
    b = len(mats)
    PD, PF, PI = C.c_void_p * b, C.c_void_p * b, C.c_int * b
    L.call("et_eigh_topk_batch", b, PD(*[G.data_ptr() for G in mats]), PI(*[G.shape[0] for G in mats]), PI(*ks),
           PF(*[U.data_ptr() for U, _ in outs]), PF(*[s.data_ptr() for _, s in outs]), L.stream(dev))
    return outs


# -------------------------------------------------------------------------------- k-means
def euc_sim(a, b):
    """kmeans.py:59-76: a (d,m), b (d,n) -> (m,n), or batched a (B,d,m), b (B,d,n) -> (B,m,n) in one launch."""
    dev = L.require_device(a, b)
    a, b = _dev_args(dev, a, b)
    if a.dim() == 3:
        B, d, m = a.shape
        n = b.shape[2]
        y = torch.empty((B, m, n), device=dev)
        L.call("et_euc_sim_batch", L.ptr(a), L.ptr(b), B, d, m, n, L.ptr(y), L.stream(dev))
        return y
    d, m = a.shape
    n = b.shape[1]
    y = torch.empty((m, n), device=dev)
    L.call("et_euc_sim", L.ptr(a), L.ptr(b), d, m, n, L.ptr(y), L.stream(dev))
    return y


def kmeans_workspace(n, d, K, device):
    nbytes = L.lib().et_kmeans_workspace_bytes(n, int(d), int(K))
    if nbytes == 0:
        raise ValueError(f"k-means dimensions out of range: d={d} (<= {L.KMEANS_MAX_D}), K={K} (<= {L.KMEANS_MAX_CLUSTERS})")
    return torch.empty((nbytes,), device=device, dtype=torch.uint8)


def kmeans_init_farthest(X, K, first_index, workspace=None):
    """kmeans.py:78-112 for one batch element: X (d,N) -> C0 (d,K)."""
    dev = L.require_device(X)
    (X,) = _dev_args(dev, X)
    d, n = X.shape
    ws = workspace if workspace is not None else kmeans_workspace(n, d, K, dev)
    c0 = torch.empty((d, K), device=dev)
    L.call("et_kmeans_init_farthest", L.ptr(X), n, d, int(K), int(first_index), L.ptr(c0), L.ptr(ws), ws.numel(),
           L.stream(dev))
    return c0


def kmeans_fit(X, centroids, max_iter=100, tol=1e-4, workspace=None, timing=False, trace=True):
    """kmeans.py:228-240 for one batch element from given initial centroids.

    Returns dict(centroids (d,K), labels (N,) int64, n_iter, error, inertia, trace (n_iter,2) | None, done).
    ``trace=False`` skips the per-iteration (error, inertia) record -- the reference only prints it when verbose
    (kmeans.py:236-237); the inertia of the last assignment is then evaluated once, after the loop (same bits).
    """
    dev = L.require_device(X)
    X, centroids = _dev_args(dev, X, centroids)
    d, n = X.shape
    K = centroids.shape[1]
    ws = workspace if workspace is not None else kmeans_workspace(n, d, K, dev)
    cen = centroids.clone()
    labels = torch.empty((n,), device=dev, dtype=torch.int64)
    trace_t = torch.zeros((max_iter, 2), device=dev) if trace else None
    st = L.KMeansState()
    tm = L.KMeansTiming() if timing else None
    L.call("et_kmeans_fit", L.ptr(X), n, d, K, int(max_iter), float(tol), L.ptr(cen), L.ptr(labels), L.ptr(trace_t),
           C.byref(st), C.byref(tm) if timing else None, L.ptr(ws), ws.numel(), L.stream(dev))
    out = dict(centroids=cen, labels=labels, n_iter=int(st.iter), error=float(st.error), inertia=float(st.inertia),
               trace=trace_t[:int(st.iter)] if trace else None, done=bool(st.done))
    if timing:
        out["assign_ms"], out["assign_launches"] = float(tm.assign_ms), int(tm.assign_launches)
        out["first_assign_ms"], out["assign_iterations"] = float(tm.first_assign_ms), int(tm.iterations)
    return out


def kmeans_fit_batch(X, centroids, max_iter=100, tol=1e-4, want_labels=False):
    """``B`` independent Lloyd fits in one call, each stopping on its own error (the n_init initialisations of the
    sklearn recipe, anchor.py:65-71): X (d,N) shared by all problems or (B,d,N); centroids (B,d,K) initial -> final.
    Returns dict(centroids (B,d,K), labels (B,N) int64 | None, n_iter [B], error [B], inertia [B], done [B])."""
    dev = L.require_device(X)
    X, centroids = _dev_args(dev, X, centroids)
    B, d, K = centroids.shape
    n = X.shape[-1]
    x_stride = 0 if X.dim() == 2 else d * n
    nbytes = L.lib().et_kmeans_batch_workspace_bytes(n, int(d), int(K), B)
    if nbytes == 0:
        raise ValueError(f"k-means dimensions out of range: d={d}, K={K}")
    ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    cen = centroids.clone()
    labels = torch.empty((B, n), device=dev, dtype=torch.int64) if want_labels else None
    states = (L.KMeansState * B)()
    L.call("et_kmeans_fit_batch", L.ptr(X), x_stride, n, int(d), int(K), B, int(max_iter), float(tol), L.ptr(cen),
           L.ptr(labels), states, L.ptr(ws), ws.numel(), L.stream(dev))
    return dict(centroids=cen, labels=labels, n_iter=[int(s_.iter) for s_ in states], error=[float(s_.error) for s_ in states],
                inertia=[float(s_.inertia) for s_ in states], done=[bool(s_.done) for s_ in states])


def kmeanspp_seed_batch(X, K, uniforms):
    """``B`` greedy k-means++ seedings of the same X (d,N) side by side (the y dimension of the same 4K-1 launches):
    uniforms (B, 1 + (K-1)*n_trials) float64 -> (centers (B,d,K), indices (B,K) int64).  No host synchronisation."""
    dev = L.require_device(X)
    (X,) = _dev_args(dev, X)
    uniforms = L.on_device(uniforms, dev, torch.float64)
    d, n = X.shape
    nt = kmeanspp_trials(K)
    B = uniforms.shape[0]
    if uniforms.dim() != 2 or uniforms.shape[1] != 1 + (K - 1) * nt:
        raise ValueError(f"k-means++ seeding of {K} centres consumes {1 + (K - 1) * nt} draws per initialisation")
    nbytes = L.lib().et_kmeanspp_batch_workspace_bytes(n, d, nt, B)
    if nbytes == 0:
        raise ValueError(f"k-means++ dimensions out of range: N={n}, d={d}, K={K}")
    ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    centers = torch.empty((B, d, K), device=dev)
    indices = torch.empty((B, K), device=dev, dtype=torch.int64)
    L.call("et_kmeanspp_seed_batch", L.ptr(X), n, d, int(K), nt, L.ptr(uniforms), B, L.ptr(centers), L.ptr(indices),
           L.ptr(ws), ws.numel(), L.stream(dev))
    return centers, indices


def kmeans_joint_done(state_ptrs, n_problems, tol):
    """kmeans.py:228-240 for a batch of problems run through the step API: ``state_ptrs`` = int64 device tensor of the
    problems' state-block addresses; sets every state's ``done`` from the SUM of their errors."""
    dev = L.require_device(state_ptrs)
    L.call("et_kmeans_joint_done", L.ptr(state_ptrs), int(n_problems), float(tol), L.stream(dev))


def kmeans_predict(X, centroids, want_maxsims=True):
    """kmeans.py:143-158 / 261-272: labels (N,) int64 and max similarity (N,); batched (B,d,N), (B,d,K) -> (B,N) in one
    launch."""
    dev = L.require_device(X)
    X, centroids = _dev_args(dev, X, centroids)
    if centroids.dim() == 3:  # a batch of centroid sets: on their own points (B,d,N) or all on the same points (d,N)
        B = centroids.shape[0]
        d, n = X.shape[-2], X.shape[-1]
        labels = torch.empty((B, n), device=dev, dtype=torch.int64)
        maxsims = torch.empty((B, n), device=dev) if want_maxsims else None
        L.call("et_kmeans_predict_batch", L.ptr(X), d * n if X.dim() == 3 else 0, B, n, d, L.ptr(centroids),
               centroids.shape[2], L.ptr(labels), L.ptr(maxsims), L.stream(dev))
        return labels, maxsims
    d, n = X.shape
    labels = torch.empty((n,), device=dev, dtype=torch.int64)
    maxsims = torch.empty((n,), device=dev) if want_maxsims else None
    L.call("et_kmeans_predict", L.ptr(X), n, d, L.ptr(centroids), centroids.shape[1], L.ptr(labels), L.ptr(maxsims),
           L.stream(dev))
    return labels, maxsims


# ------------------------------------- BatchKMeans in the reference's own summation orders (opt-in)
def _reforder_ws(n, d, K, dev):
    nbytes = L.lib().et_kmeans_reforder_workspace_bytes(n, int(d), int(K))
    if nbytes == 0:
        raise ValueError(f"k-means dimensions out of range: d={d} (<= {L.KMEANS_MAX_D}), K={K} (<= {L.KMEANS_MAX_CLUSTERS})")
    return torch.empty((nbytes,), device=dev, dtype=torch.uint8)


def euc_sim_reference_order(a, b):
    """kmeans.py:59-76 with the norms summed in torch's own order: a (d,m), b (d,n) -> (m,n), every bit the reference's."""
    dev = L.require_device(a, b)
    a, b = _dev_args(dev, a, b)
    d, m = a.shape
    n = b.shape[1]
    y = torch.empty((m, n), device=dev)
    L.call("et_euc_sim_reforder", L.ptr(a), L.ptr(b), d, m, n, L.ptr(y), L.stream(dev))
    return y


def kmeans_init_farthest_reference_order(X, K, first_index):
    """kmeans.py:78-112 literally (euc_sim against all current centroids at every step, torch's norm orders)."""
    dev = L.require_device(X)
    (X,) = _dev_args(dev, X)
    d, n = X.shape
    ws = _reforder_ws(n, d, K, dev)
    c0 = torch.empty((d, K), device=dev)
    L.call("et_kmeans_init_farthest_reforder", L.ptr(X), n, d, int(K), int(first_index), L.ptr(c0), L.ptr(ws), ws.numel(),
           L.stream(dev))
    return c0


def kmeans_predict_reference_order(X, centroids):
    """kmeans.py:143-158 with torch's norm orders: labels (N,) int64, maxsims (N,)."""
    dev = L.require_device(X)
    X, centroids = _dev_args(dev, X, centroids)
    d, n = X.shape
    K = centroids.shape[1]
    ws = _reforder_ws(n, d, K, dev)
    labels = torch.empty((n,), device=dev, dtype=torch.int64)
    maxsims = torch.empty((n,), device=dev)
    L.call("et_kmeans_predict_reforder", L.ptr(X), n, d, L.ptr(centroids), K, L.ptr(labels), L.ptr(maxsims), L.ptr(ws),
           ws.numel(), L.stream(dev))
    return labels, maxsims


def kmeans_fit_reference_order(X, centroids, max_iter=100, tol=1e-4, trace=True, timing=False):
    """kmeans.py:228-240 with the cluster sums, norms and error in the reference's fp32 orders (single GPU).
    Same return dict as :func:`kmeans_fit`.  d = 6, K <= 32, N >= 1024: one launch per iteration (the parallel form of
    ATen's cascade, csrc/et_kmeans_reforder.hip, namespace fast); any other shape: the plain kernels."""
    return kmeans_fit_reference_order_batch(X[None], centroids[None], max_iter, tol, trace=trace, timing=timing)[0]


def kmeans_fit_reference_order_batch(X, centroids, max_iter=100, tol=1e-4, trace=True, timing=False):
    """BatchKMeans.fit's loop (kmeans.py:228-240) for X (l, d, N), centroids (l, d, K) in the reference's summation
    orders: ALL problems iterate in one loop and stop together on the error summed over the whole (l, d, K) tensor.
    Returns one dict per problem (all with the same n_iter / error)."""
    dev = L.require_device(X)
    X, centroids = _dev_args(dev, X, centroids)
    nb, d, n = X.shape
    K = centroids.shape[2]
    nbytes = L.lib().et_kmeans_reforder_batch_workspace_bytes(n, int(d), int(K), nb)
    if nbytes == 0:
        if nb > 1:
            raise NotImplementedError(f"sums='reference-order' with l = {nb} > 1 problems takes d = 6, K <= 32, 1024 <= N < 2^29, "
                                      f"l <= 64 (got d={d}, K={K}, N={n})")
        raise ValueError(f"k-means dimensions out of range: d={d} (<= {L.KMEANS_MAX_D}), K={K} (<= {L.KMEANS_MAX_CLUSTERS})")
    ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    cen = centroids.clone()
    labels = torch.empty((nb, n), device=dev, dtype=torch.int64)
    trace_t = torch.zeros((nb, max_iter, 2), device=dev) if trace else None
    st = (L.KMeansState * nb)()
    tm = L.KMeansTiming() if timing else None
    L.call("et_kmeans_fit_reforder_batch", L.ptr(X), d * n, n, d, K, nb, int(max_iter), float(tol), L.ptr(cen),
           L.ptr(labels), L.ptr(trace_t), st, C.byref(tm) if timing else None, L.ptr(ws), ws.numel(), L.stream(dev))
    out = []
    for b in range(nb):
        r = dict(centroids=cen[b], labels=labels[b], n_iter=int(st[b].iter), error=float(st[b].error),
                 inertia=float(st[b].inertia), trace=trace_t[b, :int(st[b].iter)] if trace else None, done=bool(st[b].done))
        if timing:
            r["timing"] = dict(loop_ms=float(tm.assign_ms), launches=int(tm.assign_launches), iterations=int(tm.iterations))
        out.append(r)
    return out


def reference_order_shard_sizes(n_total, world, d=6, K=20):
    """How to split n_total points over `world` ranks so that sums="reference-order" gives the single-GPU bits: every
    rank before the last non-empty one holds whole level-2 blocks of ATen's cascade (include/eigentraj.h,
    et_kmeans_fit_reforder_sharded); as even as that allows.  -> list of `world` sizes (trailing ranks may be empty)."""
    block = int(L.lib().et_kmeans_reforder_shard_block(int(n_total), int(d), int(K)))
    if block == 0:
        raise NotImplementedError(f"sharded sums='reference-order' takes d = 6, K <= 32, 1024 <= N < 2^29 (got d={d}, K={K}, N={n_total})")
    blocks = -(-int(n_total) // block)
    per = -(-blocks // int(world))
    sizes, left = [], int(n_total)
    for _ in range(int(world)):
        take = min(left, per * block)
        sizes.append(take)
        left -= take
    return sizes


def kmeans_fit_reference_order_sharded(X_local, centroids, n_locals, rank, comm=None, max_iter=100, tol=1e-4, trace=True):
    """kmeans.py:228-240 in the reference's fp32 summation orders over points split across ranks (n_locals: every rank's
    size, see :func:`reference_order_shard_sizes`; comm: a dist.Communicator or None for one rank).  The same centroids,
    labels, error and iteration count as :func:`kmeans_fit_reference_order` on the whole array, on every rank."""
    dev = L.require_device(centroids)
    X_local, centroids = _dev_args(dev, X_local, centroids)
    d, n = X_local.shape
    K = centroids.shape[1]
    sizes = (C.c_int64 * len(n_locals))(*[int(v) for v in n_locals])
    if int(n_locals[rank]) != n:
        raise ValueError(f"n_locals[{rank}] = {n_locals[rank]} but this rank holds {n} points")
    nbytes = L.lib().et_kmeans_reforder_sharded_workspace_bytes(sizes, len(n_locals), int(rank), int(d), int(K))
    if nbytes == 0:
        raise NotImplementedError("sharded sums='reference-order': d = 6, K <= 32, 1024 <= N_total < 2^29 and whole level-2 "
                                  f"blocks on every rank before the last (got d={d}, K={K}, sizes={list(n_locals)})")
    ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    cen = centroids.clone()
    labels = torch.empty((n,), device=dev, dtype=torch.int64)
    trace_t = torch.zeros((max_iter, 2), device=dev) if trace else None
    st = L.KMeansState()
    L.call("et_kmeans_fit_reforder_sharded", L.ptr(X_local) if n else None, sizes, len(n_locals), int(rank), int(d), int(K),
           int(max_iter), float(tol), L.ptr(cen), L.ptr(labels) if n else None, L.ptr(trace_t), C.byref(st), L.ptr(ws),
           ws.numel(), comm.handle if comm is not None else None, L.stream(dev))
    return dict(centroids=cen, labels=labels, n_iter=int(st.iter), error=float(st.error), inertia=float(st.inertia),
                trace=trace_t[:int(st.iter)] if trace else None, done=bool(st.done))


# ---------------------------------------------------- sklearn-recipe anchors (anchor.py:65-71)
def center_columns(X, rel_tol=1e-4):
    """KMeans.fit's pre-processing on a COPY of X (d,N): -> (X - mean (d,N), mean (d,), tol (1,) = rel_tol * mean(var))
    all on the device, in numpy's float32 reduction order (csrc/et_kmeanspp.hip)."""
    dev = L.require_device(X)
    Xc = L.on_device(X, dev).clone()
    d, n = Xc.shape
    mean = torch.empty((d,), device=dev)
    tol = torch.empty((1,), device=dev)
    ws = torch.empty((2 * L.KMEANS_MAX_D,), device=dev)
    L.call("et_center_columns", L.ptr(Xc), n, d, float(rel_tol), L.ptr(mean), L.ptr(tol), L.ptr(ws), ws.numel() * 4,
           L.stream(dev))
    return Xc, mean, tol


def kmeanspp_trials(K):
    """sklearn's number of candidates per centre: 2 + floor(ln K)."""
    import math
    return 2 + int(math.log(K))


def kmeanspp_seed(X, K, uniforms, workspace=None):
    """Greedy k-means++ seeding of X (d,N) with the float64 draws ``uniforms`` (1 + (K-1)*n_trials,) on the device
    -> (centers (d,K), indices (K,) int64).  No host synchronisation."""
    dev = L.require_device(X)
    (X,) = _dev_args(dev, X)
    uniforms = L.on_device(uniforms, dev, torch.float64)
    d, n = X.shape
    nt = kmeanspp_trials(K)
    if uniforms.numel() != 1 + (K - 1) * nt:
        raise ValueError(f"k-means++ seeding of {K} centres consumes {1 + (K - 1) * nt} draws, got {uniforms.numel()}")
    if workspace is None:
        nbytes = L.lib().et_kmeanspp_workspace_bytes(n, d, nt)
        if nbytes == 0:
            raise ValueError(f"k-means++ dimensions out of range: N={n}, d={d}, K={K}")
        workspace = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    centers = torch.empty((d, K), device=dev)
    indices = torch.empty((K,), device=dev, dtype=torch.int64)
    L.call("et_kmeanspp_seed", L.ptr(X), n, d, int(K), nt, L.ptr(uniforms), L.ptr(centers), L.ptr(indices), L.ptr(workspace),
           workspace.numel(), L.stream(dev))
    return centers, indices


class KMeansShard:
    """Step-wise Lloyd iteration on one shard of the points (the sharded / multi-GPU form).

    ``scan`` -> [all-reduce MAX of ``state_f64[0]`` and ``state_i64[7]``] -> ``begin`` ->
    repeat { ``assign`` -> [all-reduce SUM of the int64 partials] -> ``update`` } -> ``labels``.
    Everything stays on the device; ``state`` is read back only when the caller asks.
    """

    def __init__(self, X, K):
        self.dev = L.require_device(X)
        self.X = L.on_device(X, self.dev)
        self.d, self.n = self.X.shape
        self.K = int(K)
        self.ws = kmeans_workspace(self.n, self.d, self.K, self.dev)
        self.state = torch.zeros((L.STATE_BYTES // 8,), device=self.dev, dtype=torch.int64)
        self.partials = torch.zeros((L.lib().et_kmeans_partials_len(self.d, self.K),), device=self.dev,
                                    dtype=torch.int64)
        self.labels_u8 = torch.zeros((max(self.n, 1) + 3,), device=self.dev, dtype=torch.uint8)
        self.best = torch.empty((max(self.n, 1),), device=self.dev)
        self.cand = torch.zeros((8 + 4 * L.KMEANS_MAX_D,), device=self.dev, dtype=torch.uint8)

    @property
    def state_f64(self):
        return self.state.view(torch.float64)

    def scan(self):
        L.call("et_kmeans_scan", L.ptr(self.X), self.n, self.d, L.ptr(self.state), L.stream(self.dev))

    def begin(self, n_total, centroids):
        L.call("et_kmeans_begin", L.ptr(self.state), int(n_total), L.ptr(centroids), self.d, self.K, L.stream(self.dev))

    def init_step(self, i, C0, index_base):
        """candidate record of farthest-first step i: uint8 tensor {key u64, d floats}."""
        L.call("et_kmeans_init_step", L.ptr(self.X), self.n, self.d, self.K, int(i), L.ptr(C0), L.ptr(self.best),
               int(index_base), L.ptr(self.cand), L.ptr(self.ws), self.ws.numel(), L.stream(self.dev))
        return self.cand

    def init_select(self, cands, n_cands, stride, col, C0):
        """Column ``col`` of C0 <- the candidate record with the smallest key among ``n_cands`` gathered records."""
        L.call("et_kmeans_init_select", L.ptr(cands), int(n_cands), int(stride), self.d, self.K, int(col), L.ptr(C0),
               L.stream(self.dev))

    def post_state(self):
        """Start an asynchronous copy of the state block to pinned host memory; -> handle for ``wait_state``."""
        if not hasattr(self, "_pins"):
            self._pins, self._pin_i = [torch.empty((L.STATE_BYTES // 8,), dtype=torch.int64).pin_memory() for _ in range(4)], 0
        host = self._pins[self._pin_i % 4]
        self._pin_i += 1
        host.copy_(self.state, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev))
        return host, ev

    def wait_state(self, handle):
        host, ev = handle
        ev.synchronize()
        return L.KMeansState.from_buffer_copy(host.numpy().tobytes())

    def gather_point(self, local_index):
        pt = torch.empty((self.d,), device=self.dev)
        L.call("et_kmeans_gather_point", L.ptr(self.X), self.n, self.d, int(local_index), L.ptr(pt), L.stream(self.dev))
        return pt

    def assign(self, centroids, given_labels=None):
        L.call("et_kmeans_assign_accumulate", L.ptr(self.X), self.n, self.d, self.K, L.ptr(self.state), L.ptr(centroids),
               L.ptr(given_labels), L.ptr(self.labels_u8), L.ptr(self.partials), L.ptr(self.ws), self.ws.numel(),
               L.stream(self.dev))
        return self.partials

    def update(self, partials, centroids, tol, trace=None):
        L.call("et_kmeans_update", L.ptr(self.state), L.ptr(partials), self.d, self.K, float(tol), L.ptr(centroids),
               L.ptr(trace), L.stream(self.dev))

    def labels(self):
        out = torch.empty((self.n,), device=self.dev, dtype=torch.int64)
        L.call("et_kmeans_labels_i64", L.ptr(self.labels_u8), self.n, L.ptr(out), L.stream(self.dev))
        return out

    def read_state(self):
        """Blocking read-back of the state block -> _lib.KMeansState."""
        host = self.state.cpu().numpy().tobytes()
        return L.KMeansState.from_buffer_copy(host)
