"""Graph-TERN, the predictor of ET-Graph-TERN (baseline/graphtern/model.py: graph_tern_light), inference on HIP kernels.

Same constructor signature and the same sub-module / parameter names as the reference (``tp_mrgcns.{i}.gcn.conv``,
``tp_mrgcns.{i}.tcn.{0,1}``, ``tp_mrgcns.{i}.residual.0``, ``tp_mrgcns.{i}.prelu``, ``tpcnns.{j}.tpcns.0.{0,1}``,
``tpcnns.{j}.cpcns.0.{0,1}``, ``tpcnns.0.restconv.0``, ``tpcnns.{last}.rescconv.0``), so a reference ET-Graph-TERN
checkpoint's ``baseline_model.*`` keys load unchanged (``strict=True``), and the module plugs into
:class:`eigentrajectory_amd.EigenTrajectory` through the existing ``graphtern`` bridge::

    model = EigenTrajectory(GraphTERNLight(n_epgcn=1, n_epcnn=6, input_feat=1, seq_len=hp.k + 2, pred_seq_len=hp.k,
                                           n_smpl=hp.num_samples),
                            get_hook_func("graphtern"), hp).eval()

``forward(S_obs)`` in eval mode is ONE launch of ``et_graphtern_forward_graph`` (csrc/et_graphtern.hip): S_obs
(1, 2, T, N, 1) = [abs, rel] as the bridge's pre-hook builds it -> (1, k, N, S), which the post-hook squeezes.  The weights
are read in place from this module's tensors (a ``load_state_dict``, a ``.to()`` or an in-place edit is seen by the next
call, and by a captured graph's next replay).  ``tp_mrgcns.{i}.prelu`` is a parameter of the reference's state_dict that
its forward never applies (``use_mdn``); it is kept for the checkpoint's sake and not applied here either.
A whole split runs as one launch through :meth:`EigenTrajectory.evaluate_split` /
:func:`eigentrajectory_amd.ops.graphtern_forward_scenes`.
A forward in training mode raises -- unless the instance was switched by
``eigentrajectory_amd.enable_native_training(model)``.  Then a training-mode ``forward(S_obs, keep=None)`` is
``et_graphtern_train_forward_graph`` (csrc/et_graphtern_train.hip, one launch), which is NOT the eval forward:
MultiRelationalGCN applies ``drop_edge(A, 0.8)`` to the float tensor A (1, 4, T, N, N) before ``+ I`` and before the
normalisation, so the degrees change with the mask and each normalised graph is no longer symmetric.  The draw is
:meth:`GraphTERNLight.draw_keep` -- one ``torch.rand((1, 4, T, N, N))``, an entry kept where ``~(rand > 0.8)`` -- unless
``keep`` (uint8, (4, T, N, N), indexed [r, t, w, v]) is given.  The output is differentiable with respect to every parameter
the forward reads (``et_graphtern_backward_graph``, three launches; no input gradient; ``tp_mrgcns.0.prelu.weight.grad``
stays None, as torch leaves it).  The switch is the plain attribute ``native_training`` (no parameter, no buffer, not in
the ``state_dict``, default False).  Trained natively: the family below with ``n_epgcn = 1`` (the only depth ET builds; a
deeper stack needs a gradient through the graph contraction), every ``Dropout.p = 0`` and scenes of at most 512
pedestrians.
Supported family: ``input_feat = 1``, ``seq_len = pred_seq_len + 2``, ``pred_seq_len <= 32``, ``1 <= n_smpl <= 64``,
``1 <= n_epgcn <= 4``, ``2 <= n_epcnn <= 8`` (the hidden width is the reference's constant 16); other shapes construct,
but their forward raises.

The network's graphs hold inverse distances, 1 / |u_i - u_j|, so its output is NOT stable under a change of a coefficient
in the last place: on the same fp32 input this module agrees with the reference to 1e-5, but two projections that differ
by an ulp can move a scene's output by per cent ("Graph-TERN").
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib as L
from ._lib import _p
from ._native_train import train_forward

HIDDEN_FEAT = 16  # model.py:229
KERNEL_SIZE = 3   # model.py:230


class _MultiRelationalGCN(nn.Module):
    """A 1x1 convolution to out * relation channels (channel r * out + c), relation r contracted with its own normalised
    graph."""

    def __init__(self, in_channels, out_channels, kernel_size, relation):
        super().__init__()
        self.kernel_size, self.relation, self.out_channels = kernel_size, relation, out_channels
        self.conv = nn.Conv2d(in_channels, out_channels * relation, kernel_size=(1, 1))


class _STMRGCNBlock(nn.Module):
    """One st_mrgcn block: gcn -> PReLU -> (t, 1) temporal conv (-> dropout, off), + residual.  ``prelu`` exists and is
    unused (use_mdn).  No BatchNorm."""

    def __init__(self, in_channels, out_channels, kernel_size, relation=4):
        super().__init__()
        t_kernel, graph_kernel = kernel_size
        self.prelu = nn.PReLU()
        self.gcn = _MultiRelationalGCN(in_channels, out_channels, graph_kernel, relation)
        self.tcn = nn.Sequential(nn.PReLU(),
                                 nn.Conv2d(out_channels, out_channels, (t_kernel, 1), (1, 1), ((t_kernel - 1) // 2, 0)),
                                 nn.Dropout(0, inplace=True))
        if in_channels != out_channels:
            self.residual = nn.Sequential(nn.Conv2d(in_channels, out_channels, kernel_size=1, stride=(1, 1)))
        else:
            self.residual = None  # identity


class _EPCNN(nn.Module):
    """One epcnn block: a 3x3 convolution with the rows as channels, one with the channels as channels (both replicate
    padded, each followed by PReLU), + residual (identity, or a 1x1 convolution over whichever of the two widths changes)."""

    def __init__(self, obs_seq_len, pred_seq_len, in_channels, out_channels):
        super().__init__()
        self.tpcns = nn.ModuleList([nn.Sequential(
            nn.Conv2d(obs_seq_len, pred_seq_len, 3, padding=1, padding_mode="replicate"), nn.PReLU(),
            nn.Dropout(0, inplace=True))])
        self.cpcns = nn.ModuleList([nn.Sequential(
            nn.Conv2d(in_channels, out_channels, 3, padding=1, padding_mode="replicate"), nn.PReLU(),
            nn.Dropout(0, inplace=True))])
        if in_channels != out_channels:
            self.rescconv = nn.Sequential(nn.Conv2d(in_channels, out_channels, kernel_size=1))
        if obs_seq_len != pred_seq_len:
            self.restconv = nn.Sequential(nn.Conv2d(obs_seq_len, pred_seq_len, kernel_size=1))


class GraphTERNLight(nn.Module):
    r"""baseline/graphtern/model.py's ``graph_tern_light`` (eval-mode inference on the GPU).  ``forward(S_obs)``: S_obs
    (1, 2, T, N, 1) = [abs, rel] as the graphtern bridge's pre-hook builds it -> (1, k, N, S); the post-hook squeezes it."""

    native_training = False  # a plain attribute, set per instance by eigentrajectory_amd.enable_native_training
    #: how enable_native_training ends its refusal of an instance outside the native family
    trains_natively = ("LBEBM, PECNet, SocialImplicitLight, SGCN, SocialSTGCNN, SocialDMRGCN and a GraphTERNLight with "
                       "n_epgcn = 1 and no dropout train natively")
    drop_edge_percent = 0.8  # stmrgcn.py:22: drop_edge(A, 0.8, self.training) keeps an entry where ~(rand > 0.8)

    def __init__(self, n_epgcn=1, n_epcnn=6, input_feat=2, seq_len=8, pred_seq_len=12, n_smpl=20):
        super().__init__()
        self.n_epgcn, self.n_epcnn, self.n_smpl = n_epgcn, n_epcnn, n_smpl
        self.input_feat, self.seq_len, self.pred_seq_len = input_feat, seq_len, pred_seq_len
        self.tp_mrgcns = nn.ModuleList(
            [_STMRGCNBlock(input_feat if i == 0 else HIDDEN_FEAT, HIDDEN_FEAT, (KERNEL_SIZE, seq_len))
             for i in range(max(n_epgcn, 1))])
        blocks = [_EPCNN(seq_len, pred_seq_len, HIDDEN_FEAT, HIDDEN_FEAT)]
        blocks += [_EPCNN(pred_seq_len, pred_seq_len, HIDDEN_FEAT, HIDDEN_FEAT) for _ in range(1, n_epcnn - 1)]
        blocks.append(_EPCNN(pred_seq_len, pred_seq_len, HIDDEN_FEAT, n_smpl))
        self.tpcnns = nn.ModuleList(blocks)

    def et_params(self):
        """-> (et_graphtern_params, device): this module's tensors as the kernel reads them (include/eigentraj.h)."""
        p = L.GraphTERNParams()
        p.n_epgcn, p.n_epcnn, p.input_feat, p.hidden_feat = self.n_epgcn, self.n_epcnn, self.input_feat, HIDDEN_FEAT
        p.seq_len, p.pred_seq_len, p.n_smpl = self.seq_len, self.pred_seq_len, self.n_smpl
        dev = L.module_device("GraphTERNLight", self)
        if (len(self.tp_mrgcns) != self.n_epgcn or len(self.tpcnns) != self.n_epcnn
                or self.n_epgcn > L.GRAPHTERN_MAX_EPGCN or self.n_epcnn > L.GRAPHTERN_MAX_EPCNN):
            return p, dev  # the kernel answers ET_ERR_UNSUPPORTED
        for i, blk in enumerate(self.tp_mrgcns):
            s = p.tp_mrgcns[i]
            s.gcn_w, s.gcn_b = _p(blk.gcn.conv.weight), _p(blk.gcn.conv.bias)
            s.tcn_prelu, s.tcn_w, s.tcn_b = _p(blk.tcn[0].weight), _p(blk.tcn[1].weight), _p(blk.tcn[1].bias)
            if blk.residual is not None:
                s.res_w, s.res_b = _p(blk.residual[0].weight), _p(blk.residual[0].bias)
            s.prelu = _p(blk.prelu.weight)
        for j, blk in enumerate(self.tpcnns):
            t = p.tpcnns[j]
            t.tpcn_w, t.tpcn_b, t.tpcn_a = _p(blk.tpcns[0][0].weight), _p(blk.tpcns[0][0].bias), _p(blk.tpcns[0][1].weight)
            t.cpcn_w, t.cpcn_b, t.cpcn_a = _p(blk.cpcns[0][0].weight), _p(blk.cpcns[0][0].bias), _p(blk.cpcns[0][1].weight)
            if hasattr(blk, "restconv"):
                t.rest_w, t.rest_b = _p(blk.restconv[0].weight), _p(blk.restconv[0].bias)
            if hasattr(blk, "rescconv"):
                t.resc_w, t.resc_b = _p(blk.rescconv[0].weight), _p(blk.rescconv[0].bias)
        return p, dev

    def outside_native_training(self):
        """-> None, or the field that puts this instance outside the family that trains natively, as text"""
        if self.n_epgcn != 1:
            return (f"n_epgcn = {self.n_epgcn} (native: 1; a deeper stack sends a gradient through the graph contraction "
                    "and is out of scope)")
        for field, want in (("input_feat", 1), ("seq_len", self.pred_seq_len + 2)):
            if getattr(self, field) != want:
                return f"{field} = {getattr(self, field)} (native: {want})"
        for field, lo, hi in (("n_epcnn", 2, L.GRAPHTERN_MAX_EPCNN), ("n_smpl", 1, 64), ("pred_seq_len", 1, L.MAX_K)):
            if not lo <= getattr(self, field) <= hi:
                return f"{field} = {getattr(self, field)} (native: {lo} to {hi})"
        for name, m in self.named_modules():
            if isinstance(m, nn.Dropout) and m.p != 0:
                return f"{name}.p = {m.p} (native: 0)"
        return None

    def draw_keep(self, n, device, generator=None):
        """The DropEdge draw of one training-mode forward on ``n`` pedestrians -> uint8 (4, T, n, n), indexed [r, t, w, v]:
        one ``torch.rand((1, 4, T, n, n))``, as the reference's MultiRelationalGCN draws ``rand_like(A)``; an entry is kept
        where ``~(rand > drop_edge_percent)``."""
        draw = torch.rand((1, L.GRAPHTERN_REL, self.seq_len, n, n), device=device, generator=generator)
        return (~(draw > self.drop_edge_percent))[0].to(torch.uint8)

    native_parameters = nn.Module.parameters  # what :mod:`._native_train` differentiates: every parameter

    def native_forward(self, et, S_obs, keep):
        from . import ops
        ws = ops.graphtern_train_workspace(self, S_obs.shape[3], et_params=et)
        return ops.graphtern_train_forward_graph(self, S_obs, ws, keep=keep, et_params=et), (() if ws is None else (ws,))

    def native_backward(self, et, kept, g_out):
        from . import ops
        ws = kept[0] if kept else None
        views = ops.graphtern_grad_views(self, ops.graphtern_backward_graph(self, ws, g_out, et_params=et))
        return [None if name == "tp_mrgcns.0.prelu.weight" else g for name, g in views.items()]  # never applied: no gradient

    def forward(self, S_obs, keep=None):
        if self.training and self.native_training and self.outside_native_training() is None:
            if S_obs.requires_grad:
                raise RuntimeError("GraphTERNLight: no input gradient is built (the graphtern bridge detaches S_obs); an "
                                   "input requires one")
            dev = L.module_device("GraphTERNLight", self)
            S_obs = L.on_device(S_obs, dev)
            if keep is None:
                keep = self.draw_keep(S_obs.shape[3] if S_obs.dim() == 5 else 0, dev)
            return train_forward(self, S_obs, keep)
        if self.training:
            raise RuntimeError("GraphTERNLight: only inference is native (no drop_edge, no dropout); training-mode forward "
                               "and backward are not implemented -- call .eval() first")
        from . import ops
        return ops.graphtern_forward_graph(self, S_obs)
