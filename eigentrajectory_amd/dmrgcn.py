"""DMRGCN, the predictor of ET-DMRGCN (baseline/dmrgcn/predictor.py: social_dmrgcn), inference on HIP kernels.

Same constructor signature and the same sub-module / parameter names as the reference (``st_dmrgcns.{i}.gcns.{r}.conv``,
``st_dmrgcns.{i}.tcn.{0,1}``, ``st_dmrgcns.{i}.residual.0``, ``st_dmrgcns.{i}.prelu``, ``tpcnns.{j}.tpcn.{0,1}.{0,1}``,
``tpcnns.{j}.gtacn.0.{0,1}``, ``tpcnns.0.residual.0``), so a reference ET-DMRGCN checkpoint's ``baseline_model.*`` keys load
unchanged (``strict=True``), and the module plugs into :class:`eigentrajectory_amd.EigenTrajectory` through the existing
``dmrgcn`` bridge::

    model = EigenTrajectory(SocialDMRGCN(n_stgcn=1, n_tpcnn=4, input_feat=1, output_feat=hp.num_samples,
                                         seq_len=hp.k + 2, pred_seq_len=hp.k, kernel_size=3),
                            get_hook_func("dmrgcn"), hp).eval()

``forward(v, a)`` in eval mode is ONE launch of ``et_dmrgcn_forward_graph`` (csrc/et_dmrgcn.hip) and returns ``(out, a)``
as the reference does: v (1, 1, K, N), a (1, 2, K, N, N) = [A_disp, A_dist] as the bridge's pre-hook builds them, out
(1, S, k, N).  The weights are read in place from this module's tensors (a ``load_state_dict``, a ``.to()`` or an in-place
edit is seen by the next call, and by a captured graph's next replay).  ``split`` holds the two disentangling scale sets
(constructor constants of the reference, not part of the state_dict); bin b of a relation is the open interval
``split[r][b] < distance < split[r][b+1]`` (1e10 after the last value), so a distance equal to a split value is in no bin.
A whole split runs as one launch through :meth:`EigenTrajectory.evaluate_split` /
:func:`eigentrajectory_amd.ops.dmrgcn_forward_scenes`.
A forward in training mode raises -- unless the instance was switched by
``eigentrajectory_amd.enable_native_training(model)``.  Then a training-mode ``forward(v, a, keep=None)`` is
``et_dmrgcn_train_forward_graph`` (csrc/et_dmrgcn_train.hip, one launch), which is NOT the eval forward: every
MultiRelationalGCN applies ``drop_edge(A_, 0.8)`` to its clipped 0/1 bin tensor, so each (relation, bin, time row) graph loses
entries independently per direction and is no longer symmetric.  The draw is :meth:`SocialDMRGCN.draw_keep` -- two
``torch.rand((1, 5, K, N, N))`` draws, relation 0 (displacement) first, an entry kept where ``~(rand > 0.8)`` -- unless
``keep`` (uint8, (2, 5, K, N, N), indexed [r, b, t, w, v]) is given.  The output is differentiable with respect to every
parameter (``et_dmrgcn_backward_graph``, three launches; no input gradient).  The switch is the plain attribute
``native_training`` (no parameter, no buffer, not in the ``state_dict``, default False).  Trained natively: the family
below with ``n_stgcn = 1`` (the only depth the reference constructs; deeper stacks would send a gradient through the
Laplacians), every ``Dropout.p = 0`` and scenes of at most 512 pedestrians.
Supported family: ``input_feat = 1``, ``kernel_size = 3``, ``seq_len = pred_seq_len + 2``, ``1 <= output_feat <= 64``,
``pred_seq_len <= 32``, ``1 <= n_stgcn <= 4``, ``1 <= n_tpcnn <= 8``, five ascending non-negative split values per relation;
other shapes construct, but their forward raises.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib as L
from ._lib import _p
from ._native_train import train_forward


class _MultiRelationalGCN(nn.Module):
    """One relation's graph convolution: a 1x1 convolution to out * bins channels (channel b * out + c), bin b contracted
    with its own normalised Laplacian."""

    def __init__(self, in_channels, out_channels, kernel_size, relation):
        super().__init__()
        self.kernel_size, self.relation, self.out_channels = kernel_size, relation, out_channels
        self.conv = nn.Conv2d(in_channels, out_channels * relation, kernel_size=(1, 1))


class _STDMRGCNBlock(nn.Module):
    """One st_dmrgcn block: the two relations' gcns summed -> PReLU -> (t, 1) temporal conv (-> dropout, off), + residual,
    PReLU.  No BatchNorm."""

    def __init__(self, in_channels, out_channels, kernel_size, split):
        super().__init__()
        t_kernel, graph_kernel = kernel_size
        self.gcns = nn.ModuleList([_MultiRelationalGCN(in_channels, out_channels, graph_kernel, len(s)) for s in split])
        self.tcn = nn.Sequential(nn.PReLU(),
                                 nn.Conv2d(out_channels, out_channels, (t_kernel, 1), (1, 1), ((t_kernel - 1) // 2, 0)),
                                 nn.Dropout(0, inplace=True))
        if in_channels != out_channels:
            self.residual = nn.Sequential(nn.Conv2d(in_channels, out_channels, kernel_size=1, stride=(1, 1)))
        else:
            self.residual = None  # identity
        self.prelu = nn.PReLU()


class _TPCNN(nn.Module):
    """One tpcnn block: two 3x3 convolutions + PReLU with residuals, then the global temporal aggregation."""

    def __init__(self, seq_len, pred_seq_len, output_feat, kernel_size=3):
        super().__init__()
        self.tpcn = nn.ModuleList([
            nn.Sequential(nn.Conv2d(seq_len if m == 0 else pred_seq_len, pred_seq_len, kernel_size, padding=1), nn.PReLU(),
                          nn.Dropout(0, inplace=True)) for m in range(2)])
        self.gtacn = nn.ModuleList([nn.Sequential(nn.Conv2d(output_feat, output_feat, (pred_seq_len, 1), padding=0),
                                                  nn.PReLU(), nn.Dropout(0, inplace=True))])
        if seq_len != pred_seq_len:
            self.residual = nn.Sequential(nn.Conv2d(seq_len, pred_seq_len, kernel_size=1))
        else:
            self.residual = None  # identity


class SocialDMRGCN(nn.Module):
    r"""baseline/dmrgcn/predictor.py's ``social_dmrgcn`` (eval-mode inference on the GPU).  ``forward(v, a)``: v (1, 1, K, N),
    a (1, 2, K, N, N) as the dmrgcn bridge's pre-hook builds them -> ``(out (1, S, k, N), a)``; the post-hook takes [0]."""

    native_training = False  # a plain attribute, set per instance by eigentrajectory_amd.enable_native_training
    #: how enable_native_training ends its refusal of an instance outside the native family
    trains_natively = ("LBEBM, PECNet, SocialImplicitLight, SGCN, SocialSTGCNN and a SocialDMRGCN with n_stgcn = 1 and no dropout train "
                       "natively")
    drop_edge_percent = 0.8  # dmrgcn.py:68: drop_edge(A, 0.8, self.training) keeps an entry where ~(rand > 0.8)

    def __init__(self, n_stgcn=1, n_tpcnn=4, input_feat=2, output_feat=5, seq_len=8, pred_seq_len=12, kernel_size=3):
        super().__init__()
        self.n_stgcn, self.n_tpcnn = n_stgcn, n_tpcnn
        self.input_feat, self.output_feat = input_feat, output_feat
        self.seq_len, self.pred_seq_len, self.kernel_size = seq_len, pred_seq_len, kernel_size
        #: disentangling scale sets [A_disp, A_dist] (predictor.py:68-69)
        self.split = [[0, 1 / 4, 2 / 4, 3 / 4, 1], [0, 1 / 2, 1, 2, 4]]
        self.st_dmrgcns = nn.ModuleList(
            [_STDMRGCNBlock(input_feat if i == 0 else output_feat, output_feat, (kernel_size, seq_len), self.split)
             for i in range(n_stgcn)])
        self.tpcnns = nn.ModuleList(
            [_TPCNN(seq_len if j == 0 else pred_seq_len, pred_seq_len, output_feat) for j in range(n_tpcnn)])

    def et_params(self):
        """-> (et_dmrgcn_params, device): this module's tensors as the kernel reads them (include/eigentraj.h)."""
        p = L.DMRGCNParams()
        p.n_stgcn, p.n_tpcnn, p.input_feat = self.n_stgcn, self.n_tpcnn, self.input_feat
        p.output_feat, p.seq_len, p.pred_seq_len, p.kernel_size = (self.output_feat, self.seq_len, self.pred_seq_len,
                                                                   self.kernel_size)
        dev = L.module_device("SocialDMRGCN", self)
        if len(self.split) != 2 or any(len(s) != L.DMRGCN_BINS for s in self.split):
            raise L.ETLibraryError(f"SocialDMRGCN: the kernel takes two relations of {L.DMRGCN_BINS} split values each")
        for r, s in enumerate(self.split):
            for b, val in enumerate(s):
                p.split[r][b] = float(val)
        if self.n_stgcn > L.DMRGCN_MAX_STGCN or self.n_tpcnn > L.DMRGCN_MAX_TPCNN:
            return p, dev  # the kernel answers ET_ERR_UNSUPPORTED
        for i, blk in enumerate(self.st_dmrgcns):
            s = p.st_dmrgcns[i]
            for r, g in enumerate(blk.gcns):
                s.gcn_w[r], s.gcn_b[r] = _p(g.conv.weight), _p(g.conv.bias)
            s.tcn_prelu, s.tcn_w, s.tcn_b = _p(blk.tcn[0].weight), _p(blk.tcn[1].weight), _p(blk.tcn[1].bias)
            if blk.residual is not None:
                s.res_w, s.res_b = _p(blk.residual[0].weight), _p(blk.residual[0].bias)
            s.prelu = _p(blk.prelu.weight)
        for j, blk in enumerate(self.tpcnns):
            t = p.tpcnns[j]
            for m in range(2):
                t.conv_w[m], t.conv_b[m], t.conv_a[m] = (_p(blk.tpcn[m][0].weight), _p(blk.tpcn[m][0].bias),
                                                         _p(blk.tpcn[m][1].weight))
            t.gta_w, t.gta_b, t.gta_a = _p(blk.gtacn[0][0].weight), _p(blk.gtacn[0][0].bias), _p(blk.gtacn[0][1].weight)
            if blk.residual is not None:
                t.res_w, t.res_b = _p(blk.residual[0].weight), _p(blk.residual[0].bias)
        return p, dev

    def outside_native_training(self):
        """-> None, or the field that puts this instance outside the family that trains natively, as text"""
        if self.n_stgcn != 1:
            return (f"n_stgcn = {self.n_stgcn} (native: 1; deeper stacks send a gradient through the Laplacian "
                    "contraction and are out of scope)")
        for field, want in (("input_feat", 1), ("kernel_size", 3), ("seq_len", self.pred_seq_len + 2)):
            if getattr(self, field) != want:
                return f"{field} = {getattr(self, field)} (native: {want})"
        for field, hi in (("n_tpcnn", L.DMRGCN_MAX_TPCNN), ("output_feat", 64), ("pred_seq_len", L.MAX_K)):
            if not 1 <= getattr(self, field) <= hi:
                return f"{field} = {getattr(self, field)} (native: 1 to {hi})"
        for name, m in self.named_modules():
            if isinstance(m, nn.Dropout) and m.p != 0:
                return f"{name}.p = {m.p} (native: 0)"
        return None

    def draw_keep(self, n, device, generator=None):
        """The DropEdge draw of one training-mode forward on ``n`` pedestrians -> uint8 (2, 5, K, n, n), indexed
        [r, b, t, w, v]: one ``torch.rand((1, 5, K, n, n))`` per relation, r = 0 (displacement) first, as the reference's two
        MultiRelationalGCNs draw ``rand_like(A_)``; an entry is kept where ``~(rand > drop_edge_percent)``."""
        shape = (1, L.DMRGCN_BINS, self.seq_len, n, n)
        draws = [torch.rand(shape, device=device, generator=generator) for _ in range(2)]
        return torch.cat([~(d > self.drop_edge_percent) for d in draws]).to(torch.uint8)

    native_parameters = nn.Module.parameters  # what :mod:`._native_train` differentiates: every parameter

    def native_forward(self, et, v, a, keep):
        from . import ops
        ws = ops.dmrgcn_train_workspace(self, v.shape[-1], et_params=et)
        return ops.dmrgcn_train_forward_graph(self, v, a, ws, keep=keep, et_params=et), (() if ws is None else (ws,))

    def native_backward(self, et, kept, g_out):
        from . import ops
        ws = kept[0] if kept else None
        return ops.dmrgcn_grad_views(self, ops.dmrgcn_backward_graph(self, ws, g_out, et_params=et)).values()

    def forward(self, v, a, keep=None):
        if self.training and self.native_training and self.outside_native_training() is None:
            if v.requires_grad or a.requires_grad:
                raise RuntimeError("SocialDMRGCN: no input gradient is built (the dmrgcn bridge detaches v); an input "
                                   "requires one")
            dev = L.module_device("SocialDMRGCN", self)
            v, a = (L.on_device(t, dev) for t in (v, a))
            if keep is None:
                keep = self.draw_keep(v.shape[-1], dev)
            return train_forward(self, v, a, keep), a
        if self.training:
            raise RuntimeError("SocialDMRGCN: only inference is native (no drop_edge, no dropout); training-mode forward and "
                               "backward are not implemented -- call .eval() first")
        from . import ops
        return ops.dmrgcn_forward_graph(self, v, a), a
