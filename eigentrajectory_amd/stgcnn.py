"""Social-STGCNN, the predictor of ET-STGCNN (baseline/stgcnn/model.py: social_stgcnn), inference on HIP kernels.

Same constructor signature and the same sub-module / parameter / buffer names as the reference (``st_gcns.{i}.gcn.conv``,
``st_gcns.{i}.tcn.{0,1,2,3}``, ``st_gcns.{i}.residual.{0,1}``, ``st_gcns.{i}.prelu``, ``tpcnns.{j}``, ``tpcnn_ouput``,
``prelus.{j}``), so a reference ET-STGCNN checkpoint's ``baseline_model.*`` keys load unchanged, and the module plugs into
:class:`eigentrajectory_amd.EigenTrajectory` through the existing ``stgcnn`` bridge::

    model = EigenTrajectory(SocialSTGCNN(n_stgcnn=1, n_txpcnn=5, input_feat=1, output_feat=hp.num_samples,
                                         seq_len=hp.k + 2, pred_seq_len=hp.k, kernel_size=3),
                            get_hook_func("stgcnn"), hp).eval()

``forward(v, a)`` in eval mode is ONE launch of ``et_stgcnn_forward_graph`` (csrc/et_stgcnn.hip): BatchNorm uses its
running statistics, dropout is off, the weights are read in place from this module's tensors (a ``load_state_dict``, a
``.to()`` or an in-place edit is seen by the next call, and by a captured graph's next replay).  A whole split runs as one
launch through :meth:`EigenTrajectory.evaluate_split` / :func:`eigentrajectory_amd.ops.stgcnn_forward_scenes`.
A forward in training mode raises -- unless the instance was switched by
``eigentrajectory_amd.enable_native_training(model)``.  Then a training-mode ``forward(v, a)`` is
``et_stgcnn_train_forward_graph`` (csrc/et_stgcnn_train.hip, two launches), which is NOT the eval forward: ``tcn.0``,
``tcn.3`` and ``residual.1`` normalise with the scene's batch statistics (mean and biased variance per channel over the K N
values) and update ``running_mean`` / ``running_var`` / ``num_batches_tracked`` as torch does, in the forward, whether or
not a backward follows.  The output is differentiable with respect to every parameter (``et_stgcnn_backward_graph``, two
launches; no input gradient: the stgcnn bridge detaches v).  ``tcn.2.bias`` and ``residual.0.bias`` feed a BatchNorm
directly and get an exact zero; ``tpcnns[n_txpcnn-1]`` / ``prelus[n_txpcnn-1]``, which the forward never reads when
``n_txpcnn >= 2``, keep ``.grad = None`` as in the reference.  The switch is the plain attribute ``native_training`` (no
parameter, no buffer, not in the ``state_dict``, default False).  Trained natively: the family below with ``n_stgcnn = 1``
(the only depth the reference constructs; deeper stacks would send a gradient through the Laplacian contraction),
``graph_per_time_row=False``, affine BatchNorms that track running statistics with one float momentum and one eps, and
``tcn[4].p = 0``.
Supported family: ``input_feat = 1``, ``kernel_size = 3``, ``seq_len = pred_seq_len + 2``, ``1 <= output_feat <= 64``,
``pred_seq_len <= 32``, ``1 <= n_stgcnn, n_txpcnn <= 8``; other shapes construct, but their forward raises.

``SocialSTGCNN(..., graph_per_time_row=True)`` is baseline/gpgraphstgcnn/model_baseline.py's variant -- the original
Social-STGCNN gcn, the base of :class:`eigentrajectory_amd.gpgraph.GPGraphSTGCNN`: ``gcn.conv`` has ``output_feat`` channels
(not ``output_feat * seq_len``) and time row t is contracted with its own graph only (``einsum('nctv,tvw->nctw')``).  It runs
only as the three passes of GPGraphSTGCNN's call; its own forward raises.
"""
from __future__ import annotations

import torch.nn as nn

from . import _lib as L
from ._lib import _p
from ._native_train import train_forward


class _GraphConv(nn.Module):
    """The gcn of an st_gcn block: a 1x1 convolution to out * K channels, contracted with the (K, V, V) graph."""

    def __init__(self, in_channels, out_channels, kernel_size, per_time_row=False):
        super().__init__()
        self.kernel_size = kernel_size
        self.conv = nn.Conv2d(in_channels, out_channels * (1 if per_time_row else kernel_size), kernel_size=(1, 1))


class _STGCNBlock(nn.Module):
    """One st_gcn block: gcn -> BN -> PReLU -> (t, 1) temporal conv -> BN (-> dropout, off), + residual, PReLU."""

    def __init__(self, in_channels, out_channels, kernel_size, per_time_row=False):
        super().__init__()
        t_kernel, graph_kernel = kernel_size
        self.gcn = _GraphConv(in_channels, out_channels, graph_kernel, per_time_row)
        self.tcn = nn.Sequential(nn.BatchNorm2d(out_channels), nn.PReLU(),
                                 nn.Conv2d(out_channels, out_channels, (t_kernel, 1), (1, 1), ((t_kernel - 1) // 2, 0)),
                                 nn.BatchNorm2d(out_channels), nn.Dropout(0.0, inplace=True))
        if in_channels != out_channels:
            self.residual = nn.Sequential(nn.Conv2d(in_channels, out_channels, kernel_size=1, stride=(1, 1)),
                                          nn.BatchNorm2d(out_channels))
        else:
            self.residual = None  # identity
        self.prelu = nn.PReLU()


class SocialSTGCNN(nn.Module):
    r"""baseline/stgcnn/model.py's ``social_stgcnn`` (eval-mode inference on the GPU).  ``forward(v, a)``: v (1, 1, K, N),
    a (K, N, N) as the stgcnn bridge's pre-hook builds them -> (1, S, k, N), the raw output the post-hook permutes."""

    native_training = False  # a plain attribute, set per instance by eigentrajectory_amd.enable_native_training
    #: how enable_native_training ends its refusal of an instance outside the native family
    trains_natively = ("LBEBM, PECNet, SocialImplicitLight, SGCN and a SocialSTGCNN with n_stgcnn = 1 and graph_per_time_row = False "
                       "train natively")

    def __init__(self, n_stgcnn=1, n_txpcnn=1, input_feat=2, output_feat=5, seq_len=8, pred_seq_len=12, kernel_size=3,
                 graph_per_time_row=False):
        super().__init__()
        self.n_stgcnn, self.n_txpcnn, self.graph_per_time_row = n_stgcnn, n_txpcnn, bool(graph_per_time_row)
        self.input_feat, self.output_feat = input_feat, output_feat
        self.seq_len, self.pred_seq_len, self.kernel_size = seq_len, pred_seq_len, kernel_size
        self.st_gcns = nn.ModuleList(
            [_STGCNBlock(input_feat if i == 0 else output_feat, output_feat, (kernel_size, seq_len), self.graph_per_time_row)
             for i in range(n_stgcnn)])
        self.tpcnns = nn.ModuleList(
            [nn.Conv2d(seq_len if j == 0 else pred_seq_len, pred_seq_len, 3, padding=1) for j in range(n_txpcnn)])
        self.tpcnn_ouput = nn.Conv2d(pred_seq_len, pred_seq_len, 3, padding=1)  # (sic: the reference's name)
        self.prelus = nn.ModuleList([nn.PReLU() for _ in range(n_txpcnn)])

    def et_params(self):
        """-> (et_stgcnn_params, device): this module's tensors as the kernel reads them (include/eigentraj.h)."""
        p = L.STGCNNParams()
        p.n_stgcnn, p.n_txpcnn, p.input_feat = self.n_stgcnn, self.n_txpcnn, self.input_feat
        p.output_feat, p.seq_len, p.pred_seq_len, p.kernel_size = (self.output_feat, self.seq_len, self.pred_seq_len,
                                                                   self.kernel_size)
        dev = L.module_device("SocialSTGCNN", self, buffers=True)
        bns = [m for m in self.modules() if isinstance(m, nn.BatchNorm2d)]
        eps = {float(m.eps) for m in bns}
        if len(eps) != 1 or any(m.running_mean is None or m.weight is None for m in bns):
            raise L.ETLibraryError("SocialSTGCNN: the kernel takes one BatchNorm eps and affine BatchNorms with running "
                                   "statistics")
        p.bn_eps = eps.pop()
        if self.n_stgcnn > L.STGCNN_MAX_LAYERS or self.n_txpcnn > L.STGCNN_MAX_LAYERS:
            return p, dev  # the kernel answers ET_ERR_UNSUPPORTED
        for i, blk in enumerate(self.st_gcns):
            s = p.st_gcns[i]
            bn1, pr1, conv, bn2 = blk.tcn[0], blk.tcn[1], blk.tcn[2], blk.tcn[3]
            s.gcn_w, s.gcn_b = _p(blk.gcn.conv.weight), _p(blk.gcn.conv.bias)
            s.bn1_w, s.bn1_b, s.bn1_mean, s.bn1_var = (_p(bn1.weight), _p(bn1.bias), _p(bn1.running_mean),
                                                       _p(bn1.running_var))
            s.prelu1 = _p(pr1.weight)
            s.tcn_w, s.tcn_b = _p(conv.weight), _p(conv.bias)
            s.bn2_w, s.bn2_b, s.bn2_mean, s.bn2_var = (_p(bn2.weight), _p(bn2.bias), _p(bn2.running_mean),
                                                       _p(bn2.running_var))
            if blk.residual is not None:
                rc, rb = blk.residual[0], blk.residual[1]
                s.res_w, s.res_b = _p(rc.weight), _p(rc.bias)
                s.res_bn_w, s.res_bn_b, s.res_bn_mean, s.res_bn_var = (_p(rb.weight), _p(rb.bias), _p(rb.running_mean),
                                                                       _p(rb.running_var))
            s.prelu = _p(blk.prelu.weight)
        for j, (conv, pr) in enumerate(zip(self.tpcnns, self.prelus)):
            p.tpcnn_w[j], p.tpcnn_b[j], p.prelus[j] = _p(conv.weight), _p(conv.bias), _p(pr.weight)
        p.out_w, p.out_b = _p(self.tpcnn_ouput.weight), _p(self.tpcnn_ouput.bias)
        return p, dev

    def outside_native_training(self):
        """-> None, or the field that puts this instance outside the family that trains natively, as text"""
        if self.graph_per_time_row:
            return "graph_per_time_row = True (native: False; the per-time-row base of GPGraphSTGCNN has no native backward)"
        if self.n_stgcnn != 1:
            return (f"n_stgcnn = {self.n_stgcnn} (native: 1; deeper stacks send a gradient through the Laplacian "
                    "contraction and are out of scope)")
        for field, want in (("input_feat", 1), ("kernel_size", 3), ("seq_len", self.pred_seq_len + 2)):
            if getattr(self, field) != want:
                return f"{field} = {getattr(self, field)} (native: {want})"
        for field, hi in (("n_txpcnn", L.STGCNN_MAX_LAYERS), ("output_feat", 64), ("pred_seq_len", L.MAX_K)):
            if not 1 <= getattr(self, field) <= hi:
                return f"{field} = {getattr(self, field)} (native: 1 to {hi})"
        blk = self.st_gcns[0]
        bns = {"tcn.0": blk.tcn[0], "tcn.3": blk.tcn[3]}
        if blk.residual is not None:
            bns["residual.1"] = blk.residual[1]
        for name, m in bns.items():
            if not isinstance(m, nn.BatchNorm2d):
                return f"st_gcns.0.{name} is {type(m).__name__} (native: BatchNorm2d)"
            if not m.affine or m.weight is None:
                return f"st_gcns.0.{name}.affine = False (native: True)"
            if not m.track_running_stats or m.running_mean is None:
                return f"st_gcns.0.{name}.track_running_stats = False (native: True)"
            if not isinstance(m.momentum, float):
                return f"st_gcns.0.{name}.momentum = {m.momentum} (native: a float)"
        for field in ("momentum", "eps"):
            if len({float(getattr(m, field)) for m in bns.values()}) != 1:
                return f"BatchNorm {field} differs between {', '.join(bns)} (native: one {field})"
        if getattr(blk.tcn[4], "p", 0) != 0:
            return f"st_gcns.0.tcn.4.p = {blk.tcn[4].p} (native: 0)"
        return None

    def unused_parameter_names(self):
        """the parameters the forward never reads (model.py:140: the last tpcnn / PReLU pair when n_txpcnn >= 2)"""
        j = self.n_txpcnn - 1
        return {f"tpcnns.{j}.weight", f"tpcnns.{j}.bias", f"prelus.{j}.weight"} if j >= 1 else set()

    def et_train_state(self):
        """-> et_stgcnn_train: the momentum, the writable running statistics and num_batches_tracked of st_gcns.0"""
        t = L.STGCNNTrain()
        blk = self.st_gcns[0]
        t.momentum = float(blk.tcn[0].momentum)
        for name, m in (("bn1", blk.tcn[0]), ("bn2", blk.tcn[3]), ("res_bn", None if blk.residual is None else blk.residual[1])):
            if m is not None:
                setattr(t, name + "_mean", _p(m.running_mean))
                setattr(t, name + "_var", _p(m.running_var))
                setattr(t, name + "_batches", m.num_batches_tracked.data_ptr())
        return t

    native_parameters = nn.Module.parameters  # what :mod:`._native_train` differentiates: every parameter

    def native_forward(self, et, v, a):
        from . import ops
        ws = ops.stgcnn_train_workspace(self, v.shape[-1], et_params=et)
        return ops.stgcnn_train_forward_graph(self, v, a, ws, et_params=et), (() if ws is None else (ws,))

    def native_backward(self, et, kept, g_out):
        from . import ops
        views = ops.stgcnn_grad_views(self, ops.stgcnn_backward_graph(self, kept[0] if kept else None, g_out, et_params=et))
        unused = self.unused_parameter_names()
        return [None if name in unused else g for name, g in views.items()]

    def forward(self, v, a):
        if self.training and self.native_training and self.outside_native_training() is None:
            if v.requires_grad or a.requires_grad:
                raise RuntimeError("SocialSTGCNN: no input gradient is built (the stgcnn bridge detaches v); an input "
                                   "requires one")
            dev = L.module_device("SocialSTGCNN", self, buffers=True)
            v, a = (L.on_device(t, dev) for t in (v, a))
            return train_forward(self, v, a)
        if self.training:
            raise RuntimeError("SocialSTGCNN: only inference is native (BatchNorm running statistics, no dropout); "
                               "training-mode forward and backward are not implemented -- call .eval() first")
        if self.graph_per_time_row:
            raise NotImplementedError("SocialSTGCNN: the per-time-row variant (graph_per_time_row=True) runs only as the three "
                                      "passes of GPGraphSTGCNN's call (eigentrajectory_amd.gpgraph); there is no stand-alone "
                                      "kernel for it")
        from . import ops
        return ops.stgcnn_forward_graph(self, v, a)
