"""GP-Graph-SGCN, the predictor of ET-GPGraph-SGCN (baseline/gpgraphsgcn/model.py: get_GPGraph_SGCN_model, the reference's
default configuration), and GP-Graph-STGCNN, the predictor of ET-GPGraph-STGCNN (baseline/gpgraphstgcnn/model.py:
get_GPGraph_STGCNN_model), inference on HIP kernels.

Same sub-module / parameter names as the reference's ``GPGraph`` -- ``baseline_model.*`` (the two-channel SGCN,
:class:`eigentrajectory_amd.sgcn.SGCN` with ``position_channel=True``), ``group_gen.group_cnn.0``, ``group_gen.th``,
``group_mix.st_gcns_mix.{0,1}`` -- so a reference ET-GPGraph-SGCN checkpoint's ``baseline_model.baseline_model.*``,
``baseline_model.group_gen.*`` and ``baseline_model.group_mix.*`` keys load unchanged, and the module plugs into
:class:`eigentrajectory_amd.EigenTrajectory` through the existing ``gpgraphsgcn`` bridge::

    model = EigenTrajectory(get_GPGraph_SGCN_model(obs_len=hp.k + 2, pred_len=hp.k, in_dims=1, out_dims=hp.num_samples),
                            get_hook_func("gpgraphsgcn"), hp).eval()

``forward(v_abs, v_rel)`` in eval mode is ``et_gpgraph_sgcn_forward_graph`` (csrc/et_gpgraph.hip): v_abs (1, 1, T, N) and
v_rel (1, 2, T, N) as the bridge builds them -> ``(v, indices)`` with v (1, out_dims, pred_len, N) and indices int64 (N,),
the group of every pedestrian, as the reference returns them.  The weights, ``group_gen.th`` included, are read in place on
the device at every call (an in-place edit is seen by the next call and by a captured graph's next replay).  A whole split
runs in a fixed number of launches through :meth:`EigenTrajectory.evaluate_split` /
:func:`eigentrajectory_amd.ops.gpgraph_sgcn_forward_scenes`.

GP-Graph-STGCNN is the same wrapper around the original Social-STGCNN
(:class:`eigentrajectory_amd.stgcnn.SocialSTGCNN` with ``graph_per_time_row=True``), under the ``gpgraphstgcnn`` bridge::

    model = EigenTrajectory(get_GPGraph_STGCNN_model(obs_len=hp.k + 2, pred_len=hp.k, in_dims=1, out_dims=hp.num_samples),
                            get_hook_func("gpgraphstgcnn"), hp).eval()

``forward(v_abs, v_rel)`` is then ``et_gpgraph_stgcnn_forward_graph`` (csrc/et_gpgraph_stgcnn.hip, three launches), both
inputs (1, 1, T, N); a whole split runs through :func:`eigentrajectory_amd.ops.gpgraph_stgcnn_forward_scenes`.

Native: the ET configuration -- ``d_type='learned_l2norm'``, ``d_th='learned'``, ``mix_type='mlp'``, ``group_type=(True,
True, True)``, ``weight_share=True`` -- in eval mode with ``dropout = 0``, around either base.  The other ``d_type`` /
``d_th`` / ``mix_type`` / ``group_type`` / ``weight_share=False`` variants are not: they construct (with the reference's
parameters), and their forward raises.  A training-mode forward raises too -- unless the instance, around an SGCN base, was
switched by ``eigentrajectory_amd.enable_native_training(model)``: with ``dropout = 0`` the training-mode forward *is* the
eval forward, and ``forward(v_abs, v_rel)`` then runs the same kernels on a layout that keeps what the backward pass reads
(``et_gpgraph_sgcn_train_forward_graph``) and returns ``(v, indices)`` with ``v`` differentiable with respect to every
parameter of the wrapper and of its base (``et_gpgraph_sgcn_backward_graph``, csrc/et_gpgraph_train.inl; ``indices`` is
not differentiable, the grouping reaches ``v`` through the straight-through soft assignment; no input gradient: the bridge
detaches the graph; ``key.bias`` of both attentions gets an exact zero).  The switch is the plain attribute
``native_training`` (no parameter, no buffer, not in the ``state_dict``, default False).  GP-Graph around Social-STGCNN
has no native training: its per-time-row base (BatchNorm batch statistics in training mode) has no native backward, unlike the
stand-alone ``SocialSTGCNN`` of ET-STGCNN.
"""
from __future__ import annotations

import copy

import torch
import torch.nn as nn

from . import _lib as L
from ._lib import _p
from ._native_train import train_forward
from .sgcn import SGCN
from .stgcnn import SocialSTGCNN


class _GroupGenerator(nn.Module):
    def __init__(self, d_type="learned_l2norm", th=1.0, in_channels=16, hid_channels=32, n_head=1, dropout=0):
        super().__init__()
        self.d_type = d_type
        if d_type == "learned":
            self.group_cnn = nn.Sequential(nn.Conv2d(in_channels, hid_channels, 1), nn.ReLU(), nn.BatchNorm2d(hid_channels),
                                           nn.Dropout(dropout, inplace=True), nn.Conv2d(hid_channels, n_head, 1))
        elif d_type == "estimate_th":
            self.group_cnn = nn.Sequential(nn.Conv2d(in_channels, n_head, 1))
        elif d_type == "learned_l2norm":
            self.group_cnn = nn.Sequential(nn.Conv2d(in_channels, hid_channels, kernel_size=(3, 1), padding=(1, 0)))
        # (as in the reference: a float is a fixed threshold, anything else -- 'learned' -- a parameter that starts at 1)
        self.th = th if type(th) == float else nn.Parameter(torch.Tensor([1]))


class _GroupIntegrator(nn.Module):
    def __init__(self, mix_type="mean", n_mix=3, out_channels=5, pred_seq_len=12):
        super().__init__()
        self.mix_type, self.pred_seq_len = mix_type, pred_seq_len
        if mix_type == "mlp":
            self.st_gcns_mix = nn.Sequential(nn.PReLU(), nn.Conv2d(out_channels * pred_seq_len * n_mix,
                                                                    out_channels * pred_seq_len, kernel_size=1))
        elif mix_type == "cnn":
            self.st_gcns_mix = nn.Sequential(nn.PReLU(), nn.Conv2d(out_channels * n_mix, out_channels, kernel_size=(3, 1),
                                                                    padding=(1, 0)))


class GPGraph(nn.Module):
    r"""model_groupwrapper.py's ``GPGraph`` (baseline/gpgraphsgcn and baseline/gpgraphstgcnn: the same class) around an
    :class:`SGCN` (``position_channel=True``) or a :class:`SocialSTGCNN` (``graph_per_time_row=True``) base (eval-mode
    inference on the GPU).  ``forward(v_abs, v_rel)`` -> ``(v (1, S, k, N), indices (N,) int64)``."""

    TAU = 0.1  # GroupGenerator.forward's default temperature; GPGraph.forward does not pass another
    native_training = False  # a plain attribute, set per instance by eigentrajectory_amd.enable_native_training
    #: how enable_native_training ends its refusal of an instance outside the native family
    trains_natively = ("LBEBM, PECNet, SocialImplicitLight, SGCN and a GPGraph in the ET configuration around "
                       "SGCN(position_channel=True, dropout=0) train natively")

    def __init__(self, baseline_model, in_channels=2, out_channels=5, obs_seq_len=8, pred_seq_len=12,
                 d_type="learned_l2norm", d_th="learned", mix_type="mlp", group_type=None, weight_share=True):
        super().__init__()
        group_type = (True,) * 3 if group_type is None else tuple(bool(g) for g in group_type)
        self.obs_seq_len, self.pred_seq_len, self.in_channels, self.out_channels = obs_seq_len, pred_seq_len, in_channels, out_channels
        self.d_type, self.d_th, self.mix_type, self.weight_share = d_type, d_th, mix_type, weight_share
        self.include_original, self.include_inter_group, self.include_intra_group = group_type
        # (weight_share=False: one copy of the base per graph, as the callers of the reference build it)
        self.baseline_model = baseline_model if weight_share else nn.ModuleList(
            [baseline_model] + [copy.deepcopy(baseline_model) for _ in range(2)])
        self.group_gen = _GroupGenerator(d_type=d_type, th=d_th, in_channels=in_channels, hid_channels=8)
        self.group_mix = _GroupIntegrator(mix_type=mix_type, n_mix=sum(group_type), out_channels=out_channels,
                                          pred_seq_len=pred_seq_len)

    @property
    def stgcnn_base(self):
        """True around a Social-STGCNN base (GP-Graph-STGCNN), False around an SGCN base (GP-Graph-SGCN)."""
        return isinstance(self.baseline_model, SocialSTGCNN)

    def outside_native_training(self):
        """-> None, or what puts this instance outside the family that trains natively, as text"""
        if self.stgcnn_base:
            return ("the per-time-row SocialSTGCNN base (graph_per_time_row=True, BatchNorm batch statistics in training "
                    "mode) has no native backward; only the stand-alone SocialSTGCNN of ET-STGCNN trains natively")
        for field, want in (("d_type", "learned_l2norm"), ("mix_type", "mlp"), ("weight_share", True)):
            if getattr(self, field) != want:
                return f"{field} = {getattr(self, field)!r} (native: {want!r})"
        if not isinstance(self.group_gen.th, nn.Parameter):
            return f"d_th = {self.d_th!r} (native: 'learned')"
        if not (self.include_original and self.include_inter_group and self.include_intra_group):
            return (f"group_type = {(self.include_original, self.include_inter_group, self.include_intra_group)} "
                    "(native: (True, True, True))")
        base = self.baseline_model
        if not isinstance(base, SGCN):
            return f"baseline_model = {type(base).__name__} (native: SGCN)"
        for field, want in (("in_dims", 1), ("num_heads", 4), ("embedding_dims", 64), ("dropout", 0),
                            ("position_channel", True)):
            if getattr(base, field) != want:
                return f"baseline_model.{field} = {getattr(base, field)} (native: {want})"
        return None

    def _check_mode(self):
        base = self.baseline_model
        base_ok = ((isinstance(base, SGCN) and base.position_channel)
                   or (isinstance(base, SocialSTGCNN) and base.graph_per_time_row))
        if (self.d_type != "learned_l2norm" or not isinstance(self.group_gen.th, nn.Parameter) or self.mix_type != "mlp"
                or not (self.include_original and self.include_inter_group and self.include_intra_group)
                or not self.weight_share or not base_ok):
            raise NotImplementedError("GPGraph: only the ET configuration is native -- d_type='learned_l2norm', d_th='learned', "
                                      "mix_type='mlp', group_type=(True, True, True), weight_share=True around "
                                      "SGCN(position_channel=True) or SocialSTGCNN(graph_per_time_row=True); the other "
                                      "variants are not implemented")
        if self.training:
            raise RuntimeError("GPGraph: only inference is native (no backward, no straight-through gradient); "
                               "training-mode forward is not implemented -- call .eval() first")
        if isinstance(base, SGCN):
            base._check_mode()
        elif base.training:
            raise RuntimeError("GPGraph: the SocialSTGCNN base is in training mode (BatchNorm batch statistics are not "
                               "native) -- call .eval() on the whole model")

    def et_params(self):
        """-> (et_gpgraph_sgcn_params or et_gpgraph_stgcnn_params, device): this module's tensors as the kernels read them
        (include/eigentraj.h)."""
        base, dev = self.baseline_model.et_params()
        p = L.GPGraphSTGCNNParams() if self.stgcnn_base else L.GPGraphSGCNParams()
        p.base = base
        L.module_device("GPGraph", self.group_gen, self.group_mix, device=dev)  # (the base has checked its own)
        if self.stgcnn_base:
            b = self.baseline_model
            if self.in_channels != 1 or self.out_channels != b.output_feat or self.pred_seq_len != b.pred_seq_len \
                    or self.obs_seq_len != b.seq_len:
                p.base.input_feat = -1  # the kernels answer ET_ERR_UNSUPPORTED
                return p, dev
        elif self.in_channels != 1 or self.out_channels != self.baseline_model.out_dims \
                or self.pred_seq_len != self.baseline_model.pred_len or self.obs_seq_len != self.baseline_model.obs_len:
            p.base.in_dims = -1  # the kernels answer ET_ERR_UNSUPPORTED
            return p, dev
        conv = self.group_gen.group_cnn[0]
        p.group_w, p.group_b, p.th, p.tau = _p(conv.weight), _p(conv.bias), _p(self.group_gen.th), self.TAU
        act, mix = self.group_mix.st_gcns_mix[0], self.group_mix.st_gcns_mix[1]
        p.mix_a, p.mix_w, p.mix_b = _p(act.weight), _p(mix.weight), _p(mix.bias)
        return p, dev

    native_parameters = nn.Module.parameters  # what :mod:`._native_train` differentiates: every parameter, the base's too

    def native_forward(self, et, v_abs, v_rel):
        from . import ops
        ws = ops.gpgraph_sgcn_train_workspace(self, v_abs.shape[3], et_params=et)
        return ops.gpgraph_sgcn_train_forward_graph(self, v_abs, v_rel, ws, et_params=et), (ws,)  # (v, the indices)

    def native_backward(self, et, kept, g_out):
        from . import ops
        return ops.gpgraph_sgcn_grad_views(self, ops.gpgraph_sgcn_backward_graph(self, kept[0], g_out, et_params=et)).values()

    def forward(self, v_abs, v_rel):
        if self.training and self.native_training and self.outside_native_training() is None:
            if v_abs.requires_grad or v_rel.requires_grad:
                raise RuntimeError("GPGraph: no input gradient is built (the gpgraphsgcn bridge detaches the graph); an "
                                   "input requires one")
            dev = L.module_device("GPGraph", self)
            v_abs, v_rel = (L.on_device(t, dev) for t in (v_abs, v_rel))
            return train_forward(self, v_abs, v_rel)
        self._check_mode()
        from . import ops
        if self.stgcnn_base:
            return ops.gpgraph_stgcnn_forward_graph(self, v_abs, v_rel)
        return ops.gpgraph_sgcn_forward_graph(self, v_abs, v_rel)


class GPGraphSGCN(GPGraph):
    r"""``get_GPGraph_SGCN_model``'s network as a class: the ET base (7 asymmetric layers, 5 tcns, dropout 0) inside
    :class:`GPGraph` with the reference's fixed arguments."""

    def __init__(self, obs_len=8, pred_len=12, in_dims=2, out_dims=5):
        base = SGCN(number_asymmetric_conv_layer=7, embedding_dims=64, number_gcn_layers=1, dropout=0, obs_len=obs_len,
                    pred_len=pred_len, n_tcn=5, in_dims=in_dims, out_dims=out_dims, position_channel=True)
        super().__init__(baseline_model=base, in_channels=in_dims, out_channels=out_dims, obs_seq_len=obs_len,
                         pred_seq_len=pred_len, d_type="learned_l2norm", d_th="learned", mix_type="mlp",
                         group_type=(True, True, True), weight_share=True)


def get_GPGraph_SGCN_model(obs_len=8, pred_len=12, in_dims=2, out_dims=5):
    """The reference's factory (baseline/gpgraphsgcn/model.py), without its ``.cuda()``: move the result yourself."""
    return GPGraphSGCN(obs_len=obs_len, pred_len=pred_len, in_dims=in_dims, out_dims=out_dims)


class GPGraphSTGCNN(GPGraph):
    r"""``get_GPGraph_STGCNN_model``'s network as a class: the original Social-STGCNN (one st_gcn, five tpcnns, kernel 3)
    inside :class:`GPGraph` with the reference's fixed arguments."""

    def __init__(self, obs_len=8, pred_len=12, in_dims=2, out_dims=5):
        base = SocialSTGCNN(n_stgcnn=1, n_txpcnn=5, input_feat=in_dims, output_feat=out_dims, kernel_size=3, seq_len=obs_len,
                            pred_seq_len=pred_len, graph_per_time_row=True)
        super().__init__(baseline_model=base, in_channels=in_dims, out_channels=out_dims, obs_seq_len=obs_len,
                         pred_seq_len=pred_len, d_type="learned_l2norm", d_th="learned", mix_type="mlp",
                         group_type=(True, True, True), weight_share=True)


def get_GPGraph_STGCNN_model(obs_len=8, pred_len=12, in_dims=2, out_dims=5):
    """The reference's factory (baseline/gpgraphstgcnn/model.py), without its ``.cuda()``: move the result yourself."""
    return GPGraphSTGCNN(obs_len=obs_len, pred_len=pred_len, in_dims=in_dims, out_dims=out_dims)
