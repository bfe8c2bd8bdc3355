"""SGCN, the predictor of ET-SGCN (baseline/sgcn/model.py: TrajectoryModel), inference on HIP kernels.

Same constructor signature and the same sub-module / parameter names as the reference
(``sparse_weighted_adjacency_matrices.{spatial,temporal}_attention.{embedding,query,key}``, ``….spa_fusion.conv.{0,1}``,
``….interaction_mask.{spatial,temporal}_asymmetric_convolutions.{j}.{conv1,conv2,activation}``,
``stsgcn.{spatial_temporal,temporal_spatial}_sparse_gcn.{0,1}.{embedding,activation}``, ``fusion_``, ``tcns.{j}.{0,1}``,
``output``), so a reference ET-SGCN checkpoint's ``baseline_model.*`` keys load unchanged, and the module plugs into
:class:`eigentrajectory_amd.EigenTrajectory` through the existing ``sgcn`` bridge::

    model = EigenTrajectory(SGCN(number_asymmetric_conv_layer=7, embedding_dims=64, number_gcn_layers=1, dropout=0,
                                 obs_len=hp.k + 2, pred_len=hp.k, n_tcn=5, in_dims=1, out_dims=hp.num_samples),
                            get_hook_func("sgcn"), hp).eval()

``forward(graph, identity)`` in eval mode is ``et_sgcn_forward_graph`` (csrc/et_sgcn.hip): graph (1, T, N, 1), identity a
list of the spatial (1 or T, N, N) and the temporal (N, 1, 1) or (N, T, T) one -> (pred_len, N, out_dims).  The identities
are read as given: the bridge's temporal one is all ones, not ``eye(T)``.  The weights are read in place from this module's
tensors (a ``load_state_dict``, a ``.to()`` or an in-place edit is seen by the next call, and by a captured graph's next
replay).  A forward in training mode, or with ``dropout != 0`` (the reference's always-active ``F.dropout``), raises -- unless
the instance was switched by ``eigentrajectory_amd.enable_native_training(model)``: with ``dropout = 0`` the training-mode
forward *is* the eval forward, and a training-mode ``forward(graph, identity)`` then runs the same kernels on a layout that
keeps every layer's input (``et_sgcn_train_forward_graph``) and is differentiable with respect to every parameter
(``et_sgcn_backward_graph``, csrc/et_sgcn_train.inl; no input gradient: the sgcn bridge detaches the graph; ``key.bias`` of
both attentions gets an exact zero).  The switch is the plain attribute ``native_training`` (no parameter, no buffer, not in
the ``state_dict``, default False).  A whole split runs in a fixed number of launches through
:meth:`EigenTrajectory.evaluate_split` / :func:`eigentrajectory_amd.ops.sgcn_forward_scenes`.
Supported family: ``in_dims = 1``, ``num_heads = 4``, ``embedding_dims = 64``, ``1 <= number_asymmetric_conv_layer, n_tcn <=
8``, ``pred_len <= 32``, ``obs_len = pred_len + 2``, ``1 <= out_dims <= 64``, ``N <= 512``; other shapes construct, but their
forward raises.

``SGCN(..., position_channel=True)`` is baseline/gpgraphsgcn/model_baseline.py's variant, the base of
:class:`eigentrajectory_amd.gpgraph.GPGraphSGCN`: the graph carries a position channel in front of the coefficient channel,
the temporal attention reads both (its embedding is ``Linear(in_dims + 1, 64)``), and ``forward(graph, identity, mask=None)``
takes a (1, T, N, 2) graph.  Natively it runs only inside GP-Graph's call, where its three passes are the virtual scenes of
one run of the kernels; called on its own its forward raises.
"""
from __future__ import annotations

import math

import torch.nn as nn

from . import _lib as L
from ._lib import _p
from ._native_train import train_forward


class _AsymmetricConvolution(nn.Module):
    """PReLU(conv(1x3) + conv(3x1)) + shortcut; conv1 (3x1) carries no bias."""

    def __init__(self, in_cha, out_cha):
        super().__init__()
        self.conv1 = nn.Conv2d(in_cha, out_cha, kernel_size=(3, 1), padding=(1, 0), bias=False)
        self.conv2 = nn.Conv2d(in_cha, out_cha, kernel_size=(1, 3), padding=(0, 1))
        self.activation = nn.PReLU()


class _InteractionMask(nn.Module):
    def __init__(self, number_asymmetric_conv_layer=7, spatial_channels=4, temporal_channels=4):
        super().__init__()
        self.number_asymmetric_conv_layer = number_asymmetric_conv_layer
        self.spatial_asymmetric_convolutions = nn.ModuleList()
        self.temporal_asymmetric_convolutions = nn.ModuleList()
        for _ in range(number_asymmetric_conv_layer):
            self.spatial_asymmetric_convolutions.append(_AsymmetricConvolution(spatial_channels, spatial_channels))
            self.temporal_asymmetric_convolutions.append(_AsymmetricConvolution(temporal_channels, temporal_channels))


class _SelfAttention(nn.Module):
    def __init__(self, in_dims=2, d_model=64, num_heads=4):
        super().__init__()
        self.embedding = nn.Linear(in_dims, d_model)
        self.query = nn.Linear(d_model, d_model)
        self.key = nn.Linear(d_model, d_model)
        self.scaled_factor = math.sqrt(d_model)  # a plain attribute, as in the reference: not in the state dict
        self.num_heads = num_heads


class _SpatialTemporalFusion(nn.Module):
    def __init__(self, obs_len=8):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(obs_len, obs_len, 1), nn.PReLU())


class _SparseWeightedAdjacency(nn.Module):
    def __init__(self, spa_in_dims=2, tem_in_dims=3, embedding_dims=64, obs_len=8, dropout=0,
                 number_asymmetric_conv_layer=7):
        super().__init__()
        self.spatial_attention = _SelfAttention(spa_in_dims, embedding_dims)
        self.temporal_attention = _SelfAttention(tem_in_dims, embedding_dims)
        self.spa_fusion = _SpatialTemporalFusion(obs_len=obs_len)
        self.interaction_mask = _InteractionMask(number_asymmetric_conv_layer=number_asymmetric_conv_layer)
        self.dropout = dropout


class _GraphConvolution(nn.Module):
    def __init__(self, in_dims=2, embedding_dims=16, dropout=0):
        super().__init__()
        self.embedding = nn.Linear(in_dims, embedding_dims, bias=False)
        self.activation = nn.PReLU()
        self.dropout = dropout


class _SparseGraphConvolution(nn.Module):
    def __init__(self, in_dims=16, embedding_dims=16, dropout=0):
        super().__init__()
        self.dropout = dropout
        self.spatial_temporal_sparse_gcn = nn.ModuleList()
        self.temporal_spatial_sparse_gcn = nn.ModuleList()
        self.spatial_temporal_sparse_gcn.append(_GraphConvolution(in_dims, embedding_dims))
        self.spatial_temporal_sparse_gcn.append(_GraphConvolution(embedding_dims, embedding_dims))
        self.temporal_spatial_sparse_gcn.append(_GraphConvolution(in_dims, embedding_dims))
        self.temporal_spatial_sparse_gcn.append(_GraphConvolution(embedding_dims, embedding_dims))


class SGCN(nn.Module):
    r"""baseline/sgcn/model.py's ``TrajectoryModel`` (eval-mode inference on the GPU).  ``forward(graph, identity)``: graph
    (1, T, N, 1) and the two identities as the sgcn bridge's pre-hook builds them -> (pred_len, N, out_dims)."""

    native_training = False  # a plain attribute, set per instance by eigentrajectory_amd.enable_native_training
    #: how enable_native_training ends its refusal of an instance outside the native family
    trains_natively = ("LBEBM, PECNet, SocialImplicitLight and an SGCN with in_dims = 1, num_heads = 4, embedding_dims = 64, dropout = 0 "
                       "and no position channel train natively")

    def __init__(self, number_asymmetric_conv_layer=7, embedding_dims=64, number_gcn_layers=1, dropout=0, obs_len=8,
                 pred_len=12, n_tcn=5, in_dims=2, out_dims=5, num_heads=4, position_channel=False):
        super().__init__()
        self.position_channel = bool(position_channel)
        self.number_asymmetric_conv_layer = number_asymmetric_conv_layer
        self.embedding_dims, self.number_gcn_layers, self.n_tcn, self.dropout = embedding_dims, number_gcn_layers, n_tcn, dropout
        self.obs_len, self.pred_len, self.in_dims, self.out_dims, self.num_heads = obs_len, pred_len, in_dims, out_dims, num_heads
        # (the reference leaves the adjacency's embedding_dims and the attention's num_heads at their defaults, 64 and 4)
        self.sparse_weighted_adjacency_matrices = _SparseWeightedAdjacency(
            number_asymmetric_conv_layer=number_asymmetric_conv_layer, obs_len=obs_len, spa_in_dims=in_dims,
            tem_in_dims=in_dims + 1 if position_channel else in_dims)
        self.stsgcn = _SparseGraphConvolution(in_dims=in_dims, embedding_dims=embedding_dims // num_heads, dropout=dropout)
        self.fusion_ = nn.Conv2d(num_heads, num_heads, kernel_size=1, bias=False)
        self.tcns = nn.ModuleList()
        self.tcns.append(nn.Sequential(nn.Conv2d(obs_len, pred_len, 3, padding=1), nn.PReLU()))
        for _ in range(1, n_tcn):
            self.tcns.append(nn.Sequential(nn.Conv2d(pred_len, pred_len, 3, padding=1), nn.PReLU()))
        self.output = nn.Linear(embedding_dims // num_heads, out_dims)

    def et_params(self):
        """-> (et_sgcn_params, device): this module's tensors as the kernels read them (include/eigentraj.h)."""
        p = L.SGCNParams()
        p.n_asym, p.embedding_dims, p.n_gcn_layers = self.number_asymmetric_conv_layer, self.embedding_dims, self.number_gcn_layers
        p.obs_len, p.pred_len, p.n_tcn, p.in_dims = self.obs_len, self.pred_len, self.n_tcn, self.in_dims
        p.out_dims, p.num_heads, p.dropout = self.out_dims, self.num_heads, float(self.dropout)
        dev = L.module_device("SGCN", self)
        if (self.number_asymmetric_conv_layer > L.SGCN_MAX_LAYERS or self.n_tcn > L.SGCN_MAX_LAYERS or self.in_dims != 1
                or self.num_heads != 4 or self.embedding_dims != 64):
            return p, dev  # the kernels answer ET_ERR_UNSUPPORTED
        swa = self.sparse_weighted_adjacency_matrices
        for a, att in enumerate((swa.spatial_attention, swa.temporal_attention)):
            s = p.att[a]
            s.emb_w, s.emb_b = _p(att.embedding.weight), _p(att.embedding.bias)
            s.q_w, s.q_b, s.k_w, s.k_b = _p(att.query.weight), _p(att.query.bias), _p(att.key.weight), _p(att.key.bias)
        conv, act = swa.spa_fusion.conv[0], swa.spa_fusion.conv[1]
        p.fus_w, p.fus_b, p.fus_a = _p(conv.weight), _p(conv.bias), _p(act.weight)
        im = swa.interaction_mask
        for dst, layers in ((p.asym_s, im.spatial_asymmetric_convolutions), (p.asym_t, im.temporal_asymmetric_convolutions)):
            for j, m in enumerate(layers):
                dst[j].conv1_w, dst[j].conv2_w = _p(m.conv1.weight), _p(m.conv2.weight)
                dst[j].conv2_b, dst[j].act = _p(m.conv2.bias), _p(m.activation.weight)
        gcns = list(self.stsgcn.spatial_temporal_sparse_gcn) + list(self.stsgcn.temporal_spatial_sparse_gcn)
        for g, m in enumerate(gcns):
            p.gcn[g].w, p.gcn[g].act = _p(m.embedding.weight), _p(m.activation.weight)
        p.fusion_w = _p(self.fusion_.weight)
        for j, seq in enumerate(self.tcns):
            p.tcn_w[j], p.tcn_b[j], p.tcn_a[j] = _p(seq[0].weight), _p(seq[0].bias), _p(seq[1].weight)
        p.out_w, p.out_b = _p(self.output.weight), _p(self.output.bias)
        return p, dev

    def outside_native_training(self):
        """-> None, or the field that puts this instance outside the family that trains natively, as text"""
        for field, want in (("in_dims", 1), ("num_heads", 4), ("embedding_dims", 64), ("dropout", 0),
                            ("position_channel", False)):
            if getattr(self, field) != want:
                return f"{field} = {getattr(self, field)} (native: {want})"
        return None

    def _check_mode(self):
        if self.training:
            raise RuntimeError("SGCN: only inference is native (no dropout, no backward); training-mode forward is not "
                               "implemented -- call .eval() first")
        if self.dropout != 0:
            raise RuntimeError(f"SGCN: dropout = {self.dropout} is not implemented natively (the reference's F.dropout is "
                               "active even in eval mode); construct with dropout=0")

    native_parameters = nn.Module.parameters  # what :mod:`._native_train` differentiates: every parameter

    def native_forward(self, et, graph, id_s, id_t):
        from . import ops
        ws = ops.sgcn_train_workspace(self, graph.shape[2], et_params=et)
        return ops.sgcn_train_forward_graph(self, graph, (id_s, id_t), ws, et_params=et), (id_s, id_t, ws)

    def native_backward(self, et, kept, g_out):
        from . import ops
        id_s, id_t, ws = kept
        return ops.sgcn_grad_views(self, ops.sgcn_backward_graph(self, (id_s, id_t), ws, g_out, et_params=et)).values()

    def forward(self, graph, identity, mask=None):
        if self.training and self.native_training and not self.position_channel and mask is None and self.dropout == 0:
            if graph.requires_grad or any(i.requires_grad for i in identity):
                raise RuntimeError("SGCN: no input gradient is built (the sgcn bridge detaches the graph); an input "
                                   "requires one")
            dev = L.module_device("SGCN", self)
            graph, id_s, id_t = (L.on_device(t, dev) for t in (graph, *identity))
            return train_forward(self, graph, id_s, id_t)
        self._check_mode()
        if self.position_channel or mask is not None:
            raise NotImplementedError("SGCN: the two-channel base (position_channel=True) and the mask argument run only as "
                                      "the three passes of GPGraphSGCN's call (eigentrajectory_amd.gpgraph); there is no "
                                      "stand-alone kernel entry for them")
        from . import ops
        return ops.sgcn_forward_graph(self, graph, identity)
