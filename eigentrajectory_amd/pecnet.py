"""PECNet, the predictor of ET-PECNet (baseline/pecnet/model.py), inference and training of ``predict`` on HIP kernels.

Same constructor signature and the same sub-module / parameter names as the reference (``encoder_past.layers.{i}``,
``encoder_dest``, ``encoder_latent``, ``decoder``, ``non_local_theta``, ``non_local_phi``, ``non_local_g``, ``predictor``),
so a reference ET-PECNet checkpoint's ``baseline_model.*`` keys load unchanged (``strict=True``), and the module plugs into
:class:`eigentrajectory_amd.EigenTrajectory` through the existing ``pecnet`` bridge, which calls ``predict`` only::

    model = EigenTrajectory(PECNet([512, 256], [8, 16], [8, 50], [1024, 512, 1024], [1024, 512, 256], [256, 128, 64],
                                   [256, 128, 64], [256, 128, 64], 16, 16, 3, 128, 1.3, hp.k // 2,
                                   hp.k * hp.num_samples // 2 + 1, False), get_hook_func("pecnet"), hp).eval()

``predict(past, generated_dest, mask, initial_pos)`` in eval mode is ``2 + 2 * nonlocal_pools`` launches of
csrc/et_mlp.hip (8 for the ET configuration): the two encoders side by side; per pooling round theta, phi and g side by
side, then the attention step; the predictor.  Every Linear runs on the f32-input MFMA in exact fp32.  The pooling follows
the reference's order: softmax over ALL columns of the row, then the mask, then ``F.normalize(p=1)``.  ``mask`` (N, N) may
be bool or float32 (it is converted to float32 here); the weights are read in place from this module's tensors.
``encoder_latent`` and ``decoder`` only hold their tensors: ``forward`` (the CVAE path, random sampling) and a ``predict``
in training mode raise.  A whole split runs in the same fixed number of launches through
:meth:`EigenTrajectory.evaluate_split` / :func:`eigentrajectory_amd.ops.pecnet_forward_scenes`.
Supported family: ``activation='relu'``, ``discrim=False``, ``dropout=-1``, 1 to 4 hidden layers per MLP, widths 1 to 1024,
``nonlocal_pools`` 0 to 8, up to 4096 rows per ``predict`` call with pooling; other shapes construct, but their use raises.

Training (opt-in): the reference's ``pecnet`` bridge calls ``predict`` in training too, so training ET-PECNet differentiates
exactly what ``predict`` computes (no CVAE, no sampling).  After ``eigentrajectory_amd.enable_native_training(model)`` a
``predict`` in training mode runs the same ``2 + 2 * nonlocal_pools`` launches with everything the backward needs kept, and
its backward pass is ``3 + 3 * nonlocal_pools`` launches of csrc/et_mlp_train.hip (12 for the ET configuration): the
predictor's rows; per pooling round, last to first, the attention step's rows, its column sums, then theta, phi and g side by
side; both encoders' rows; every dW / db, the shared theta / phi / g weights summed over the rounds.  The gradients reach
``.grad`` of the tensors of ``encoder_past``, ``encoder_dest``, ``non_local_theta``, ``non_local_phi``, ``non_local_g`` and
``predictor`` the ordinary autograd way; ``encoder_latent`` and ``decoder`` get none, the mask gets none::

    model = EigenTrajectory(PECNet(...), get_hook_func("pecnet"), hp)
    eigentrajectory_amd.enable_native_training(model)
    ETTrainer(model, hp, train_data, val_data).fit(epochs)

The switch is the plain attribute ``native_training`` (no parameter, no buffer, not in the ``state_dict``, default False);
without the call everything is as before: ``predict`` in training mode raises.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib as L


class MLP(nn.Module):
    """The reference's MLP as a holder of ``layers.{i}`` (``nn.Linear``); the native chain is Linear + ReLU, no activation
    after the last layer."""

    def __init__(self, input_dim, output_dim, hidden_size=(1024, 512), activation="relu", discrim=False, dropout=-1):
        super().__init__()
        dims = [input_dim, *hidden_size, output_dim]
        self.layers = nn.ModuleList([nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)])
        self.activation = {"relu": nn.ReLU, "sigmoid": nn.Sigmoid}[activation]()
        self.activation_name, self.discrim, self.dropout = activation, discrim, dropout

    def et_chain(self, chain, who):
        """Fill the ``et_mlp_chain`` mirror ``chain`` from this module's tensors."""
        if self.activation_name != "relu" or self.discrim or self.dropout != -1:
            raise L.ETLibraryError(f"{who}: only activation='relu', discrim=False, dropout=-1 are native "
                                   f"(got {self.activation_name!r}, {self.discrim}, {self.dropout})")
        chain.n_layers = len(self.layers)
        if len(self.layers) > L.MLP_MAX_LAYERS:
            return  # the library answers ET_ERR_UNSUPPORTED
        chain.widths[0] = self.layers[0].in_features
        for i, lin in enumerate(self.layers):
            chain.widths[i + 1] = lin.out_features
            chain.w[i], chain.b[i] = lin.weight.data_ptr(), lin.bias.data_ptr()


def require_eval(module, who):
    if module.training:
        raise RuntimeError(f"{who}: only predict() in eval mode is native (no CVAE, no sampling, no backward pass) -- call "
                           ".eval() first")


class _TrainPredict(torch.autograd.Function):
    """``predict`` with a backward pass (csrc/et_mlp_train.hip).  The tensors of the six chains are inputs, so their gradients
    accumulate into ``.grad`` like any other parameter's; they, the inputs, the mask and the kept values are saved through
    ``save_for_backward``: the kernels read the weights in place, and an in-place change between forward and backward (an
    optimiser step) is caught by autograd's version counters.  ``generated_dest`` and ``initial_pos`` may be one tensor
    (the bridge's): each gets its own gradient tensor and autograd sums the two."""

    @staticmethod
    def forward(ctx, model, mask, past, dest, pos, *params):
        from . import ops
        out, saved = ops.pecnet_train_fwd(model, past, dest, mask, pos)
        ctx.model = model
        ctx.has_mask = mask is not None
        ctx.save_for_backward(past, dest, pos, saved, *(() if mask is None else (mask,)), *params)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, g_out):
        need = ctx.needs_input_grad
        if g_out is None:
            return (None,) * len(need)
        from . import ops
        past, dest, pos, saved = ctx.saved_tensors[:4]
        mask = ctx.saved_tensors[4] if ctx.has_mask else None
        params = ctx.saved_tensors[4 + ctx.has_mask:]
        model = ctx.model
        if any(p.data_ptr() != q.data_ptr() for p, q in zip(params, model.chain_parameters())):
            raise RuntimeError("PECNet: a parameter tensor of the six chains was replaced between forward and backward")
        g = ops.pecnet_train_bwd(model, past, dest, mask, pos, saved, g_out, (need[2], need[3], need[4]))
        return (None, None, g.get("past"), g.get("dest"), g.get("pos"),
                *(g.get(name) if wanted else None for name, wanted in zip(model.chain_parameter_names(), need[5:])))


class PECNet(nn.Module):
    """baseline/pecnet/model.py's ``PECNet``: ``predict`` natively (eval mode; training mode after
    :func:`eigentrajectory_amd.enable_native_training`), everything else a tensor holder."""

    CHAINS = ("encoder_past", "encoder_dest", "non_local_theta", "non_local_phi", "non_local_g", "predictor")  # of ``predict``
    CHAINS_WITHOUT_POOLING = ("encoder_past", "encoder_dest", "predictor")  # nonlocal_pools = 0
    native_training = False  # a plain attribute, set per instance by eigentrajectory_amd.enable_native_training

    def __init__(self, enc_past_size, enc_dest_size, enc_latent_size, dec_size, predictor_size, non_local_theta_size,
                 non_local_phi_size, non_local_g_size, fdim, zdim, nonlocal_pools, non_local_dim, sigma, past_length,
                 future_length, verbose=False):
        super().__init__()
        self.fdim, self.zdim, self.nonlocal_pools, self.non_local_dim, self.sigma = fdim, zdim, nonlocal_pools, non_local_dim, sigma
        self.encoder_past = MLP(past_length * 2, fdim, enc_past_size)
        self.encoder_dest = MLP(2, fdim, enc_dest_size)
        self.encoder_latent = MLP(2 * fdim, 2 * zdim, enc_latent_size)
        self.decoder = MLP(fdim + zdim, 2, dec_size)
        self.non_local_theta = MLP(2 * fdim + 2, non_local_dim, non_local_theta_size)
        self.non_local_phi = MLP(2 * fdim + 2, non_local_dim, non_local_phi_size)
        self.non_local_g = MLP(2 * fdim + 2, 2 * fdim + 2, non_local_g_size)
        self.predictor = MLP(2 * fdim + 2, 2 * (future_length - 1), predictor_size)

    def et_params(self):
        """-> (et_mlp_params, device): this module's tensors as the kernels read them (include/eigentraj.h)."""
        p = L.MLPParams()
        p.fdim, p.nonlocal_pools, p.non_local_dim, p.pos_width = self.fdim, self.nonlocal_pools, self.non_local_dim, 2
        p.out_width = self.predictor.layers[-1].out_features
        for name in ("encoder_past", "encoder_dest", "non_local_theta", "non_local_phi", "non_local_g", "predictor"):
            getattr(self, name).et_chain(getattr(p, name), f"PECNet.{name}")
        return p, L.module_device("PECNet", self)

    def chain_parameter_names(self):
        return [f"{name}.layers.{i}.{kind}" for name in self.CHAINS for i in range(len(getattr(self, name).layers))
                for kind in ("weight", "bias")]

    def chain_parameters(self):
        """the tensors of :meth:`chain_parameter_names`, in its order"""
        return [t for name in self.CHAINS for lin in getattr(self, name).layers for t in (lin.weight, lin.bias)]

    def forward(self, *args, **kwargs):
        raise NotImplementedError("PECNet: only predict() is native; forward() (the CVAE path with its random sampling) is "
                                  "not implemented")

    def predict(self, past, generated_dest, mask, initial_pos):
        """past (N, 2 past_length), generated_dest (N, 2), mask (N, N) bool or float32, initial_pos (N, 2) ->
        (N, 2 (future_length - 1))"""
        if self.training and self.native_training:
            return _TrainPredict.apply(self, mask, past, generated_dest, initial_pos, *self.chain_parameters())
        require_eval(self, "PECNet")
        from . import ops
        return ops.pecnet_predict(self, past, generated_dest, mask, initial_pos)


def enable_native_training(model, flag=True):
    """Let ``model``'s predictor run in training mode with a native backward pass.  ``model`` is an
    :class:`eigentrajectory_amd.EigenTrajectory` wrapper or a bare predictor: an ``LBEBM`` (its own
    ``enable_native_training``), a ``PECNet``, a ``SocialImplicitLight``, an ``SGCN`` of its native family (``in_dims =
    1``, four heads, width 64, ``dropout = 0``, no position channel) or a ``GPGraph`` in the ET configuration around
    ``SGCN(position_channel=True, dropout=0)``, or a ``SocialSTGCNN`` of its native family (``n_stgcnn = 1``, no per-time-row
    graph, affine BatchNorms that track running statistics with one float momentum, no dropout; its training-mode forward
    uses BatchNorm batch statistics and updates the running ones), or a ``SocialDMRGCN`` of its native family (``n_stgcn =
    1``, every ``Dropout.p = 0``; its training-mode forward applies DropEdge through a keep mask it draws per call), or a
    ``GraphTERNLight`` of its native family (``n_epgcn = 1``, every ``Dropout.p = 0``; DropEdge on its float graphs through a
    keep mask it draws per call) (the plain attribute ``native_training``); the other two predictors have no native backward
    pass and raise.  -> ``model``"""
    from ._native_train import family_name
    from .gpgraph import GPGraph
    from .implicit import SocialImplicitLight
    from .lbebm import LBEBM
    net = model if isinstance(model, GPGraph) else getattr(model, "baseline_model", model)  # (a GPGraph has a base of its own)
    if isinstance(net, LBEBM):
        net.enable_native_training(flag)
    elif isinstance(net, (PECNet, SocialImplicitLight)):
        net.native_training = bool(flag)
    elif hasattr(net, "outside_native_training"):  # SGCN, GPGraph, SocialSTGCNN, SocialDMRGCN, GraphTERNLight: a family each
        why = net.outside_native_training()
        if why is not None:
            raise NotImplementedError(f"enable_native_training: {family_name(net)} has no native backward pass outside its "
                                      f"native family: {why}; {net.trains_natively}")
        net.native_training = bool(flag)
    else:
        raise NotImplementedError(f"enable_native_training: {type(net).__name__} has no native backward pass; only LBEBM, "
                                  "PECNet, SocialImplicitLight, SGCN, SocialSTGCNN, SocialDMRGCN and GraphTERNLight, and GPGraph "
                                  "around SGCN, train natively")
    return model
