"""LBEBM, the predictor of ET-LBEBM (baseline/lbebm/model.py), inference and training of ``predict`` on HIP kernels.

Same constructor signature and the same sub-module / parameter names as the reference (``encoder_past.layers.{i}``,
``encoder_dest``, ``encoder_latent``, ``decoder``, ``predictor``, ``non_local_theta``, ``non_local_phi``, ``non_local_g``,
``EBM.{0,2,4}``), so a reference ET-LBEBM checkpoint's ``baseline_model.*`` keys load unchanged (``strict=True``), and the
module plugs into :class:`eigentrajectory_amd.EigenTrajectory` through the existing ``lbebm`` bridge, which calls
``predict`` only.  ``args`` is the reference's parameter object (attributes or keys ``nonlocal_pools``, ``non_local_dim``,
``non_local_theta_size``, ``non_local_phi_size``, ``non_local_g_size``, ``sub_goal_indexes``, ``ny``).

``predict(past, generated_dest)`` in eval mode is 2 launches of csrc/et_mlp.hip: ``encoder_past`` and ``encoder_dest`` side
by side, then ``predictor`` on their concatenation (gathered, never stored), every Linear on the f32-input MFMA in exact
fp32.  The weights are read in place from this module's tensors.  ``encoder_latent``, ``decoder``, the non-local MLPs and
``EBM`` only hold their tensors: ``forward`` (Langevin sampling, the CVAE path) and a ``predict`` in training mode raise.
A whole split runs in the same 2 launches through :meth:`EigenTrajectory.evaluate_split` /
:func:`eigentrajectory_amd.ops.lbebm_forward_scenes`.
Supported family: ``activation='relu'``, ``discrim=False``, ``dropout=-1``, 1 to 4 hidden layers per MLP, widths 1 to 1024;
the whole-split form takes one sub-goal (a destination of 2 numbers); other shapes construct, but their use raises.

Training (opt-in): the reference's ``lbebm`` bridge calls ``predict`` in training too, so training ET-LBEBM differentiates
exactly what ``predict`` computes.  After ``enable_native_training()`` a ``predict`` in training mode runs the same 2
launches with the activations kept, and its backward pass is 3 launches of csrc/et_mlp_train.hip (the predictor's rows,
both encoders' rows, every dW / db); the gradients reach ``.grad`` of the 20 tensors of ``encoder_past``, ``encoder_dest``
and ``predictor`` the ordinary autograd way, the other sub-modules get none (``predict`` does not touch them)::

    model = EigenTrajectory(LBEBM(...), get_hook_func("lbebm"), hp)
    model.baseline_model.enable_native_training()
    ETTrainer(model, hp, train_data, val_data).fit(epochs)

Without the call everything is as before: ``predict`` in training mode raises.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib as L
from .pecnet import MLP, require_eval


def _arg(args, name):
    return args[name] if isinstance(args, dict) else getattr(args, name)


class _TrainPredict(torch.autograd.Function):
    """``predict`` with a backward pass (csrc/et_mlp_train.hip).  The 20 tensors of the three chains are inputs, so their
    gradients accumulate into ``.grad`` like any other parameter's; they, the inputs and the kept activations are saved
    through ``save_for_backward``: the kernels read the weights in place, and an in-place change between forward and
    backward (an optimiser step) is caught by autograd's version counters."""

    @staticmethod
    def forward(ctx, model, past, dest, *params):
        from . import ops
        out, saved = ops.lbebm_train_fwd(model, past, dest)
        ctx.model = model
        ctx.save_for_backward(past, dest, saved, *params)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, g_out):
        need = ctx.needs_input_grad
        if g_out is None:
            return (None,) * len(need)
        from . import ops
        past, dest, saved = ctx.saved_tensors[:3]
        model = ctx.model
        if any(p.data_ptr() != q.data_ptr() for p, q in zip(ctx.saved_tensors[3:], model.chain_parameters())):
            raise RuntimeError("LBEBM: a parameter tensor of the three chains was replaced between forward and backward")
        g = ops.lbebm_train_bwd(model, past, dest, saved, g_out, (need[1], need[2]))
        return (None, g.get("past"), g.get("dest"),
                *(g[name] if wanted else None for name, wanted in zip(model.chain_parameter_names(), need[3:])))


class LBEBM(nn.Module):
    """baseline/lbebm/model.py's ``LBEBM``: ``predict`` natively (eval mode; training mode after
    :meth:`enable_native_training`), everything else a tensor holder."""

    CHAINS = ("encoder_past", "encoder_dest", "predictor")  # what ``predict`` runs

    def __init__(self, enc_past_size, enc_dest_size, enc_latent_size, dec_size, predictor_size, fdim, zdim, sigma,
                 past_length, future_length, args):
        super().__init__()
        self.fdim, self.zdim, self.sigma, self.args = fdim, zdim, sigma, args
        self.nonlocal_pools = _arg(args, "nonlocal_pools")
        non_local_dim, goals = _arg(args, "non_local_dim"), len(_arg(args, "sub_goal_indexes"))
        self.encoder_past = MLP(past_length * 2, fdim, enc_past_size)
        self.encoder_dest = MLP(goals * 2, fdim, enc_dest_size)
        self.encoder_latent = MLP(2 * fdim, 2 * zdim, enc_latent_size)
        self.decoder = MLP(fdim + zdim, goals * 2, dec_size)
        self.predictor = MLP(2 * fdim, 2 * future_length, predictor_size)
        self.non_local_theta = MLP(fdim, non_local_dim, _arg(args, "non_local_theta_size"))
        self.non_local_phi = MLP(fdim, non_local_dim, _arg(args, "non_local_phi_size"))
        self.non_local_g = MLP(fdim, fdim, _arg(args, "non_local_g_size"))
        self.EBM = nn.Sequential(nn.Linear(zdim + fdim, 200), nn.GELU(), nn.Linear(200, 200), nn.GELU(),
                                 nn.Linear(200, _arg(args, "ny")))
        self.native_training = False

    def enable_native_training(self, flag=True):
        """Let ``predict`` run in training mode, with a native backward pass (a plain attribute: no parameter, no buffer,
        not in the ``state_dict``).  -> self"""
        self.native_training = bool(flag)
        return self

    def chain_parameter_names(self):
        return [f"{name}.layers.{i}.{kind}" for name in self.CHAINS for i in range(len(getattr(self, name).layers))
                for kind in ("weight", "bias")]

    def chain_parameters(self):
        """the tensors of :meth:`chain_parameter_names`, in its order"""
        return [t for name in self.CHAINS for lin in getattr(self, name).layers for t in (lin.weight, lin.bias)]

    def et_params(self):
        """-> (et_mlp_params, device): the three chains ``predict`` runs (no pooling, no initial_pos)."""
        p = L.MLPParams()
        p.fdim, p.nonlocal_pools, p.non_local_dim, p.pos_width = self.fdim, 0, 0, 0
        p.out_width = self.predictor.layers[-1].out_features
        for name in ("encoder_past", "encoder_dest", "predictor"):
            getattr(self, name).et_chain(getattr(p, name), f"LBEBM.{name}")
        return p, L.module_device("LBEBM", self)

    def forward(self, *args, **kwargs):
        raise NotImplementedError("LBEBM: only predict() is native; forward() (Langevin sampling of the latent, the CVAE "
                                  "path) is not implemented")

    def predict(self, past, generated_dest):
        """past (N, 2 past_length), generated_dest (N, 2 sub-goals) -> (N, 2 future_length)"""
        if self.training and self.native_training:
            return _TrainPredict.apply(self, past, generated_dest, *self.chain_parameters())
        require_eval(self, "LBEBM")
        from . import ops
        return ops.lbebm_predict(self, past, generated_dest)
