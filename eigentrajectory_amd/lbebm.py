"""LBEBM, the predictor of ET-LBEBM (baseline/lbebm/model.py), inference on HIP kernels.

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
"""
from __future__ import annotations

import torch.nn as nn

from . import _lib as L
from .pecnet import MLP, check_tensors, require_eval


def _arg(args, name):
    return args[name] if isinstance(args, dict) else getattr(args, name)


class LBEBM(nn.Module):
    """baseline/lbebm/model.py's ``LBEBM``: ``predict`` natively in eval mode, everything else a tensor holder."""

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

    def et_params(self):
        """-> (et_mlp_params, device): the three chains ``predict`` runs (no pooling, no initial_pos)."""
        p = L.MLPParams()
        p.fdim, p.nonlocal_pools, p.non_local_dim, p.pos_width = self.fdim, 0, 0, 0
        p.out_width = self.predictor.layers[-1].out_features
        for name in ("encoder_past", "encoder_dest", "predictor"):
            getattr(self, name).et_chain(getattr(p, name), f"LBEBM.{name}")
        return p, check_tensors(self, "LBEBM")

    def forward(self, *args, **kwargs):
        raise NotImplementedError("LBEBM: only predict() is native; forward() (Langevin sampling of the latent, the CVAE "
                                  "path) is not implemented")

    def predict(self, past, generated_dest):
        """past (N, 2 past_length), generated_dest (N, 2 sub-goals) -> (N, 2 future_length)"""
        require_eval(self, "LBEBM")
        from . import ops
        return ops.lbebm_predict(self, past, generated_dest)
