"""ETDescriptor -- the reference's EigenTrajectory/descriptor.py interface on HIP kernels.

Reference: EigenTrajectory/descriptor.py:6-181.  Same constructor, parameters
(``U_obs_trunc`` (2*t_obs,k), ``U_pred_trunc`` (2*t_pred,k), so reference
checkpoints load unchanged) and methods.  What differs is the execution:

* ``projection`` is ONE kernel (normaliser state + normalise + U^T x), the
  reference's is ~15 ATen launches (descriptor.py:157-159, normalizer.py:17-51);
* ``reconstruction`` is ONE kernel for all S samples, the reference loops over S in
  Python (descriptor.py:173-175, ~6*S launches);
* ``truncated_SVD`` forms the 2T x 2T Gram matrix in fp64 on the GPU and
  diagonalises it (Jacobi) instead of LAPACK gesdd on the (2T x N) matrix
  (descriptor.py:109-110).  Eigenvector signs are this build's convention (largest
  component positive); LAPACK's are unspecified.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from .normalizer import TrajNorm


class ETDescriptor(nn.Module):
    r"""Truncated-SVD descriptor of normalised trajectories (descriptor.py:6-27 of the reference).

    ``hyper_params``: DotDict (``obs_len, pred_len, obs_svd, pred_svd, k, num_samples, traj_dim``); the three flags
    choose which of origin / rotation / scale the embedded :class:`TrajNorm` removes."""

    def __init__(self, hyper_params, norm_ori=True, norm_rot=True, norm_sca=True):
        super().__init__()

        self.hyper_params = hyper_params
        self.t_obs, self.t_pred = hyper_params.obs_len, hyper_params.pred_len
        self.obs_svd, self.pred_svd = hyper_params.obs_svd, hyper_params.pred_svd
        self.k = hyper_params.k
        self.s = hyper_params.num_samples
        self.dim = hyper_params.traj_dim
        if self.dim != 2:
            raise ValueError("the HIP descriptor kernels are written for traj_dim == 2 (normalizer.py rotates in 2-D)")
        self.traj_normalizer = TrajNorm(ori=norm_ori, rot=norm_rot, sca=norm_sca)

        self.U_obs_trunc = nn.Parameter(torch.zeros((self.t_obs * self.dim, self.k)))
        self.U_pred_trunc = nn.Parameter(torch.zeros((self.t_pred * self.dim, self.k)))

    # The fused kernels implement the reference's only configuration of the flags
    # (norm_ori=norm_rot=True, norm_sca per descriptor: model.py:29-30).
    @property
    def _fused(self):
        tn = self.traj_normalizer
        return tn.ori and tn.rot

    @property
    def _mode(self):
        return ops.MODE_MOVING if self.traj_normalizer.sca else ops.MODE_STATIC

    def normalize_trajectory(self, obs_traj, pred_traj=None):
        r"""descriptor.py:29-44: normaliser state from the observations, applied to both halves"""
        tn = self.traj_normalizer
        tn.calculate_params(obs_traj)
        return tn.normalize(obs_traj), (None if pred_traj is None else tn.normalize(pred_traj))

    def denormalize_trajectory(self, traj_norm):
        r"""Trajectory denormalization (descriptor.py:46-57)"""
        return self.traj_normalizer.denormalize(traj_norm)

    def to_ET_space(self, traj, evec):
        r"""Euclidean -> ET: C = evec^T . traj.reshape(N, 2T)^T   (descriptor.py:59-73) -> (k,N)"""
        tdim = evec.size(0)
        traj = traj.reshape(-1, tdim // 2, 2)
        C, _, _, _ = ops.norm_project(traj, None, None, None, evec, None, ops.MODE_IDENTITY,
                                      want_nrm=False, want_flag=False)
        return C

    def to_Euclidean_space(self, C, evec):
        r"""ET -> Euclidean: (evec . C)^T reshaped to (N,T,2)   (descriptor.py:75-89)"""
        out = ops.anchor_reconstruct(C.unsqueeze(-1), None, None, None, evec, ops.MODE_IDENTITY)
        return out[0]

    def truncated_SVD(self, traj, k=None, full_matrices=False):
        r"""Truncated SVD of M = traj.reshape(N,2T)^T (descriptor.py:91-114) via the Gram matrix.

        Returns U_trunc (2T,k), S_trunc (k,), V_trunc (N,k) like the reference (U up to sign).
        """
        assert traj.size(2) == self.dim  # NTC
        k = self.k if k is None else k
        # Gram of the rows as they are (identity normalisation); obs and pred slots both get `traj`
        G, _, _ = ops.fit_gram(traj, traj, ops.MODE_IDENTITY, which=0)
        U, S = ops.eigh_topk(G, k)
        C = self.to_ET_space(traj, U)               # (k,N) = S * V^T
        V = (C / S[:, None]).T
        return U, S, V

    def parameter_initialization(self, obs_traj, pred_traj):
        r"""Initialize the ET descriptor parameters (descriptor.py:116-142; call once before training)"""
        if self._fused:
            U_obs_trunc, U_pred_trunc = ops.fit_descriptor(obs_traj, pred_traj, self.k, self._mode, which=self._mode)[:2]  # three launches
            self.traj_normalizer.calculate_params(obs_traj)
            pred_traj_norm = self.traj_normalizer.normalize(pred_traj)
        else:  # any other flag combination: stand-alone normalise, then one Gram + eigh per half
            obs_norm, pred_traj_norm = self.normalize_trajectory(obs_traj, pred_traj)
            U_obs_trunc, U_pred_trunc = self.truncated_SVD(obs_norm)[0], self.truncated_SVD(pred_traj_norm)[0]

        # fresh Parameters like descriptor.py:134-135 (the reference re-registers instead of copying in place)
        for name, U in (("U_obs_trunc", U_obs_trunc), ("U_pred_trunc", U_pred_trunc)):
            setattr(self, name, nn.Parameter(U.to(getattr(self, name).device)))
        return pred_traj_norm, U_pred_trunc  # what the anchor fit consumes (model.py:55-56)

    def projection(self, obs_traj, pred_traj=None):
        r"""Trajectory projection to the ET space (descriptor.py:144-160) -> C_obs (k,N), C_pred (k,N)|None"""
        if not self._fused:
            obs_norm, pred_norm = self.normalize_trajectory(obs_traj, pred_traj)
            C_obs = self.to_ET_space(obs_norm, self.U_obs_trunc.detach())
            return C_obs, (None if pred_norm is None else self.to_ET_space(pred_norm, self.U_pred_trunc.detach()))
        mv = self._mode == ops.MODE_MOVING
        u_o, u_p = self.U_obs_trunc.detach(), self.U_pred_trunc.detach()
        C_obs, C_pred, nrm, _ = ops.norm_project(obs_traj, pred_traj, u_o if mv else None, u_p if mv else None,
                                                 None if mv else u_o, None if mv else u_p, self._mode, want_flag=False)
        self.traj_normalizer._from_nrm(nrm, obs_traj.shape[1])  # the state reconstruction() will use
        return C_obs, C_pred

    def reconstruction(self, C_pred):
        r"""Trajectory reconstruction from the ET space (descriptor.py:162-176): (k,N,S) -> (S,N,T_pred,2)"""
        tn = self.traj_normalizer
        if not self._fused or tn._nrm is None:
            # generic path: bare U.C for every sample, then the stand-alone denormalise
            s = C_pred.shape[2]
            flat = ops.anchor_reconstruct(C_pred, None, None, None, self.U_pred_trunc.detach(), ops.MODE_IDENTITY)
            return torch.stack([self.denormalize_trajectory(flat[i]) for i in range(s)], dim=0)
        mv = self._mode == ops.MODE_MOVING
        u_p = self.U_pred_trunc.detach()
        return ops.anchor_reconstruct(C_pred, None, None, u_p if mv else None, None if mv else u_p, self._mode,
                                      nrm=tn._nrm, t_obs=tn._t_obs)

    def forward(self, C_pred):
        r"""nn.Module call == :meth:`reconstruction` (descriptor.py:178-181)"""
        return self.reconstruction(C_pred)
