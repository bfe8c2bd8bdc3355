"""Social-Implicit, the predictor of ET-Implicit (baseline/implicit/model.py: SocialImplicitLight), inference and training on
HIP kernels.

Same constructor signature and the same sub-module / parameter names as the reference
(``implicit_cells.{i}.{feat,highway_input,highway,tpcnn}.{weight,bias}``, the same under ``implicit_cells.{i}.ped.``, and
``implicit_cells.{i}.{noise_w,global_w,local_w}``), so a reference ET-Implicit checkpoint's ``baseline_model.*`` keys load
unchanged (``strict=True``), and the module plugs into :class:`eigentrajectory_amd.EigenTrajectory` through the existing
``implicit`` bridge::

    model = EigenTrajectory(SocialImplicitLight(spatial_input=1, spatial_output=hp.num_samples, temporal_input=hp.k + 2,
                                                temporal_output=hp.k, bins=[0, 0.01, 0.1, 1.2],
                                                noise_weight=[0.05, 1, 4, 8]),
                            get_hook_func("implicit"), hp).eval()

``forward(v)`` in eval mode is TWO launches of ``et_implicit_forward_graph`` (csrc/et_implicit.hip): v (1, 1, T, N) as the
bridge's pre-hook builds it -> (1, S, T_out, N).  A pedestrian's Social-Zone is the number of ``bins`` not greater than
``|v[0, 0, 0, n]|``, minus one (exact fp32 comparisons); each zone has its own cell, which sees the zone's pedestrians
compacted in scene order.  The weights are read in place from this module's tensors (a ``load_state_dict``, a ``.to()`` or
an in-place edit is seen by the next call, and by a captured graph's next replay).  ``bins`` and ``noise_weight`` are plain
attributes (constructor constants of the reference, not part of the state_dict); in the Light form the noise is
identically zero, so the ``noise_w`` term is not computed -- ``noise_w`` is a parameter only so that checkpoints load (a
non-finite ``noise_w``, whose product with the zero noise is NaN in the reference, is not reproduced).
A whole split runs as two launches through :meth:`EigenTrajectory.evaluate_split` /
:func:`eigentrajectory_amd.ops.implicit_forward_scenes`.
Supported family: ``spatial_input = 1``, ``1 <= spatial_output <= 64``, ``temporal_input, temporal_output <= 16``, 1 to 8
ascending bins; other shapes construct, but their forward raises.

Training (opt-in): the Light form has no dropout, no BatchNorm and no sampling, so its training-mode forward IS its eval
forward.  After ``eigentrajectory_amd.enable_native_training(model)`` a ``forward(v)`` in training mode runs the same two
launches as a ``torch.autograd.Function`` whose backward is two launches more (csrc/et_implicit.hip, "backward"): the
gradients of the 18 tensors of every cell that the forward reads, each pedestrian's contribution formed on its own from its
five gathered columns and added in a fixed order, no atomics.  They reach ``.grad`` the ordinary autograd way, as views of
one block; every ``noise_w`` gets an exact zero (the reference's is a sum of products with the zero noise).  ``v`` gets no
gradient (the bridge detaches it): a ``v`` that requires one raises.  A cell that no pedestrian of the scene is in gets
exact zeros where the reference leaves ``.grad`` None ("Implicit training")::

    model = EigenTrajectory(SocialImplicitLight(...), get_hook_func("implicit"), hp)
    eigentrajectory_amd.enable_native_training(model)
    ETTrainer(model, hp, train_data, val_data, mode="sequenced").fit(epochs)

The switch is the plain attribute ``native_training`` (no parameter, no buffer, not in the ``state_dict``, default False);
without it a forward in training mode raises, as before.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib as L
from ._native_train import train_forward


class _SocialCellLocal(nn.Module):
    """The local stream: per pedestrian, 1-d convolutions over time (spatial section) and over the S axis with time as
    channels (temporal section)."""

    def __init__(self, spatial_input, spatial_output, temporal_input, temporal_output):
        super().__init__()
        self.feat = nn.Conv1d(spatial_input, spatial_output, 3, padding=1)
        self.highway_input = nn.Conv1d(spatial_input, spatial_output, 1)
        self.highway = nn.Conv1d(temporal_input, temporal_output, 1)
        self.tpcnn = nn.Conv1d(temporal_input, temporal_output, 3, padding=1)


class _SocialCellGlobal(nn.Module):
    """One Social-Zone's cell: the global stream's 2-d convolutions over the (time, pedestrian) and (S, pedestrian) planes,
    the local stream ``ped`` and the three learnt scalars."""

    def __init__(self, spatial_input, spatial_output, temporal_input, temporal_output, noise_w):
        super().__init__()
        self.feat = nn.Conv2d(spatial_input, spatial_output, 3, padding=1)
        self.highway_input = nn.Conv2d(spatial_input, spatial_output, 1)
        self.highway = nn.Conv2d(temporal_input, temporal_output, 1)
        self.tpcnn = nn.Conv2d(temporal_input, temporal_output, 3, padding=1)
        self.noise_w = nn.Parameter(torch.zeros(1))
        self.noise_weights = noise_w
        self.global_w = nn.Parameter(torch.zeros(1))
        self.local_w = nn.Parameter(torch.zeros(1))
        self.ped = _SocialCellLocal(spatial_input, spatial_output, temporal_input, temporal_output)


_TENSORS = ("feat", "highway_input", "highway", "tpcnn")


class SocialImplicitLight(nn.Module):
    r"""baseline/implicit/model.py's ``SocialImplicitLight`` (inference in eval mode; training mode after
    :func:`eigentrajectory_amd.enable_native_training`).  ``forward(v)``: v (1, 1, T, N) as the implicit bridge's pre-hook
    builds it -> (1, S, T_out, N)."""

    native_training = False  # a plain attribute, set per instance by eigentrajectory_amd.enable_native_training

    def __init__(self, spatial_input=2, spatial_output=2, temporal_input=8, temporal_output=12,
                 bins=[0, 0.01, 0.1, 1.2], noise_weight=[0.05, 1, 4, 8]):
        super().__init__()
        bins, noise_weight = [float(b) for b in bins], [float(w) for w in noise_weight]
        if not bins:
            raise ValueError("SocialImplicitLight: bins is empty; a Social-Zone needs a lower bound")
        if len(noise_weight) < len(bins):
            raise ValueError(f"SocialImplicitLight: {len(bins)} bins need as many noise weights, got {len(noise_weight)}")
        if min(spatial_input, spatial_output, temporal_input, temporal_output) < 1:
            raise ValueError("SocialImplicitLight: spatial_input, spatial_output, temporal_input and temporal_output are "
                             "channel counts and must be positive")
        #: ascending zone bounds and the per-zone noise scales (model.py:127-128), constructor constants
        self.bins, self.noise_weight = bins, noise_weight
        self.spatial_input, self.spatial_output = spatial_input, spatial_output
        self.temporal_input, self.temporal_output = temporal_input, temporal_output
        self.implicit_cells = nn.ModuleList(
            [_SocialCellGlobal(spatial_input, spatial_output, temporal_input, temporal_output, noise_weight) for _ in bins])

    def et_params(self):
        """-> (et_implicit_params, device): this module's tensors as the kernel reads them (include/eigentraj.h)."""
        p = L.ImplicitParams()
        p.spatial_input, p.spatial_output = self.spatial_input, self.spatial_output
        p.temporal_input, p.temporal_output = self.temporal_input, self.temporal_output
        dev = L.module_device("SocialImplicitLight", self)
        bins = [float(b) for b in self.bins]
        if len(bins) != len(self.implicit_cells):
            raise L.ETLibraryError(f"SocialImplicitLight: {len(bins)} bins for {len(self.implicit_cells)} cells")
        p.n_bins = len(bins)
        if len(bins) > L.IMPLICIT_MAX_BINS:
            return p, dev  # the kernel answers ET_ERR_UNSUPPORTED
        for b, val in enumerate(bins):
            p.bins[b] = val
        for i, cell in enumerate(self.implicit_cells):
            c = p.cells[i]
            for j, name in enumerate(_TENSORS):
                g, l = getattr(cell, name), getattr(cell.ped, name)
                c.global_t[2 * j], c.global_t[2 * j + 1] = g.weight.data_ptr(), g.bias.data_ptr()
                c.local_t[2 * j], c.local_t[2 * j + 1] = l.weight.data_ptr(), l.bias.data_ptr()
            c.noise_w, c.global_w, c.local_w = cell.noise_w.data_ptr(), cell.global_w.data_ptr(), cell.local_w.data_ptr()
        return p, dev

    def cell_parameter_names(self):
        """the state_dict keys of every cell's 19 tensors: the 8 of the global stream, the 8 of ``ped``, then the scalars"""
        per_cell = [f"{prefix}{name}.{kind}" for prefix in ("", "ped.") for name in _TENSORS for kind in ("weight", "bias")]
        return [f"implicit_cells.{i}.{key}" for i in range(len(self.implicit_cells))
                for key in per_cell + ["noise_w", "global_w", "local_w"]]

    def cell_parameters(self):
        """the tensors of :meth:`cell_parameter_names`, in its order"""
        own = dict(self.named_parameters())
        return [own[name] for name in self.cell_parameter_names()]

    native_parameters = cell_parameters  # what :mod:`._native_train` differentiates

    def native_forward(self, et, v):
        from . import ops
        v = L.on_device(v, et[1])
        ws = ops.implicit_workspace(self, v.shape[-1], et_params=et)  # (holds the neighbour table for the backward)
        return ops.implicit_forward_graph(self, v, workspace=ws, et_params=et), (v, *(() if ws is None else (ws,)))

    def native_backward(self, et, kept, g_out):
        from . import ops
        v, ws = kept if len(kept) == 2 else (kept[0], None)
        views = ops.implicit_grad_views(self, ops.implicit_backward_graph(self, v, ws, g_out, et_params=et))
        zero = torch.zeros((len(self.implicit_cells), 1), device=v.device)  # noise_w: an exact zero each, one fill
        return [views[name] if name in views else zero[int(name.split(".")[1])] for name in self.cell_parameter_names()]

    def forward(self, v):
        if self.training and self.native_training:
            if v.requires_grad:
                raise RuntimeError("SocialImplicitLight: no input gradient is built (the implicit bridge detaches v); v "
                                   "requires one")
            return train_forward(self, v)
        if self.training:
            raise RuntimeError("SocialImplicitLight: only inference is native; training-mode forward and backward are not "
                               "implemented -- call .eval() first")
        from . import ops
        return ops.implicit_forward_graph(self, v)
