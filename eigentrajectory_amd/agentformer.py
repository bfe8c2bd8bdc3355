"""AgentFormer, the predictor of ET-AgentFormer (baseline/agentformer/model.py: AgentFormerLight), inference on HIP kernels.

Same constructor (one configuration object) and the same sub-module, parameter and buffer names as the reference
(``context_encoder.{input_fc, tf_encoder.layers.{i}, pos_encoder.{pe, fc}}``, ``future_decoder.{input_fc,
tf_decoder.layers.{i}, pos_encoder.{pe, fc}, out_fc}``, every layer's ``self_attn`` / ``multihead_attn`` with
``in_proj_weight``, ``in_proj_bias``, ``in_proj_weight_self``, ``in_proj_bias_self`` and ``out_proj``), so a reference
ET-AgentFormer checkpoint's ``baseline_model.*`` keys load unchanged (``strict=True``), and the module plugs into
:class:`eigentrajectory_amd.EigenTrajectory` through the existing ``agentformer`` bridge::

    model = EigenTrajectory(AgentFormerLight(et_config(hp.k, hp.num_samples)), get_hook_func("agentformer"), hp).eval()

``cfg`` is the reference's ``Config`` object or any mapping / namespace with the same field names; :func:`et_config` returns
the settings ET uses (utils/trainer.py:387-392 on top of agentformer_pre.yml).  ``set_data(data)`` takes the bridge's
``pre_motion`` (T, N, 1); ``forward()`` runs ``et_agentformer_forward_graph`` (csrc/et_agentformer.hip; 1 + 2 encoder layers
+ 4 decoder layers launches) and fills ``self.data``.  The reference's k-pass decoder loop feeds the same input every pass
(``nz = 0``) under a block-causal mask, so its last pass alone gives every output: the native path runs ONE decoder pass.
The weights are read in place from this module's tensors (a ``load_state_dict``, a ``.to()`` or an in-place edit is seen by
the next call, and by a captured graph's next replay).  Training (the backward pass) is not implemented natively: a
forward in training mode raises.  A whole split runs in a fixed number of launches through
:meth:`EigenTrajectory.evaluate_split` / :func:`eigentrajectory_amd.ops.agentformer_forward_scenes`.

Supported family: ``motion_dim = 1``, ``tf_model_dim`` a multiple of 16 up to 256, ``head_dim`` a multiple of 4,
``tf_ff_dim <= 512``, 1 to 4 layers each side, ``past_frames, future_frames <= 16``, ``1 <= forecast_dim <= 64``, scenes of
up to 128 pedestrians; ``input_type = ['pos']``, ``pred_type = 'pos'``, ``nz = 0``, no learnt prior, ``pos_concat``, no agent
encoding, ``tf_cfg``: no gaussian kernel, ``sep_attn``; ``conn_dist >= 1000`` (an all-zero agent mask); no ``out_mlp_dim``.
A configuration outside it raises at construction and names the field.
"""
from __future__ import annotations

import math
from collections import defaultdict

import torch
import torch.nn as nn

from . import _lib as L

_MISSING = object()


def cfg_get(cfg, name, default=None):
    """field ``name`` of a configuration: a mapping, a namespace, or an object with the reference's ``get``"""
    if cfg is None:
        return default
    if isinstance(cfg, dict):
        return cfg.get(name, default)
    val = getattr(cfg, name, _MISSING)
    if val is _MISSING and hasattr(cfg, "get"):
        val = cfg.get(name, _MISSING)
    return default if val is _MISSING else val


def et_config(k, num_samples, **overrides):
    """The settings EigenTrajectory builds AgentFormer with for ``k`` coefficients and ``num_samples`` samples: the
    model section of agentformer_pre.yml with the trainer's overrides."""
    cfg = dict(past_frames=k + 2, future_frames=k, motion_dim=1, forecast_dim=num_samples, input_type=["pos"],
               pred_type="pos", sn_out_type=None, scene_orig_all_past=False, nz=0, ar_train=False, learn_prior=False,
               pos_concat=True, tf_model_dim=256, tf_ff_dim=512, tf_nhead=8, tf_dropout=0.1, tf_cfg={},
               context_encoder={"nlayer": 2}, future_decoder={"nlayer": 2}, loss_cfg={})
    cfg.update(overrides)
    return cfg


def build_pos_enc(max_len, d_model):
    """the sinusoidal table (max_len, 1, d_model): sin on the even columns, cos on the odd ones"""
    pe = torch.zeros(max_len, d_model)
    position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe.unsqueeze(1)


class AgentAwareAttention(nn.Module):
    """The tensors of agentformer_lib.py's AgentAwareAttention (sep_attn on)."""

    def __init__(self, embed_dim, num_heads):
        super().__init__()
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * embed_dim))
        self.out_proj = nn.Linear(embed_dim, embed_dim)
        self.in_proj_weight_self = nn.Parameter(torch.empty(2 * embed_dim, embed_dim))
        self.in_proj_bias_self = nn.Parameter(torch.zeros(2 * embed_dim))
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.xavier_uniform_(self.in_proj_weight_self)
        nn.init.constant_(self.out_proj.bias, 0.)

    def fill(self, a):
        a.in_proj_weight, a.in_proj_bias = self.in_proj_weight.data_ptr(), self.in_proj_bias.data_ptr()
        a.in_proj_weight_self, a.in_proj_bias_self = self.in_proj_weight_self.data_ptr(), self.in_proj_bias_self.data_ptr()
        a.out_proj_weight, a.out_proj_bias = self.out_proj.weight.data_ptr(), self.out_proj.bias.data_ptr()


class _Layer(nn.Module):
    def __init__(self, d_model, nhead, ff, decoder):
        super().__init__()
        self.self_attn = AgentAwareAttention(d_model, nhead)
        if decoder:
            self.multihead_attn = AgentAwareAttention(d_model, nhead)
        self.linear1 = nn.Linear(d_model, ff)
        self.linear2 = nn.Linear(ff, d_model)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        if decoder:
            self.norm3 = nn.LayerNorm(d_model)

    def fill(self, y):
        self.self_attn.fill(y.self_attn)
        norms = [self.norm1, self.norm2]
        if hasattr(self, "multihead_attn"):
            self.multihead_attn.fill(y.multihead_attn)
            norms.append(self.norm3)
        y.linear1_weight, y.linear1_bias = self.linear1.weight.data_ptr(), self.linear1.bias.data_ptr()
        y.linear2_weight, y.linear2_bias = self.linear2.weight.data_ptr(), self.linear2.bias.data_ptr()
        for j, nm in enumerate(norms):
            y.norm_weight[j], y.norm_bias[j] = nm.weight.data_ptr(), nm.bias.data_ptr()


class AgentFormerEncoderLayer(_Layer):
    def __init__(self, d_model, nhead, ff):
        super().__init__(d_model, nhead, ff, False)


class AgentFormerDecoderLayer(_Layer):
    def __init__(self, d_model, nhead, ff):
        super().__init__(d_model, nhead, ff, True)


class _Stack(nn.Module):
    def __init__(self, layers):
        super().__init__()
        self.layers = nn.ModuleList(layers)


class PositionalAgentEncoding(nn.Module):
    """pos_concat form: ``fc(cat[x, pe[t]])``; ``pe`` is a buffer of ``max_t_len`` rows, as in the reference"""

    def __init__(self, d_model, max_t_len=200):
        super().__init__()
        self.register_buffer("pe", build_pos_enc(max_t_len, d_model))
        self.fc = nn.Linear(2 * d_model, d_model)

    def fill(self, e):
        e.fc_weight, e.fc_bias, e.pe = self.fc.weight.data_ptr(), self.fc.bias.data_ptr(), self.pe.data_ptr()


class ContextEncoder(nn.Module):
    def __init__(self, motion_dim, d_model, nhead, ff, nlayer):
        super().__init__()
        self.input_fc = nn.Linear(motion_dim, d_model)
        self.tf_encoder = _Stack([AgentFormerEncoderLayer(d_model, nhead, ff) for _ in range(nlayer)])
        self.pos_encoder = PositionalAgentEncoding(d_model)


class FutureDecoder(nn.Module):
    def __init__(self, motion_dim, forecast_dim, d_model, nhead, ff, nlayer):
        super().__init__()
        self.input_fc = nn.Linear(motion_dim, d_model)
        self.tf_decoder = _Stack([AgentFormerDecoderLayer(d_model, nhead, ff) for _ in range(nlayer)])
        self.pos_encoder = PositionalAgentEncoding(d_model)
        self.out_fc = nn.Linear(d_model, forecast_dim)
        nn.init.zeros_(self.out_fc.bias)


def _check_family(cfg):
    """raise ValueError naming the first field that puts ``cfg`` outside what the kernels compute"""
    def bad(field, got, want):
        raise ValueError(f"AgentFormerLight: {field} = {got!r} is outside the native family ({want})")

    input_type = cfg_get(cfg, "input_type", "pos")
    input_type = [input_type] if isinstance(input_type, str) else list(input_type)
    if cfg_get(cfg, "nz") != 0:
        bad("nz", cfg_get(cfg, "nz"), "0: no latent code")
    if cfg_get(cfg, "learn_prior", False):
        bad("learn_prior", True, "False")
    if input_type != ["pos"]:
        bad("input_type", input_type, "['pos']")
    if cfg_get(cfg, "pred_type", input_type[0]) != "pos":
        bad("pred_type", cfg_get(cfg, "pred_type"), "'pos'")
    if list(cfg_get(cfg, "dec_input_type", [])):
        bad("dec_input_type", cfg_get(cfg, "dec_input_type"), "[]")
    if not cfg_get(cfg, "pos_concat", False):
        bad("pos_concat", False, "True")
    if cfg_get(cfg, "use_agent_enc", False):
        bad("use_agent_enc", True, "False")
    tf_cfg = cfg_get(cfg, "tf_cfg", {})
    if cfg_get(tf_cfg, "gaussian_kernel", False):
        bad("tf_cfg.gaussian_kernel", True, "False")
    if not cfg_get(tf_cfg, "sep_attn", True):
        bad("tf_cfg.sep_attn", False, "True")
    if cfg_get(cfg, "conn_dist", 100000.0) < 1000.0:
        bad("conn_dist", cfg_get(cfg, "conn_dist"), ">= 1000: an all-zero agent mask")
    dec = cfg_get(cfg, "future_decoder", {})
    if cfg_get(dec, "out_mlp_dim", None) is not None:
        bad("future_decoder.out_mlp_dim", cfg_get(dec, "out_mlp_dim"), "None")
    if cfg_get(dec, "pos_offset", False):
        bad("future_decoder.pos_offset", True, "False")
    if cfg_get(cfg, "motion_dim") != 1:
        bad("motion_dim", cfg_get(cfg, "motion_dim"), "1")
    D, H, ff = cfg_get(cfg, "tf_model_dim"), cfg_get(cfg, "tf_nhead"), cfg_get(cfg, "tf_ff_dim")
    if not (isinstance(D, int) and 16 <= D <= 256 and D % 16 == 0):
        bad("tf_model_dim", D, "a multiple of 16 up to 256")
    if not (isinstance(H, int) and H >= 1 and D % H == 0 and (D // H) % 4 == 0):
        bad("tf_nhead", H, "divides tf_model_dim into a head_dim that is a multiple of 4")
    if not (isinstance(ff, int) and 1 <= ff <= 512):
        bad("tf_ff_dim", ff, "1 to 512")
    for side in ("context_encoder", "future_decoder"):
        nl = cfg_get(cfg_get(cfg, side, {}), "nlayer", 6)
        if not 1 <= nl <= L.AGENTFORMER_MAX_LAYERS:
            bad(f"{side}.nlayer", nl, f"1 to {L.AGENTFORMER_MAX_LAYERS}")
    for name in ("past_frames", "future_frames"):
        if not 1 <= cfg_get(cfg, name) <= 16:
            bad(name, cfg_get(cfg, name), "1 to 16")
    if not 1 <= cfg_get(cfg, "forecast_dim") <= 64:
        bad("forecast_dim", cfg_get(cfg, "forecast_dim"), "1 to 64")


class AgentFormerLight(nn.Module):
    r"""baseline/agentformer/model.py's ``AgentFormerLight`` (eval-mode inference on the GPU).

    ``set_data(data)`` takes ``data['pre_motion']`` (T, N, 1); ``forward()`` fills and returns ``self.data``, a
    ``defaultdict(lambda: None)`` with ``_dec_motion`` (N, k, S), ``_seq_out`` (k, N, S), ``pre_motion``, ``agent_num`` and
    ``batch_size``.  The reference also stores ``scene_orig``, ``pre_motion_scene_norm``, ``pre_vel``, ``cur_motion``,
    ``pre_motion_norm``, ``agent_enc_shuffle``, ``agent_mask``, ``context_enc``, ``agent_context`` and ``p_z_dist``; none of
    them feeds the output in this configuration and they are not formed here."""

    def __init__(self, cfg):
        super().__init__()
        _check_family(cfg)
        self.cfg = cfg
        self.past_frames, self.future_frames = cfg_get(cfg, "past_frames"), cfg_get(cfg, "future_frames")
        self.motion_dim, self.forecast_dim = cfg_get(cfg, "motion_dim"), cfg_get(cfg, "forecast_dim")
        self.model_dim, self.ff_dim = cfg_get(cfg, "tf_model_dim"), cfg_get(cfg, "tf_ff_dim")
        self.nhead = cfg_get(cfg, "tf_nhead")
        n_enc = cfg_get(cfg_get(cfg, "context_encoder", {}), "nlayer", 6)
        n_dec = cfg_get(cfg_get(cfg, "future_decoder", {}), "nlayer", 6)
        self.data = None
        self.context_encoder = ContextEncoder(self.motion_dim, self.model_dim, self.nhead, self.ff_dim, n_enc)
        self.future_decoder = FutureDecoder(self.motion_dim, self.forecast_dim, self.model_dim, self.nhead, self.ff_dim,
                                            n_dec)

    def et_params(self):
        """-> (et_agentformer_params, device): this module's tensors as the kernels read them (include/eigentraj.h)."""
        dev = L.module_device("AgentFormerLight", self, buffers=True)  # (its one buffer: the positional encoding)
        p = L.AgentFormerParams()
        p.motion_dim, p.model_dim, p.ff_dim, p.nhead = self.motion_dim, self.model_dim, self.ff_dim, self.nhead
        p.forecast_dim, p.past_frames, p.future_frames = self.forecast_dim, self.past_frames, self.future_frames
        enc, dec = self.context_encoder, self.future_decoder
        p.n_enc, p.n_dec = len(enc.tf_encoder.layers), len(dec.tf_decoder.layers)
        for side, e in ((enc, p.enc_embed), (dec, p.dec_embed)):
            e.input_fc_weight, e.input_fc_bias = side.input_fc.weight.data_ptr(), side.input_fc.bias.data_ptr()
            side.pos_encoder.fill(e)
        p.out_fc_weight, p.out_fc_bias = dec.out_fc.weight.data_ptr(), dec.out_fc.bias.data_ptr()
        for i, layer in enumerate(enc.tf_encoder.layers):
            layer.fill(p.enc[i])
        for i, layer in enumerate(dec.tf_decoder.layers):
            layer.fill(p.dec[i])
        return p, dev

    def set_data(self, data):
        pre = data["pre_motion"]
        self.data = defaultdict(lambda: None)
        self.data["batch_size"] = self.data["agent_num"] = pre.shape[1]
        self.data["pre_motion"] = pre.contiguous()

    def forward(self):
        if self.training:
            raise RuntimeError("AgentFormerLight: only inference is native; training-mode forward and backward are not "
                               "implemented -- call .eval() first")
        if self.data is None:
            raise RuntimeError("AgentFormerLight: set_data() first")
        from . import ops
        seq_out = ops.agentformer_forward_graph(self, self.data["pre_motion"])
        self.data["_seq_out"] = seq_out
        self.data["_dec_motion"] = seq_out.transpose(0, 1).contiguous()
        return self.data
