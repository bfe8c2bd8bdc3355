#!/usr/bin/env python3
"""Time ET-AgentFormer inference over test splits (weights drawn from the seed recorded in
tests/golden/g26_agentformer_net.npz, descriptors of G2) three ways:

  split   EigenTrajectory.evaluate_split: projection -> et_agentformer_forward_scenes (14 launches) -> fused metrics
  hook    the default per-scene path with the native module: EigenTrajectory.evaluate once per scene (bridge pre-hook,
          AgentFormerLight.forward = et_agentformer_forward_graph, 13 launches, metrics)
  torch   an outside yardstick: the same network written with stock torch ops (matmul / softmax / layer_norm, fp32) on the
          same GPU, scene by scene in the reference's k-pass decoder form -- the predictor alone, no projection or metrics

    python tools/time_agentformer.py [--reps 5] [--splits eth,hotel,univ]

Prints one JSON line per split: median wall ms per whole split with a device synchronisation at both ends (median of
--reps after one warm-up call), the predictor's launches alone as ``scenes_ms``, the workspace bytes of the whole-split
call, the matrix FLOPs of one pass (Linear layers, Q K^T, P V) and the fraction of the 157.3 TFLOP/s f32 MFMA rate that
``scenes_ms`` amounts to."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
PEAK_F32_MFMA = 157.3e12


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def torch_attention(sd, pre, x, mem, n, nhead, causal):
    D = x.shape[1]
    hd = D // nhead
    W, B, Ws, Bs = sd[pre + "in_proj_weight"], sd[pre + "in_proj_bias"], sd[pre + "in_proj_weight_self"], \
        sd[pre + "in_proj_bias_self"]
    scale = float(hd) ** -0.5
    q = F.linear(x, W[:D], B[:D]) * scale
    kv = F.linear(mem, W[D:], B[D:])
    qs = F.linear(x, Ws[:D], Bs[:D]) * scale
    ks = F.linear(mem, Ws[D:], Bs[D:])
    heads = lambda t: t.view(t.shape[0], nhead, hd).transpose(0, 1)
    s = heads(q) @ heads(kv[:, :D]).transpose(1, 2)
    s_self = heads(qs) @ heads(ks).transpose(1, 2)
    iq, ik = torch.arange(x.shape[0], device=x.device), torch.arange(mem.shape[0], device=x.device)
    s = torch.where((iq[:, None] % n) == (ik[None, :] % n), s_self, s)
    if causal:
        s = s.masked_fill((ik[None, :] // n) > (iq[:, None] // n), float("-inf"))
    out = (torch.softmax(s, dim=-1) @ heads(kv[:, D:])).transpose(0, 1).reshape(x.shape[0], D)
    return F.linear(out, sd[pre + "out_proj.weight"], sd[pre + "out_proj.bias"])


def torch_layer(sd, pre, x, mem, n, nhead, decoder):
    D = x.shape[1]
    ln = lambda t, i: F.layer_norm(t, (D,), sd[f"{pre}norm{i}.weight"], sd[f"{pre}norm{i}.bias"])
    x = ln(x + torch_attention(sd, pre + "self_attn.", x, x, n, nhead, decoder), 1)
    if decoder:
        x = ln(x + torch_attention(sd, pre + "multihead_attn.", x, mem, n, nhead, False), 2)
    y = F.linear(F.relu(F.linear(x, sd[pre + "linear1.weight"], sd[pre + "linear1.bias"])), sd[pre + "linear2.weight"],
                 sd[pre + "linear2.bias"])
    return ln(x + y, 3 if decoder else 2)


def torch_forward(sd, u, nhead, n_enc, n_dec):
    """u (T, n) -> (k, n, S), the decoder run k times over 1 .. k frames as the reference runs it"""
    T, n = u.shape
    k = T - 2
    E, Fd = "context_encoder.", "future_decoder."

    def embed(side, vals, frames):
        x = F.linear(vals[:, None], sd[side + "input_fc.weight"], sd[side + "input_fc.bias"])
        cat = torch.cat([x, sd[side + "pos_encoder.pe"][:frames, 0].repeat_interleave(n, dim=0)], dim=1)
        return F.linear(cat, sd[side + "pos_encoder.fc.weight"], sd[side + "pos_encoder.fc.bias"])

    x = embed(E, u.reshape(-1), T)
    for i in range(n_enc):
        x = torch_layer(sd, f"{E}tf_encoder.layers.{i}.", x, None, n, nhead, False)
    out = None
    for frames in range(1, k + 1):
        y = embed(Fd, u[-1].repeat(frames), frames)
        for i in range(n_dec):
            y = torch_layer(sd, f"{Fd}tf_decoder.layers.{i}.", y, x, n, nhead, True)
        out = F.linear(y, sd[Fd + "out_fc.weight"], sd[Fd + "out_fc.bias"]).view(frames, n, -1)
    return out


def matrix_flops(sizes, T, k, D, ff, S, n_enc, n_dec):
    """2 x multiply-adds of one pass: the token-wise Linear layers and, per scene, Q K^T and P V of every attention"""
    n = float(sum(sizes))
    sq = float(sum(s * s for s in sizes))
    enc_tok = 2 * D * D + n_enc * (5 * D * D + D * D + 2 * D * ff)
    dec_tok = 2 * D * D + n_dec * (5 * D * D + D * D + 2 * D * D + D * D + 2 * D * ff) + D * S
    mem_tok = n_dec * 3 * D * D
    attn = sq * (n_enc * T * T + n_dec * (k * k + k * T)) * 2 * D
    return 2.0 * (n * T * (enc_tok + mem_tok) + n * k * dec_tok + attn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--splits", default="eth,hotel,univ")
    args = ap.parse_args()
    from eigentrajectory_amd import EigenTrajectory, _lib, ops
    from eigentrajectory_amd.agentformer import AgentFormerLight, et_config
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    from tests import _agentformer_np as AN
    from tests import _golden as G
    z, g2 = G.load("g26_agentformer_net.npz"), G.load("g2_fit_all_scenes.npz")
    dev = torch.device("cuda:0")
    drawn = AN.fixture_weights(z, "et")
    for scene in args.splits.split(","):
        hp = default_hyper_params(static_dist=float(z[f"{scene}.static_dist"]))
        native = AgentFormerLight(et_config(6, 20))
        own = native.state_dict()
        native.load_state_dict({k: own[k] if v is None else torch.from_numpy(v) for k, v in drawn.items()})
        model = EigenTrajectory(native, get_hook_func("agentformer"), hp)
        msd = model.state_dict()
        for k in msd:
            if k.startswith("ET_"):
                msd[k] = torch.from_numpy(g2[f"{scene}.{k}"])
        model.load_state_dict(msd)
        model = model.to(dev).eval()
        obs_np, pred_np, sse = G.dataset(scene, "test")
        sse = np.asarray(sse)
        obs, pred = torch.from_numpy(obs_np).to(dev), torch.from_numpy(pred_np).to(dev)
        scenes = [(obs[s:e].contiguous(), pred[s:e].contiguous()) for s, e in sse]
        sizes = (sse[:, 1] - sse[:, 0]).tolist()
        U_obs_m, _, U_obs_s, _ = model._U()
        C_obs, _, nrm, _ = ops.norm_project(obs, None, U_obs_m, None, U_obs_s, None, ops.MODE_SPLIT, model.static_dist,
                                            want_flag=False)
        _, det = ops.agentformer_forward_scenes(native, C_obs, nrm, scene_sizes=sizes, want_details=True)
        inputs = [det["graph_inputs"][:, s:e].contiguous() for s, e in sse]
        sd = dict(native.state_dict())
        n_enc, n_dec = len(native.context_encoder.tf_encoder.layers), len(native.future_decoder.tf_decoder.layers)

        def per_scene():
            with torch.no_grad():
                for o, p in scenes:
                    model.evaluate(o, p)

        def stock():
            with torch.no_grad():
                for u in inputs:
                    torch_forward(sd, u, native.nhead, n_enc, n_dec)

        params, _ = native.et_params()
        flops = matrix_flops(sizes, 8, 6, 256, 512, 20, n_enc, n_dec)
        rec = {"split": scene, "scenes": len(sse), "pedestrians": int(obs.shape[0]), "max_scene": int(max(sizes)),
               "launches": 2 + 2 * n_enc + 4 * n_dec,
               "workspace_bytes": int(_lib.lib().et_agentformer_workspace_bytes(C.byref(params), obs.shape[0], max(sizes))),
               "split_ms": timed(lambda: model.evaluate_split(obs, pred, sse), args.reps),
               "scenes_ms": timed(lambda: ops.agentformer_forward_scenes(native, C_obs, nrm, scene_sizes=sizes), args.reps),
               "hook_ms": timed(per_scene, args.reps), "torch_ms": timed(stock, args.reps), "matrix_gflop": flops / 1e9}
        rec["hook_over_split"] = rec["hook_ms"] / rec["split_ms"]
        rec["torch_over_scenes"] = rec["torch_ms"] / rec["scenes_ms"]
        rec["f32_mfma_fraction"] = flops / (rec["scenes_ms"] * 1e-3) / PEAK_F32_MFMA
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
