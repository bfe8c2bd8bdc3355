#!/usr/bin/env python3
"""G30: ET-GPGraph-SGCN training fixture -- the reference's GPGraph (baseline/gpgraphsgcn: model_groupwrapper.py around
model_baseline.py's TrajectoryModel, the ET configuration) in TRAINING mode on the CPU, its output, its group index and
every parameter's gradient.

    python tools/make_golden_gpgraph_sgcn_train.py --ref <reference checkout> --out tests/golden

The reference's text is imported at run time and nothing of it is copied; `Tensor.cuda` / `Module.cuda` are the identity for
the duration of this script, as in tools/make_golden_gpgraph_sgcn.py, and the float64 run sets torch's default dtype (the
reference's pooling allocates with the default).  The weights are tests/_gpgraph_train_cases.case_state's ("et" and "k1"), the
inputs its scenes of 1, 2, 3 and 5 and, for "et", of 17; the upstream gradients are tests/_gpgraph_train_cases.d_out's.  With
dropout = 0 the reference's F.dropout is the identity: the script asserts that the training-mode output equals the eval-mode
output bit for bit, that no mask logit of a case is within DELTA of 0 and that no pair distance is within BAND_D th of th (a
decision inside a band would make the reference's gradient one of two).  Stored per case <config>_n<n>:
  .config, .th, .v_abs (T, n), .v_rel (2, T, n), .d_out (S, k, n)
  .out32 (S, k, n), .indices (n,)                    the fp32 run's output, the group index (both runs': asserted equal)
  .grad64                                            d sum(out * d_out) / d parameter of the float64 run, every parameter in
                                                     state_dict order as one flat vector
Rank-deficient gradients are stored packed (tests/_gpgraph_train_cases.g30_gradients rebuilds them; the script asserts that
the residual is below 1e-12 of the matrix): an attention's query.weight / key.weight is M = F B^T with B the embedding's
columns and bias ((64, 2) spatial, (64, 3) temporal), stored as F; group_mix.st_gcns_mix.1.weight is sum_i g_i act_i^T =
G A^T with G = d_out as (S k, n), stored as A (3 S k, n).  Only data is written."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    from tests import _gpgraph_np as GN
    from tests import _gpgraph_train_cases as CS
    from tests import _sgcn_np as SN
    args.out = os.path.abspath(args.out)
    sys.path.insert(0, args.ref)
    os.chdir(args.ref)
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    _zeros_like = torch.zeros_like

    def zeros_like_cpu(x, *a, **k):   # (the reference's zeros_like(..., device='cuda') stays on the CPU)
        k.pop("device", None)
        return _zeros_like(x, *a, **k)
    torch.zeros_like = zeros_like_cpu
    from baseline.gpgraphsgcn.model_baseline import TrajectoryModel
    from baseline.gpgraphsgcn.model_groupwrapper import GPGraph

    torch.set_num_threads(1)
    cases = [(name, n) for name in ("et", "k1") for n in CS.EXACT_N] + [("et", 17)]
    out = {}
    for name, n in cases:
        case = f"{name}_n{n}"
        c = SN.CONFIGS[name]
        va, vr = CS.scene(name, n)
        sd = CS.case_state(name, [va])
        d_out = CS.d_out(name, n)
        runs = {}
        for dtype in (torch.float32, torch.float64):
            torch.set_default_dtype(dtype)
            base = TrajectoryModel(**SN.module_cfg(name))
            net = GPGraph(baseline_model=base, in_channels=1, out_channels=c["S"], obs_seq_len=c["k"] + 2, pred_seq_len=c["k"],
                          d_type="learned_l2norm", d_th="learned", mix_type="mlp", group_type=(True, True, True), weight_share=True)
            net.load_state_dict({k: torch.from_numpy(w) for k, w in sd.items()})
            net = net.to(dtype)
            store = {"ls": [], "lt": []}
            im = net.baseline_model.sparse_weighted_adjacency_matrices.interaction_mask
            im.spatial_output.register_forward_pre_hook(lambda m, a, s=store: s["ls"].append(a[0].detach().clone()))
            im.temporal_output.register_forward_pre_hook(lambda m, a, s=store: s["lt"].append(a[0].detach().clone()))
            a, r = torch.from_numpy(va).to(dtype)[None, None], torch.from_numpy(vr).to(dtype)[None]
            net.eval()
            with torch.no_grad():
                res_eval, idx_eval = net(a, r)
            store["ls"].clear(), store["lt"].clear()
            net.train()
            res, idx = net(a, r)
            assert torch.equal(res.detach(), res_eval) and torch.equal(idx, idx_eval), case   # dropout = 0
            res.backward(torch.from_numpy(d_out).to(dtype)[None])
            runs[dtype] = (res.detach().numpy()[0], idx.numpy().astype(np.int64), {k: p.grad.numpy() for k, p in net.named_parameters()},
                           min(float(x.abs().min()) for x in store["ls"] + store["lt"]))
        torch.set_default_dtype(torch.float32)
        o32, i32, _, _ = runs[torch.float32]
        o64, i64, g64, min_logit = runs[torch.float64]
        _, rest = GN.split_state(sd)
        th = GN.threshold(rest)
        assert np.array_equal(i32, i64), case
        assert min_logit >= SN.DELTA, (case, min_logit)
        assert GN.pair_margin(GN.distances(rest, va), th) > GN.BAND_D, case
        assert list(g64) == list(sd), case
        out[f"{case}.config"], out[f"{case}.th"] = np.array(name), np.float32(th)
        out[f"{case}.v_abs"], out[f"{case}.v_rel"], out[f"{case}.d_out"] = va, vr, d_out
        out[f"{case}.out32"], out[f"{case}.indices"] = o32, i64
        parts = []
        Sk = c["S"] * c["k"]
        for k in sd:
            if k.endswith(("query.weight", "key.weight")):
                F, res = CS.pack(sd, k, g64[k])
                assert res <= 1e-12, (case, k, res)
                parts.append(F.reshape(-1))
            elif k == "group_mix.st_gcns_mix.1.weight":
                A, res = CS.pack_mix(d_out, g64[k])
                assert res <= 1e-12, (case, k, res)
                parts.append(A.reshape(-1))
            else:
                parts.append(g64[k].reshape(-1))
        out[f"{case}.grad64"] = np.concatenate(parts).astype(np.float64)
        print(case, "G", int(i64.max()) + 1, "out", float(np.abs(o32 - o64).max()), "min |logit|", min_logit, "floats", out[f"{case}.grad64"].size, "Sk", Sk)
    path = os.path.join(args.out, "g30_gpgraph_sgcn_train.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(args.out, "MANIFEST_g30_gpgraph_sgcn_train.json"), "w") as f:
        json.dump({"g30_gpgraph_sgcn_train": {"cases": [f"{nm}_n{n}" for nm, n in cases], "numpy": np.__version__,
                                              "torch": torch.__version__, "bytes": os.path.getsize(path)}}, f, indent=1)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
