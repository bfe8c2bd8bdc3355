#!/usr/bin/env python3
"""G29: ET-SGCN training fixture -- the reference's SGCN (baseline/sgcn: TrajectoryPredictor, the ET constructor arguments of
tools/make_golden_sgcn_net.py) in TRAINING mode on the CPU, its output and every parameter's gradient.

    python tools/make_golden_sgcn_train.py --ref <reference checkout> --out tests/golden

The reference's text is imported at run time and nothing of it is copied; `Tensor.cuda` / `Module.cuda` are the identity
for the duration of this script, as in tools/make_golden_sgcn.py.  The weights are tests/_sgcn_np.random_state's ("et", and
"k1" as a second configuration); the inputs are tests/_sgcn_train_cases' scenes of 1, 2, 3 and 5 and one recorded real
scene (a pick of tests/golden/g20_sgcn_net.npz, "et" only); the upstream gradients are tests/_sgcn_train_cases.d_out's.  With
dropout = 0 the reference's F.dropout is the identity: the script asserts that the training-mode output equals the eval-mode
output bit for bit, and that no mask logit of a case is within DELTA of 0 (a decision inside the band would make the
reference's gradient one of two).  Stored per case <config>_n<n> / et_real:
  .config, .v (T, n), .d_out (k, n, S)
  .out32 (k, n, S), .logit_s32, .logit_t32           the fp32 run
  .grad32, .grad64                                    d sum(out * d_out) / d parameter of the fp32 and of the float64 run, every
                                                      parameter in state_dict order as one flat vector
                                                      (.grad32 of the ET shape: n = 5 only)
The gradient of an attention's query.weight / key.weight is sum_i d q_i e_i^T with e_i = x_i we + be (one input channel):
a (64, 64) matrix of rank two, M = F [we be]^T.  The four matrices are two thirds of the ET shape's 21 050 parameters, so
they are stored as their factors F (64, 2), the least-squares solution, in the matrix's place
(tests/_sgcn_train_cases.g29_gradients rebuilds M); the script asserts that the float64 run's residual is below 1e-12 of the matrix (the fp32 run's, rounding noise,
goes into the manifest).  Only data is written."""
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
    from tests import _golden as G
    from tests import _sgcn_np as SN
    from tests import _sgcn_train_cases as CS
    sys.path.insert(0, args.ref)
    os.chdir(args.ref)
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    _zeros_like = torch.zeros_like

    def zeros_like_cpu(x, *a, **k):
        k.pop("device", None)
        return _zeros_like(x, *a, **k)
    torch.zeros_like = zeros_like_cpu
    from baseline.sgcn import TrajectoryPredictor

    torch.set_num_threads(1)
    g20 = G.load("g20_sgcn_net.npz")
    args.out = os.path.abspath(os.path.join(REPO, args.out)) if not os.path.isabs(args.out) else args.out
    cases = [(name, f"{name}_n{n}", CS.scene(name, n)) for name in ("et", "k1") for n in CS.EXACT_N]
    cases.append(("et", "et_real", np.asarray(g20["pick2.v"], np.float32).reshape(8, -1)))
    out, residual32 = {}, 0.0
    for name, case, v in cases:
        n = v.shape[1]
        sd = SN.random_state(name)
        d_out = CS.d_out(name, n)
        ids, idt = SN.bridge_identities(v.shape[0], n)
        runs = {}
        for dtype in (torch.float32, torch.float64):
            net = TrajectoryPredictor(**SN.module_cfg(name))
            net.load_state_dict({k: torch.from_numpy(w) for k, w in sd.items()})
            net = net.to(dtype)
            store = {}
            im = net.sparse_weighted_adjacency_matrices.interaction_mask
            im.spatial_output.register_forward_pre_hook(lambda m, a: store.__setitem__("logit_s", a[0].detach().clone()))
            im.temporal_output.register_forward_pre_hook(lambda m, a: store.__setitem__("logit_t", a[0].detach().clone()))
            graph = torch.from_numpy(v).to(dtype)[None, :, :, None]
            ident = [torch.from_numpy(ids).to(dtype), torch.from_numpy(idt).to(dtype)]
            net.eval()
            with torch.no_grad():
                res_eval = net(graph, ident)
            net.train()
            res = net(graph, ident)
            assert torch.equal(res.detach(), res_eval), case   # dropout = 0: training mode IS eval mode
            res.backward(torch.from_numpy(d_out).to(dtype))
            runs[dtype] = (res.detach().numpy(), {k: p.grad.numpy() for k, p in net.named_parameters()},
                           store["logit_s"].numpy(), store["logit_t"].numpy())
        o32, g32, ls, lt = runs[torch.float32]
        o64, g64, ls64, lt64 = runs[torch.float64]
        assert min(np.abs(ls64).min(), np.abs(lt64).min()) >= SN.DELTA, (case, np.abs(ls64).min(), np.abs(lt64).min())
        assert sorted(g64) == sorted(sd), case
        out[f"{case}.config"], out[f"{case}.v"], out[f"{case}.d_out"] = np.array(name), v, d_out
        out[f"{case}.out32"] = o32.reshape(d_out.shape)
        out[f"{case}.logit_s32"], out[f"{case}.logit_t32"] = ls.reshape(v.shape[0], 4, n, n), lt.reshape(n, 4, v.shape[0], v.shape[0])
        for tag, g in (("grad32", g32), ("grad64", g64)):   # one flat vector per run, state_dict order
            if tag == "grad32" and case in ("et_n1", "et_n2", "et_n3", "et_real"):
                continue   # the file's size: the fp32 run's gradients of the ET shape are kept for n = 5
            parts = []
            for k in sd:
                if k.endswith(("query.weight", "key.weight")):
                    F, res = CS.pack(sd, k, g[k])
                    parts.append(F.reshape(-1))
                    if tag == "grad64":
                        assert res <= 1e-12, (case, k, res)
                    else:
                        residual32 = max(residual32, res)
                else:
                    parts.append(g[k].reshape(-1))
            out[f"{case}.{tag}"] = np.concatenate(parts).astype(np.float32 if tag == "grad32" else np.float64)
        print(case, "n =", n, "out", float(np.abs(o32 - o64).max()), "min |logit|", float(min(np.abs(ls64).min(), np.abs(lt64).min())))
    path = os.path.join(args.out, "g29_sgcn_train.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(args.out, "MANIFEST_g29_sgcn_train.json"), "w") as f:
        json.dump({"g29_sgcn_train": {"cases": [c for _, c, _ in cases], "numpy": np.__version__, "torch": torch.__version__,
                                      "bytes": os.path.getsize(path),
                                      "rank_two_residual_fp32_run": residual32}}, f, indent=1)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
