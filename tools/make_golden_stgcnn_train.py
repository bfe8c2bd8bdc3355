#!/usr/bin/env python3
"""G31: ET-STGCNN training fixture -- the reference's Social-STGCNN (baseline/stgcnn/model.py: social_stgcnn, the ET
constructor arguments n_stgcnn=1, n_txpcnn=5, input_feat=1) in TRAINING mode on the CPU: its output, every parameter's
gradient and the three BatchNorms' buffers after the call.

    python tools/make_golden_stgcnn_train.py --ref <reference checkout> --out tests/golden

The reference's text is imported at run time and nothing of it is copied.  The weights and buffers are
tests/_stgcnn_train_cases.module's (seeded); the cases are configuration "et" at n = 1, 2, 3, 5, "tp3" as a second
configuration at the same sizes, and one recorded real scene (pick0 of tests/golden/g19_stgcnn.npz: its v and the bridge's a,
"et" only); the upstream gradients are tests/_stgcnn_train_cases.d_out's.  The script asserts that no kept PReLU input of a
case lies within the float64 restatement's STEP bound of 0 (tests/_stgcnn_train_np.py: the bound of the one step that forms
the input from exact kept inputs) and that the reference's fp32 and float64 runs take the same branch at every PReLU (read
with forward hooks: a branch that differs would make the reference's gradient one of two) -- on failure pick another seed
in tests/_stgcnn_train_cases.SEED.  RELAXED against the PROPAGATED bound: carried through three BatchNorms (each multiplies
a bound by 1 / sqrt(var + eps)) and four tpcnns, the whole-chain bound puts about 1 % of the ET shape's PReLU inputs inside
their band for every seed tried; the count per case goes into the manifest (``undecided_under_propagated_bound``), and the
GPU test asserts instead that the device's kept PReLU words have the float64 run's signs.  Stored per case <config>_n<n> / et_real:
  .config, .v (K, n), .a (K, n, n), .d_out (1, S, k, n)
  .out32 (S, k, n)                                    the fp32 run's output
  .grad32, .grad64                                    d sum(out * d_out) / d parameter of the fp32 and of the float64 run, every
                                                      parameter in state_dict order as one flat vector, zeros where .grad is None
  .<BatchNorm>.running_mean / .running_var / .num_batches_tracked   the float64 run's buffers after the call
Only data is written."""
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
    from tests import _stgcnn_train_cases as CS
    from tests import _stgcnn_train_np as TN
    out_dir = os.path.abspath(args.out)
    sys.path.insert(0, args.ref)
    os.chdir(args.ref)
    from baseline.stgcnn.model import social_stgcnn

    torch.set_num_threads(1)
    g19 = G.load("g19_stgcnn.npz")
    cases = [(name, f"{name}_n{n}", *CS.scene(name, n)) for name in ("et", "tp3") for n in CS.EXACT_N]
    cases.append(("et", "et_real", np.ascontiguousarray(g19["pick0.v"][0, 0]), np.ascontiguousarray(g19["pick0.a"])))
    store, loose = {}, {}
    for name, case, v, a in cases:
        n = v.shape[1]
        ours = CS.module(name)
        sd = CS.state(ours)
        d_out = CS.d_out(name, n)
        R = TN.run(sd, v, a, d_out, momentum=CS.MOMENTUM, eps=CS.EPS)
        assert R["decisions"]["prelu"]["undecided"] == 0, (case, R["decisions"])   # else: another seed
        loose[case] = TN.run(sd, v, a, d_out, momentum=CS.MOMENTUM, eps=CS.EPS, propagate=True)["decisions"]["prelu"]["undecided"]
        runs, signs = {}, {}
        for dtype in (torch.float32, torch.float64):
            ref = social_stgcnn(**CS.module_kw(name)).to(dtype)
            ref.load_state_dict({k: t.to(dtype) if t.is_floating_point() else t for k, t in ours.state_dict().items()}, strict=True)
            ref.train()
            seen = []
            hooks = [m.register_forward_hook(lambda mod, inp, res, seen=seen: seen.append((inp[0].detach() > 0).numpy().copy()))
                     for m in ref.modules() if isinstance(m, torch.nn.PReLU)]
            out = ref(torch.from_numpy(v[None, None]).to(dtype), torch.from_numpy(a).to(dtype))
            out.backward(torch.from_numpy(d_out).to(dtype))
            for h in hooks:
                h.remove()
            signs[dtype] = seen
            grad = np.concatenate([(torch.zeros_like(p) if p.grad is None else p.grad).detach().numpy().reshape(-1)
                                   for _, p in ref.named_parameters()])
            runs[dtype] = (out.detach().numpy()[0], grad, {k: b.detach().numpy() for k, b in ref.named_buffers()})
        assert len(signs[torch.float32]) == len(signs[torch.float64]) >= 2
        assert all(np.array_equal(p, q) for p, q in zip(signs[torch.float32], signs[torch.float64])), case   # else: another seed
        store[f"{case}.config"] = np.asarray(name)
        store[f"{case}.v"], store[f"{case}.a"], store[f"{case}.d_out"] = v, a, d_out
        store[f"{case}.out32"] = runs[torch.float32][0].astype(np.float32)
        store[f"{case}.grad32"] = runs[torch.float32][1].astype(np.float32)
        store[f"{case}.grad64"] = runs[torch.float64][1].astype(np.float64)
        for k, b in runs[torch.float64][2].items():
            store[f"{case}.{k}"] = b
    path = os.path.join(out_dir, "g31_stgcnn_train.npz")
    np.savez_compressed(path, **store)
    size = os.path.getsize(path)
    assert size <= os.path.getsize(os.path.join(out_dir, "g29_sgcn_train.npz")), size
    with open(os.path.join(out_dir, "MANIFEST_g31_stgcnn_train.json"), "w") as f:
        json.dump({"g31_stgcnn_train": {"cases": [c[1] for c in cases], "numpy": np.__version__, "torch": torch.__version__,
                                        "bytes": size,
                                        "undecided_under_propagated_bound": loose}}, f, indent=1)
        f.write("\n")
    print(f"wrote {path} ({size} bytes, {len(cases)} cases)")


if __name__ == "__main__":
    main()
