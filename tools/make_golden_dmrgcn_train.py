#!/usr/bin/env python3
"""G32: ET-DMRGCN training fixture -- the reference's social_dmrgcn (baseline/dmrgcn/predictor.py, the ET constructor
arguments n_stgcn=1, input_feat=1, kernel_size=3) in TRAINING mode on the CPU: the DropEdge masks it drew, its output and
every parameter's gradient.

    python tools/make_golden_dmrgcn_train.py --ref <reference checkout> --out tests/golden

The reference's text is imported at run time and nothing of it is copied.  Its normalizer moves its identity matrices to
the GPU (``torch.eye(...).cuda()``); for the duration of this script ``Tensor.cuda`` / ``Module.cuda`` are the identity, as
in tools/make_golden_dmrgcn.py -- the arithmetic is the reference's own.  The weights are
tests/_dmrgcn_train_cases.random_state's (seeded); the cases are configuration "et" (S = 20, k = 6, K = 8, n_tpcnn = 4) and
"tp1" at n = 1, 2, 3, 5 (tests/_dmrgcn_train_cases.scene) and one recorded real scene (pick4 of tests/golden/g23_dmrgcn.npz:
its v, 14 pedestrians, "et" only); ``a`` is the reference bridge's generate_adjacency_matrix(v), asserted equal to
tests/_dmrgcn_np.adjacency(v) bit for bit and therefore not stored; the upstream gradients are
tests/_dmrgcn_train_cases.d_out's.

The draw.  Every case's forward runs under ``torch.manual_seed(SEED)``, set after the networks are built;
``torch.rand_like`` is wrapped for the duration of the fp32 run and records what drop_edge drew (two draws per forward,
relation 0 first); the float64 run replays the same masks (a float64 ``rand_like`` under the same seed draws other
numbers).  The script asserts
  * that ``SocialDMRGCN.draw_keep`` under the same CPU seed yields the same masks,
  * that no kept PReLU input of a case lies within the float64 restatement's STEP bound of 0 (tests/_dmrgcn_train_np.py),
    and that the restatement's PReLU inputs are the float64 run's,
  * that the reference's fp32 and float64 runs take the same branch at every PReLU (forward hooks),
  * that the restatement reproduces the float64 output and gradients within 1e-9.
SEED is the first seed for which all of this holds in every case; no case is left out.  Stored per case
<config>_n<n> / et_real:
  .config, .v (K, n), .d_out (1, S, k, n), .keep_bits (the (2, 5, K, n, n) mask, bit-packed)
  .out32, .out64 (S, k, n)     the outputs of the fp32 and of the float64 run
  .grad64                      d sum(out * d_out) / d parameter of the float64 run, every parameter in state_dict order as
                               one flat vector (the fp32 run's gradients are not stored: the ET shape has 14 156 parameters and
                               nothing compares with them; their largest distance from grad64 is in the manifest)
and per configuration net.<config>.<state_dict key>.  Only data is written."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

F64 = 1e-9
SEEDS = range(1, 50)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    from tests import _dmrgcn_np as DN
    from tests import _dmrgcn_train_cases as CS
    from tests import _dmrgcn_train_np as TN
    from tests import _golden as G
    sys.path.insert(0, args.ref)
    torch.Tensor.cuda = lambda self, *a, **k: self   # no GPU in the build container: the reference's normalizer stays on the CPU
    torch.nn.Module.cuda = lambda self, *a, **k: self
    from baseline.dmrgcn.bridge import generate_adjacency_matrix
    from baseline.dmrgcn.predictor import social_dmrgcn
    torch.set_num_threads(1)
    g23 = G.load("g23_dmrgcn.npz")

    cases = [(f"{name}_n{n}", name, CS.scene(name, n)[0]) for name in ("et", "tp1") for n in CS.EXACT_N]
    cases.append(("et_real", "et", np.ascontiguousarray(g23["pick4.v"][0, 0], np.float32)))
    states = {name: CS.random_state(name) for name in ("et", "tp1")}
    rand_like = torch.rand_like

    def reference(name, dtype):
        net = social_dmrgcn(**CS.module_kw(name))
        net.load_state_dict({q: torch.from_numpy(t) for q, t in states[name].items()}, strict=True)
        return net.to(dtype).train()

    def run(net, v, a, d_out, draw):
        """one training-mode forward and backward with ``draw`` in rand_like's place -> (out, flat grads, PReLU inputs)"""
        seen, hooks = [], []
        for m in net.modules():
            if isinstance(m, torch.nn.PReLU):
                hooks.append(m.register_forward_hook(lambda mod, inp, out: seen.append(inp[0].detach().clone().numpy())))
        dtype = next(net.parameters()).dtype
        torch.rand_like = draw
        try:
            out, _ = net(torch.from_numpy(v)[None, None].to(dtype), a.to(dtype))
        finally:
            torch.rand_like = rand_like
        net.zero_grad()
        out.backward(torch.from_numpy(d_out).to(dtype))
        for h in hooks:
            h.remove()
        flat = np.concatenate([p.grad.numpy().reshape(-1) for p in net.parameters()])
        return out.detach().numpy()[0], flat, seen

    def attempt(seed):
        out, info = {}, {}
        for case, name, v in cases:
            sd = states[name]
            n = v.shape[1]
            a = generate_adjacency_matrix(torch.from_numpy(v)[None, None])              # (1, 2, K, n, n)
            assert np.array_equal(a.numpy()[0], DN.adjacency(v)), case
            d_out = CS.d_out(name, n)
            drawn = []

            def record(x):
                drawn.append(rand_like(x))
                return drawn[-1]

            net32, net64 = reference(name, torch.float32), reference(name, torch.float64)   # (their construction draws too)
            torch.manual_seed(seed)
            out32, grad32, pre32 = run(net32, v, a, d_out, record)
            assert len(drawn) == 2 and all(tuple(d.shape) == (1, 5, v.shape[0], n, n) for d in drawn), case
            keep = torch.cat([~(d > 0.8) for d in drawn]).to(torch.uint8)
            import eigentrajectory_amd as ET
            mine = ET.SocialDMRGCN(**CS.module_kw(name))
            torch.manual_seed(seed)
            mine = mine.draw_keep(n, "cpu")
            assert mine.dtype == torch.uint8 and torch.equal(mine, keep), f"{case}: draw_keep differs from the reference's draw"
            replay = iter(keep)
            out64, grad64, pre64 = run(net64, v, a, d_out,
                                       lambda x: torch.where(next(replay)[None] != 0, 0.0, 1.0).to(x.dtype))
            if len(pre32) != len(pre64) or any(((p > 0) != (q > 0)).any() for p, q in zip(pre32, pre64)):
                return None, f"{case}: the fp32 and float64 runs branch differently at a PReLU"
            R = TN.run(sd, v, a.numpy()[0], d_out[0], keep=keep.numpy())
            if R["decisions"]["prelu"]["undecided"]:
                return None, f"{case}: {R['decisions']['prelu']['undecided']} PReLU inputs inside their step bound"
            kept = R["kept"]
            mine_pre = [kept["yp"].val, kept["s"].val]
            for j in range(len(kept["z"])):
                mine_pre += [kept["c0"][j].val, kept["c1"][j].val, kept["z"][j].val]
            assert len(mine_pre) == len(pre64), case
            for p, q in zip(mine_pre, pre64):   # (the tpcnn inputs are (1, k, S, n); the GTA's (1, S, 1, n))
                assert np.abs(p.reshape(-1) - q.reshape(-1)).max() <= F64 * max(np.abs(q).max(), 1e-300), case
            assert np.abs(R["out"].val - out64).max() <= F64 * np.abs(out64).max(), case
            at = 0
            for q, g in R["grads"].items():
                want = grad64[at:at + g.val.size].reshape(g.shape)
                tol = F64 * max(np.abs(want).max(), 1e-300) + (0.0 if g.tm is None else 2.0 ** -40 * float(np.max(g.tm)))
                assert np.abs(g.val - want).max() <= tol, (case, q)   # (tests/test_dmrgcn_train_cpu.py: _equal)
                at += g.val.size
            assert at == grad64.size
            out.update({f"{case}.config": np.array(name), f"{case}.v": v, f"{case}.d_out": d_out,
                        f"{case}.keep_bits": CS.pack_bits(keep.numpy()), f"{case}.out32": out32.astype(np.float32),
                        f"{case}.out64": out64, f"{case}.grad64": grad64})
            info[case] = dict(n=int(n), kept_fraction=float(keep.float().mean()),
                              grad32_vs_grad64=float(np.abs(grad32 - grad64).max() / np.abs(grad64).max()))
        return out, info

    for seed in SEEDS:
        out, info = attempt(seed)
        if out is not None:
            break
        print(f"seed {seed}: {info}")
    else:
        raise SystemExit("no seed in range satisfies every case")
    for name, sd in states.items():
        out.update({f"net.{name}.{q}": t for q, t in sd.items()})
    out["seed"] = np.array(seed)
    path = os.path.join(args.out, "g32_dmrgcn_train.npz")
    np.savez_compressed(path, **out)
    manifest = {"g32_dmrgcn_train": {"cases": [c for c, _, _ in cases], "seed": int(seed), "numpy": np.__version__,
                                     "torch": torch.__version__, "bytes": os.path.getsize(path), "per_case": info}}
    with open(os.path.join(args.out, "MANIFEST_g32_dmrgcn_train.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")
    print(f"wrote {path}: {os.path.getsize(path)} bytes, seed {seed}")


if __name__ == "__main__":
    main()
