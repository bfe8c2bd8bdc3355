#!/usr/bin/env python3
"""G35: ET-Graph-TERN training fixture -- the reference's graph_tern_light (baseline/graphtern/model.py, the ET constructor
arguments n_epgcn=1, input_feat=1) in TRAINING mode on the CPU: the DropEdge mask it drew, its output and every parameter's
gradient.

    python tools/make_golden_graphtern_train.py --ref <reference checkout> --out tests/golden

The reference's text is imported at run time and nothing of it is copied.  Its normalizer moves its identity matrices to
the GPU (``torch.eye(...).cuda()``); for the duration of this script ``Tensor.cuda`` / ``Module.cuda`` are the identity, as
in tools/make_golden_graphtern.py -- the arithmetic is the reference's own.  The weights are
tests/_graphtern_train_cases.random_state's (seeded); the cases are CASES below (tests/_graphtern_train_cases.scene); S_obs
is the reference bridge's model_forward_pre_hook(u), asserted equal to tests/_graphtern_np.s_obs_of(u) bit for bit and
therefore stored as ``u`` alone; the upstream gradients are tests/_graphtern_train_cases.d_out's.

The draw.  Every case's forward runs under ``torch.manual_seed(SEED)``, set after the networks are built;
``torch.rand_like`` is wrapped for the duration of the fp32 run and records what drop_edge drew (one draw per forward, of
the float tensor A (1, 4, T, n, n)); the float64 run replays the same mask (a float64 ``rand_like`` under the same seed draws
other numbers) on the same fp32 distances (the reference's generate_adjacency_matrix on the fp32 S_obs, their inverses
formed in float64: a float64 subtraction would hand the network another input).  The script asserts
  * that ``GraphTERNLight.draw_keep`` under the same CPU seed yields the same mask,
  * that no kept PReLU input of a case lies within the float64 restatement's STEP bound of 0
    (tests/_graphtern_train_np.py), and that the restatement's PReLU inputs are the float64 run's,
  * that the reference's fp32 and float64 runs take the same branch at every PReLU (forward hooks),
  * that the restatement reproduces the float64 output and gradients within 1e-9.
SEED is the first seed for which all of this holds in every case; no case is left out.  Stored per case <config>_n<n>:
  .config, .u (T, n), .d_out (1, k, n, S), .keep_bits (the (4, T, n, n) mask, bit-packed)
  .out32, .out64 (k, n, S)     the outputs of the fp32 and of the float64 run
  .grad64                      d sum(out * d_out) / d parameter of the float64 run, every parameter in state_dict order as
                               one flat vector, a parameter torch leaves without a gradient stored as zeros
  .grad_none                   the names of those parameters (tp_mrgcns.0.prelu.weight: never applied)
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
# (a case costs its 8-byte gradients and its configuration's weights: "et" 17 940 parameters, "e8" 19 000 -- left out)
CASES = [("et", 1), ("et", 2), ("et", 5), ("k1", 1), ("k1", 2), ("k1", 3), ("k1", 5), ("s16", 3)]
MAX_BYTES = 659126   # no larger than g32_dmrgcn_train.npz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    from tests import _graphtern_np as GN
    from tests import _graphtern_train_cases as CS
    from tests import _graphtern_train_np as TN
    sys.path.insert(0, args.ref)
    torch.Tensor.cuda = lambda self, *a, **k: self   # no GPU in the build container: the reference's normalizer stays on the CPU
    torch.nn.Module.cuda = lambda self, *a, **k: self
    from baseline.graphtern import TrajectoryPredictor, model_forward_pre_hook
    from baseline.graphtern import model as ref_model
    torch.set_num_threads(1)

    cases = [(f"{name}_n{n}", name, CS.scene(name, n)) for name, n in CASES]
    states = {name: CS.random_state(name) for name in dict(CASES)}
    rand_like = torch.rand_like
    adjacency = ref_model.generate_adjacency_matrix

    def fp32_distances(S, dtype):
        """the reference's own generate_adjacency_matrix on the fp32 S_obs; a float64 run gets the SAME fp32 distances (what
        the network's input is) with their inverses formed in float64, not the distances of a float64 subtraction"""
        A = adjacency(S.float())
        if dtype == torch.float32:
            return A
        dist = A[:, :2].double()
        inv = 1.0 / dist
        inv[dist == 0] = 0
        return torch.cat([dist, inv], dim=1)

    def reference(name, dtype):
        net = TrajectoryPredictor(**CS.module_kw(name))   # (the residuals are lambdas closing over the instance: built afresh)
        net.load_state_dict({q: torch.from_numpy(t) for q, t in states[name].items()}, strict=True)
        return net.to(dtype).train()

    def run(net, s_obs, d_out, draw):
        """one training-mode forward and backward with ``draw`` in rand_like's place -> (out, flat grads, the names without a
        gradient, PReLU inputs)"""
        seen, hooks = [], []
        for m in net.modules():
            if isinstance(m, torch.nn.PReLU):
                hooks.append(m.register_forward_hook(lambda mod, inp, out: seen.append(inp[0].detach().clone().numpy())))
        dtype = next(net.parameters()).dtype
        torch.rand_like = draw
        ref_model.generate_adjacency_matrix = lambda S: fp32_distances(S, dtype)
        try:
            out = net(s_obs.to(dtype))
        finally:
            torch.rand_like = rand_like
            ref_model.generate_adjacency_matrix = adjacency
        net.zero_grad()
        out.backward(torch.from_numpy(d_out).to(dtype))
        for h in hooks:
            h.remove()
        none = [q for q, p in net.named_parameters() if p.grad is None]
        flat = np.concatenate([(np.zeros(p.numel(), p.detach().numpy().dtype) if p.grad is None else p.grad.numpy().reshape(-1))
                               for p in net.parameters()])
        return out.detach().numpy()[0], flat, none, seen

    def attempt(seed):
        out, info = {}, {}
        for case, name, u in cases:
            sd = states[name]
            T, n = u.shape
            k = T - 2
            (s_obs,) = model_forward_pre_hook(torch.from_numpy(u[:k]), torch.from_numpy(u[k:]))   # (1, 2, T, n, 1)
            assert np.array_equal(s_obs.numpy(), GN.s_obs_of(u)), case
            d_out = CS.d_out(name, n)
            drawn = []

            def record(x):
                drawn.append(rand_like(x))
                return drawn[-1]

            net32, net64 = reference(name, torch.float32), reference(name, torch.float64)   # (their construction draws too)
            torch.manual_seed(seed)
            out32, grad32, none32, pre32 = run(net32, s_obs, d_out, record)
            assert len(drawn) == 1 and tuple(drawn[0].shape) == (1, 4, T, n, n), case
            keep = (~(drawn[0] > 0.8))[0].to(torch.uint8)
            import eigentrajectory_amd as ET
            mine = ET.GraphTERNLight(**CS.module_kw(name))
            torch.manual_seed(seed)
            mine = mine.draw_keep(n, "cpu")
            assert mine.dtype == torch.uint8 and torch.equal(mine, keep), f"{case}: draw_keep differs from the reference's draw"
            out64, grad64, none64, pre64 = run(net64, s_obs, d_out,
                                               lambda x: torch.where(keep[None] != 0, 0.0, 1.0).to(x.dtype))
            assert none32 == none64 == [TN.UNUSED], (case, none32, none64)
            if len(pre32) != len(pre64) or any(((p > 0) != (q > 0)).any() for p, q in zip(pre32, pre64)):
                return None, f"{case}: the fp32 and float64 runs branch differently at a PReLU"
            R = TN.run(sd, u, None, d_out[0], keep=keep.numpy())
            if R["decisions"]["prelu"]["undecided"]:
                return None, f"{case}: {R['decisions']['prelu']['undecided']} PReLU inputs inside their step bound"
            kept = R["kept"]
            mine_pre = [kept["yp"].val]
            for j in range(len(kept["c0"])):   # (tpcns' input is (1, k, 16, n); cpcns' (1, C_out, k, n))
                mine_pre += [kept["c0"][j].val, kept["c1"][j].val.transpose(1, 0, 2)]
            assert len(mine_pre) == len(pre64), case
            for p, q in zip(mine_pre, pre64):
                assert np.abs(p.reshape(-1) - q.reshape(-1)).max() <= F64 * max(np.abs(q).max(), 1e-300), case
            assert np.abs(R["out"].val - out64).max() <= F64 * np.abs(out64).max(), case
            at = 0
            for q, g in R["grads"].items():
                want = grad64[at:at + g.val.size].reshape(g.shape)
                tol = F64 * max(np.abs(want).max(), 1e-300) + (0.0 if g.tm is None else 2.0 ** -40 * float(np.max(g.tm)))
                assert np.abs(g.val - want).max() <= tol, (case, q)   # (tests/test_graphtern_train_cpu.py: _equal)
                at += g.val.size
            assert at == grad64.size
            out.update({f"{case}.config": np.array(name), f"{case}.u": u, f"{case}.d_out": d_out,
                        f"{case}.keep_bits": CS.pack_bits(keep.numpy()), f"{case}.out32": out32.astype(np.float32),
                        f"{case}.out64": out64, f"{case}.grad64": grad64, f"{case}.grad_none": np.array(none64)})
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
    path = os.path.join(args.out, "g35_graphtern_train.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= MAX_BYTES, os.path.getsize(path)
    manifest = {"g35_graphtern_train": {"cases": [c for c, _, _ in cases], "seed": int(seed), "numpy": np.__version__,
                                        "torch": torch.__version__, "bytes": os.path.getsize(path), "per_case": info}}
    with open(os.path.join(args.out, "MANIFEST_g35_graphtern_train.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")
    print(f"wrote {path}: {os.path.getsize(path)} bytes, seed {seed}")


if __name__ == "__main__":
    main()
