#!/usr/bin/env python3
"""G28: ET-Implicit training fixture -- the parameter gradients of the reference's SocialImplicitLight in TRAINING mode, run
on the CPU in the build container under G25's weights (tests/golden/g25_implicit.npz: ``net.*`` for the ET configuration,
``gen.*`` for S = 12, T = 10, T_out = 5, three bins) on G25's own inputs, which are referred to by key and not stored again.

    python tools/make_golden_implicit_train.py --ref <reference checkout> --out tests/golden

As in tools/make_golden_implicit.py, ``Tensor.cuda`` / ``Module.cuda`` are the identity for the duration of the script.  Per
case (``pick<i>``, ``single``, ``edges``, ``lonely``, ``nan`` under ``net``; ``gen0``, ``gen1`` = ``gen.v0``, ``gen.v1`` under
``gen``) a seeded fp32 G of the output's shape, then ``(net(v) * G).sum().backward()``:
  <case>.v_key        the key of its input v (1, 1, T, N) in g25_implicit.npz
  <case>.G            (1, S, T_out, N) float32
  <case>.visited      (n_bins,) bool: the cells whose parameters got a gradient (.grad is not None) -- the zones with a member
  <case>.grads32      (n_bins, 19-tensor block) float32: every parameter's gradient of the fp32 run, per cell in the order
                      of tests/_implicit_train_np.py's KINDS followed by noise_w (zeros where .grad is None)
  <case>.grads64      the same of a float64 run: module, v and the bins tensor cast to double (the fp32 bin values are exact
                      in double, so no zone moves), default dtype float64 so that the output buffer is double too
  <case>.nan_differs  (n_bins, block) bool: where the NaN pattern of the float64 gradients and of the restatement differ
                      (all False unless the script printed otherwise)
The script asserts what the tests rely on: the training-mode output equals the eval-mode output bit for bit; no cell but the
visited ones has a gradient; every noise_w gradient is an exact zero; the float64 restatement
(tests/_implicit_train_np.py) reproduces the float64 gradients within its own float64 bound (its fp32 bound scaled by
2^-27: two float64 evaluations, each within 2^-29 of that bound of the exact value, any order of summation); no ReLU of
any case is undecided; the NaN pattern of the ``nan`` case agrees.  The manifest entry (cases, versions, the ratios
above) goes to MANIFEST_g28_implicit_train.json next to the fixture; MANIFEST.json is not touched.  Only data is written;
nothing of the reference is copied."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

BINS = (0.0, 0.01, 0.1, 1.2)
NOISE_WEIGHT = (0.05, 1, 4, 8)
GEN = dict(spatial_input=1, spatial_output=12, temporal_input=10, temporal_output=5, bins=[0, 0.5, 2],
           noise_weight=[0.05, 1, 4])
F64_SCALE = 2.0 ** -27


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="a checkout of the reference implementation")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    args.out = os.path.abspath(args.out)
    from tests import _golden as G
    from tests import _implicit_train_np as TN
    sys.path.insert(0, args.ref)
    os.chdir(args.ref)
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    from baseline.implicit import TrajectoryPredictor

    torch.set_num_threads(1)
    Z = G.load("g25_implicit.npz")
    picks = sorted({k.split(".")[0] for k in Z.files if k.startswith("pick")}, key=lambda t: int(t[4:]))
    cases = [(t, f"{t}.v", "net.") for t in picks + ["single", "edges", "lonely", "nan"]]
    cases += [(f"gen{i}", f"gen.v{i}", "gen.") for i in range(2)]
    rng = np.random.default_rng(28)
    out, worst, undecided = {}, {}, 0
    order = TN.KINDS + ["noise_w"]

    def build(prefix, double):
        kw = dict(spatial_input=1, spatial_output=20, temporal_input=8, temporal_output=6, bins=list(BINS),
                  noise_weight=list(NOISE_WEIGHT)) if prefix == "net." else GEN
        sd = {k[len(prefix):]: torch.from_numpy(np.array(Z[k])) for k in Z.files if k.startswith(prefix + "implicit_cells.")}
        if double:
            torch.set_default_dtype(torch.float64)
        try:
            net = TrajectoryPredictor(**kw)
        finally:
            torch.set_default_dtype(torch.float32)
        net.load_state_dict(sd, strict=True)
        if double:
            fp32_bins = net.bins.float().clone()
            net = net.double()
            net.bins = fp32_bins.double()  # the fp32 bin values, exact in double
        return net, {k: v.numpy() for k, v in sd.items()}

    def grads_of(net, v, Gt, double):
        net.zero_grad(set_to_none=True)
        net.train()
        if double:
            torch.set_default_dtype(torch.float64)
        try:
            res = net(v)
            (res * Gt).sum().backward()
        finally:
            torch.set_default_dtype(torch.float32)
        named = dict(net.named_parameters())
        n_bins = len(net.implicit_cells)
        visited = np.asarray([named[f"implicit_cells.{i}.global_w"].grad is not None for i in range(n_bins)])
        rows = []
        for i in range(n_bins):
            got = [named[f"implicit_cells.{i}.{kind}"] for kind in order]
            assert all((p.grad is not None) == bool(visited[i]) for p in got), "a cell has some gradients only"
            rows.append(np.concatenate([(p.grad if p.grad is not None else torch.zeros_like(p)).numpy().ravel() for p in got]))
        return res.detach(), visited, np.stack(rows)

    for tag, v_key, prefix in cases:
        v = torch.from_numpy(np.array(Z[v_key]))
        net, sd = build(prefix, False)
        net64, _ = build(prefix, True)
        with torch.no_grad():
            ev = net.eval()(v)
        S, To, n = ev.shape[1:]
        Gn = rng.normal(0, 1, (1, S, To, n)).astype(np.float32)
        res, visited, g32 = grads_of(net, v, torch.from_numpy(Gn), False)
        assert res.dtype == torch.float32 and np.array_equal(res.numpy(), ev.numpy(), equal_nan=True), tag
        res64, visited64, g64 = grads_of(net64, v.double(), torch.from_numpy(Gn).double(), True)
        assert res64.dtype == torch.float64 and g64.dtype == np.float64 and np.array_equal(visited, visited64), tag
        bins = BINS if prefix == "net." else GEN["bins"]
        r = TN.run(sd, v[0, 0].numpy(), Gn[0], bins)
        assert np.array_equal(r["visited"], visited), (tag, r["visited"], visited)
        assert np.array_equal(visited, np.bincount(r["zone"][r["zone"] >= 0], minlength=len(bins)) > 0), tag
        assert r["undecided"] == 0, (tag, r["undecided"])
        undecided += r["undecided"]
        assert (g32[:, -1] == 0).all() and (g64[:, -1] == 0).all(), (tag, "noise_w")  # a sum of products with the zero noise
        want, bound = TN.block(sd, r["grads"], len(bins)), TN.block(sd, r["grads_err"], len(bins)) * F64_SCALE
        ok, ratio, same_nan = TN.compare(g64[:, :-1], want, bound)
        nan_differs = np.isnan(g64[:, :-1]) != (np.isnan(want) | np.isnan(bound))
        if not same_nan:
            print(f"{tag}: the NaN pattern of the reference and of the restatement differ at {int(nan_differs.sum())} elements, "
                  f"columns {np.flatnonzero(nan_differs.any(axis=0)).tolist()[:40]}")
        assert ok, (tag, ratio, same_nan)
        assert np.array_equal(np.isnan(g32), np.isnan(g64)), tag
        ok32, ratio32, _ = TN.compare(g32[:, :-1], want, bound / F64_SCALE)
        worst[tag] = (ratio, ratio32)
        print(f"{tag}: N {n}, visited {visited.astype(int).tolist()}, NaN gradients {int(np.isnan(g64).sum())}, restatement "
              f"against float64 autograd {ratio:.3f} of its float64 bound, torch's fp32 run {ratio32:.3f} of the fp32 bound",
              flush=True)
        out[f"{tag}.v_key"] = np.asarray(v_key)
        out[f"{tag}.G"] = Gn
        out[f"{tag}.visited"] = visited
        out[f"{tag}.grads32"], out[f"{tag}.grads64"] = g32.astype(np.float32), g64
        out[f"{tag}.nan_differs"] = nan_differs
    nan = out["nan.grads64"]
    assert np.isnan(nan).any() and not np.isnan(nan).all() and not np.isnan(nan[~out["nan.visited"]]).any()
    path = os.path.join(args.out, "g28_implicit_train.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path))
    assert os.path.getsize(path) < 1000 * 1000
    # the fixture's manifest entry is a file of its own: MANIFEST.json belongs to the fixtures it was written with
    entry = {"cases": [c[0] for c in cases], "numpy": np.__version__, "torch": torch.__version__,
             "undecided_relus": undecided,
             "restatement_over_float64_bound": {t: repr(w[0]) for t, w in worst.items()},
             "torch_fp32_over_fp32_bound": {t: repr(w[1]) for t, w in worst.items()}}
    with open(os.path.join(args.out, "MANIFEST_g28_implicit_train.json"), "w") as f:
        json.dump({"g28_implicit_train": entry}, f, indent=1, sort_keys=True)

if __name__ == "__main__":
    main()
