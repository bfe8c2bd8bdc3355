#!/usr/bin/env python3
"""G17: the reference's curve-fitting baselines (CurveModel/, script/descriptor_evaluation.py:38-85), on the CPU.

    python tools/make_golden_curves.py --ref /path/to/reference --out tests/golden [--jobs 4 --threads 4]

(a) bases: the reference's 14 bases (Linear, Bezier degree 2..5, B-spline degree 1..3 x n_curve 2..5 with n_curve >
    degree) at T = 3, 5, 8, 12, 20.  Key `a.T{T}.{name}`, (T, ncp) fp32.
(b) short fits: the reference's curve_fitting on eth test, TrajNorm(ori, rot, sca=False) computed on obs and applied to
    obs and pred, every basis, with the 100 000-step loop cut to 1 and to 10 steps (the module's `range` is rebound for
    that one loop; `range(1, n_cp)` is untouched).  Key `b.s{steps}.{part}.{name}`, (N, T, 2) fp32.
(c) long fits: the full 100 000 steps on eth test for Linear, Bezier 3 and B-spline (n_curve 3, degree 2), each on obs
    and pred, once on the input and once on the input perturbed by +-1e-7 (seeded signs).  `c.o.{part}.{name}` holds
    recon_best of the unperturbed run, `c_err.{o,p}.*` the Table-1 entry ((denormalize(recon) - traj).norm(-1).mean()),
    `c_loss.{o,p}.*` the loss of recon_best in the normalised frame.  The two runs differ by the reference's own spread.
    Each long fit runs in a child process (about 1 min at 2 threads); finished fits are cached in --cache.

Also stored: the normalised inputs (`in.obs`, `in.pred`, `in.obs_p`, `in.pred_p`) and the normaliser (`in.ori`,
`in.rot`).  Only data is written; nothing of the reference is copied."""
import argparse
import builtins
import contextlib
import io
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

from tests import _golden as G  # noqa: E402

TS = (3, 5, 8, 12, 20)
LONG = [("linear", "obs"), ("bezier3", "obs"), ("bspline_c3_d2", "obs"),
        ("linear", "pred"), ("bezier3", "pred"), ("bspline_c3_d2", "pred")]


def basis_names():
    names = [("linear", None)] + [(f"bezier{d}", ("bezier", d)) for d in range(2, 6)]
    names += [(f"bspline_c{c}_d{d}", ("bspline", c, d)) for d in range(1, 4) for c in range(2, 6) if c > d]
    return names


def ref_basis(CM, name, T):
    if name == "linear":
        return torch.stack([torch.linspace(0, 1, T), torch.linspace(1, 0, T)], dim=1)
    spec = dict(basis_names())[name]
    if spec[0] == "bezier":
        return CM.bezier_basis(degree=spec[1], step=T)
    return CM.bspline_basis(cpoint=spec[1], degree=spec[2], step=T)


def inputs(ref):
    from EigenTrajectory import TrajNorm
    obs, pred, _ = G.dataset("eth", "test")
    obs_t, pred_t = torch.from_numpy(obs), torch.from_numpy(pred)
    tn = TrajNorm(ori=True, rot=True, sca=False)
    tn.calculate_params(obs_t)
    on, pn = tn.normalize(obs_t), tn.normalize(pred_t)
    rng = np.random.default_rng(17)
    op = on + torch.from_numpy(rng.choice([-1e-7, 1e-7], size=on.shape).astype(np.float32))
    pp = pn + torch.from_numpy(rng.choice([-1e-7, 1e-7], size=pn.shape).astype(np.float32))
    return tn, obs_t, pred_t, {"obs": on, "pred": pn, "obs_p": op, "pred_p": pp}


def fit(CM, traj, basis, steps):
    mod = sys.modules["CurveModel.curve_fitting"]

    def short_range(*a):
        return builtins.range(steps) if a == (100000,) else builtins.range(*a)

    mod.range = short_range
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            return mod.curve_fitting(traj, basis)
    finally:
        del mod.range


def long_child(args):
    sys.path.insert(0, args.ref)
    os.chdir(args.ref)
    torch.set_num_threads(args.threads)
    import CurveModel as CM
    k = args.long
    name, part = LONG[k % 6]
    pert = k // 6
    _, _, _, x = inputs(args.ref)
    traj = x[part + ("_p" if pert else "")]
    t0 = time.time()
    rec = fit(CM, traj, ref_basis(CM, name, traj.shape[1]), 100000)
    np.save(os.path.join(args.cache, f"long_{k}.npy"), rec.numpy())
    print(f"long fit {k} ({name}, {part}, pert {pert}) done in {time.time() - t0:.0f} s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    ap.add_argument("--cache", default=os.path.join(tempfile.gettempdir(), "g17_cache"))
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--threads", type=int, default=4)
    ap.add_argument("--long", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.out, args.cache = os.path.abspath(args.out), os.path.abspath(args.cache)
    os.makedirs(args.cache, exist_ok=True)
    if args.long is not None:
        return long_child(args)

    todo = [k for k in range(12) if not os.path.exists(os.path.join(args.cache, f"long_{k}.npy"))]
    procs, pending = [], list(todo)
    while pending and len(procs) < args.jobs:
        k = pending.pop(0)
        procs.append((k, subprocess.Popen([sys.executable, os.path.abspath(__file__), "--ref", args.ref, "--cache",
                                           args.cache, "--threads", str(args.threads), "--long", str(k)])))

    sys.path.insert(0, args.ref)
    os.chdir(args.ref)
    torch.set_num_threads(args.threads)
    import CurveModel as CM
    tn, obs_t, pred_t, x = inputs(args.ref)
    out = {"in." + k: v.numpy() for k, v in x.items()}
    out["in.ori"], out["in.rot"] = tn.traj_ori.numpy(), tn.traj_rot.numpy()

    for T in TS:                                                          # (a)
        for name, _ in basis_names():
            out[f"a.T{T}.{name}"] = ref_basis(CM, name, T).numpy().astype(np.float32)
    t0 = time.time()
    for steps in (1, 10):                                                 # (b)
        for part in ("obs", "pred"):
            for name, _ in basis_names():
                out[f"b.s{steps}.{part}.{name}"] = fit(CM, x[part], ref_basis(CM, name, x[part].shape[1]), steps).numpy()
    print(f"(a), (b) done ({time.time() - t0:.0f} s)", flush=True)

    while procs or pending:                                               # (c)
        k, p = procs.pop(0)
        if p.wait() != 0:
            raise SystemExit(f"long fit {k} failed")
        if pending:
            j = pending.pop(0)
            procs.append((j, subprocess.Popen([sys.executable, os.path.abspath(__file__), "--ref", args.ref, "--cache",
                                               args.cache, "--threads", str(args.threads), "--long", str(j)])))
    truth = {"obs": obs_t, "pred": pred_t}
    for k in range(12):
        name, part = LONG[k % 6]
        pert = "p" if k // 6 else "o"
        rec = torch.from_numpy(np.load(os.path.join(args.cache, f"long_{k}.npy")))
        traj = x[part + ("_p" if k // 6 else "")]
        if pert == "o":  # the perturbed runs only contribute their table entry and loss
            out[f"c.{pert}.{part}.{name}"] = rec.numpy()
        out[f"c_err.{pert}.{part}.{name}"] = np.float64((tn.denormalize(rec) - truth[part]).norm(p=2, dim=-1).mean().item())
        out[f"c_loss.{pert}.{part}.{name}"] = np.float64((rec - traj).norm(p=2, dim=-1).mean().item())
    for name, part in LONG:
        e0, e1 = out[f"c_err.o.{part}.{name}"], out[f"c_err.p.{part}.{name}"]
        print(f"(c) {part} {name}: error {e0:.5f} / perturbed {e1:.5f}, spread {abs(e0 - e1):.2e}")
    path = os.path.join(args.out, "g17_curve_fit.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
