"""The curve-fitting baselines (CurveModel/curve_fitting.py) as one batched HIP launch per pass (csrc/et_curve.hip):
bit for bit against the numpy restatement (tests/_curve_fit_np.py) in recon, control points, per-step loss and best
step; batch against single calls; the six full-length eth fits against the reference (tests/golden/g17) within the
reference's own spread; argument checks; the script's --curves table."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from . import _golden as G
from ._curve_fit_np import curve_fit_np
from ._gpu_common import *  # noqa: F401,F403 -- fixtures (dev, ops) and helpers

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = G.load("g17_curve_fit.npz")


def _walks(n, T, seed):
    """Normalised-looking random walks; row 0 returns to its start (traj[0] == traj[-1])."""
    rng = np.random.default_rng(seed)
    tr = np.cumsum(rng.normal(0, 0.4, (n, T, 2)), axis=1).astype(np.float32)
    tr -= tr[:, -1:]
    tr[0, -1] = tr[0, 0]
    return tr


def _assert_bit_equal(dev, trajs, bases, steps):
    from eigentrajectory_amd import ops
    res = ops.curve_fit_batch([torch.from_numpy(t).to(dev) for t in trajs], [b.to(dev) for b in bases], steps=steps,
                              want_cp=True, want_loss=True)
    loss, best = res["loss"].cpu().numpy(), res["best"].cpu().numpy()
    for f, (t, b) in enumerate(zip(trajs, bases)):
        ref = curve_fit_np(t, b.numpy(), steps)
        what = (f, t.shape, tuple(b.shape), steps)
        assert best[f] == ref["best"], what
        assert np.array_equal(loss[f], ref["loss"]), what
        assert np.array_equal(res["recon"][f].cpu().numpy(), ref["recon"]), what
        assert np.array_equal(res["cp"][f].cpu().numpy(), ref["cp"]), what


@pytest.mark.parametrize("steps", [1, 2, 7, 500])
def test_table_batch_bit_equal_to_restatement(dev, steps):
    """All 28 fits of eth's table (14 bases x obs / pred) in one call."""
    from eigentrajectory_amd import curve
    trajs, bases = [], []
    for part in ("obs", "pred"):
        for _, _, b in curve.table_bases(Z[f"in.{part}"].shape[1]):
            trajs.append(Z[f"in.{part}"])
            bases.append(b)
    _assert_bit_equal(dev, trajs, bases, steps)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 181])
def test_shapes_bit_equal_to_restatement(dev, n):
    """ncp 2..6 at T = 3 / 8 / 12 (exact and generic kernels), ncp 7 / 8 at T = 20, a closed trajectory in row 0."""
    from eigentrajectory_amd import curve
    trajs, bases = [], []
    for T in (3, 8, 12):
        for ncp in range(2, 7):
            trajs.append(_walks(n, T, 100 * T + ncp))
            bases.append(curve.bezier_basis(ncp - 1, T) if ncp > 2 else curve.linear_basis(T))
    for ncp in (7, 8):
        trajs.append(_walks(n, 20, ncp))
        bases.append(curve.bspline_basis(ncp - 1, 3, 20))
    _assert_bit_equal(dev, trajs, bases, 300)


def test_long_run_bit_equal_to_restatement(dev):
    from eigentrajectory_amd import curve
    _assert_bit_equal(dev, [_walks(2253, 12, 1), _walks(2253, 8, 2)],
                      [curve.bezier_basis(3, 12), curve.bspline_basis(3, 2, 8)], 3000)


def test_batch_equals_single_calls(dev):
    from eigentrajectory_amd import curve
    trajs, bases = [], []
    for part in ("obs", "pred"):
        t = torch.from_numpy(Z[f"in.{part}"]).to(dev)
        for _, _, b in curve.table_bases(t.shape[1]):
            trajs.append(t)
            bases.append(b)
    recons, best, loss = curve.curve_fitting_batch(trajs, bases, steps=200, want_loss=True)
    for f, (t, b) in enumerate(zip(trajs, bases)):
        r1, b1, l1 = curve.curve_fitting_batch([t], [b], steps=200, want_loss=True)
        assert torch.equal(r1[0], recons[f]) and int(b1[0]) == int(best[f]) and torch.equal(l1[0], loss[f]), f
        if f == 0:
            assert torch.equal(curve.curve_fitting(t, b, steps=200), recons[f])


def test_full_length_eth_fits_against_the_reference(dev):
    """The six 100 000-step fits of g17 (c): each Table-1 entry within max(3 x the reference's own spread under a 1-ulp
    perturbation of the input, 1e-3), and the best loss no worse than the reference's by more than that."""
    from eigentrajectory_amd import curve
    ori, rot = torch.from_numpy(Z["in.ori"]), torch.from_numpy(Z["in.rot"])
    obs, pred, _ = G.dataset("eth", "test")
    truth = {"obs": torch.from_numpy(obs), "pred": torch.from_numpy(pred)}
    specs = [("linear", "obs"), ("bezier3", "obs"), ("bspline_c3_d2", "obs"),
             ("linear", "pred"), ("bezier3", "pred"), ("bspline_c3_d2", "pred")]
    make = {"linear": curve.linear_basis, "bezier3": lambda T: curve.bezier_basis(3, T),
            "bspline_c3_d2": lambda T: curve.bspline_basis(3, 2, T)}
    trajs = [torch.from_numpy(Z[f"in.{part}"]).to(dev) for _, part in specs]
    recons, best, _ = curve.curve_fitting_batch(trajs, [make[nm](t.shape[1]) for (nm, _), t in zip(specs, trajs)],
                                                steps=100000)
    for (nm, part), rec, tr in zip(specs, recons, trajs):
        rec = rec.cpu()
        err = (rec @ rot.transpose(-1, -2) + ori - truth[part]).norm(p=2, dim=-1).mean().item()
        loss = (rec - tr.cpu()).norm(p=2, dim=-1).mean().item()
        e0, e1 = float(Z[f"c_err.o.{part}.{nm}"]), float(Z[f"c_err.p.{part}.{nm}"])
        tol = max(3 * abs(e0 - e1), 1e-3)
        assert abs(err - e0) <= tol, (nm, part, err, e0, tol)
        assert loss <= float(Z[f"c_loss.o.{part}.{nm}"]) + tol, (nm, part, loss)


def test_bad_arguments_return_a_status(dev):
    from eigentrajectory_amd import curve, ops
    t = torch.zeros((4, 8, 2), device=dev)
    with pytest.raises(ValueError):
        ops.curve_fit_batch([t], [curve.bezier_basis(3, 12)], steps=10)       # T mismatch
    with pytest.raises(ValueError):
        ops.curve_fit_batch([t], [torch.zeros((8, 9))], steps=10)             # ncp 9
    with pytest.raises(ValueError):
        ops.curve_fit_batch([torch.zeros((4, 33, 2), device=dev)], [torch.zeros((33, 3))], steps=10)
    with pytest.raises(ValueError):
        ops.curve_fit_batch([t], [curve.bezier_basis(3, 8)], steps=0)
    with pytest.raises(ValueError):
        ops.curve_fit_batch([t], [curve.bezier_basis(3, 8)], steps=10, lr=0.0)
    torch.cuda.synchronize()
    r = ops.curve_fit_batch([t], [curve.bezier_basis(3, 8)], steps=5)  # the device is still usable
    assert torch.isfinite(r["recon"][0]).all()


def _run_script(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "descriptor_evaluation.py"), *args],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    return out.stdout


def test_script_curves_table(dev):
    plain = _run_script()
    curves = _run_script("--curves", "--steps", "200")
    svd_lines = [ln for ln in curves.splitlines() if ln.startswith("k: ") or "Singular" in ln]
    assert "\n".join(svd_lines) == plain.strip()
    for head in ("===Linear===", "===Bezier Curve===", "===B-Spline==="):
        assert curves.count(head) == 5
    assert curves.count("obs error:") == 5 * (14 + 12)
