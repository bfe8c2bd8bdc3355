"""The reference's TCC / COL test metrics (utils/metrics.py:30-155) as the scene-batched HIP kernel
(csrc/et_metrics.hip): tensor form against the numpy restatement (tests/_traj_metrics_np.py), fused form against the
tensor form of the reconstruction's output, whole-split replay against the reference (tests/golden/g16), and the
trainer / wrapper entry points."""
import numpy as np
import pytest
import torch

from . import _golden as G
from . import _traj_metrics_np as R
from ._gpu_common import *  # noqa: F401,F403 -- fixtures (dev, ops) and helpers
from ._gpu_common import _trainer_for

pytestmark = pytest.mark.gpu
Z16 = G.load("g16_tcc_col.npz")


def _compare_to_restatement(got, ref, pred, per_sample_bits=None, tcc_atol=1e-6):
    """COL / TCC / best / ADE / FDE of the kernel against the restatement on the same data."""
    near = np.abs(ref["min_dist"] - np.float32(0.2)) <= 1e-6      # (S,N): samples on the threshold
    ok_rows = ~near.any(axis=0)
    assert not near.any(), f"samples within 1e-6 of the threshold: {np.argwhere(near).tolist()}"
    if per_sample_bits is not None:
        assert np.array_equal(per_sample_bits[~near], ref["col_bits"][~near])
    assert np.array_equal(N_(got["COL"])[ok_rows], ref["COL"][ok_rows])
    tcc = N_(got["TCC"])
    np.testing.assert_allclose(tcc, ref["TCC"], rtol=0, atol=tcc_atol)
    assert np.all(tcc[ref["TCC"] == 0] == 0)
    best = N_(got["best"])
    diff = np.nonzero(best != ref["best"])[0]  # allowed only on exact ties of the final error
    for i in diff:
        a, b = pred[best[i], i, -1], pred[ref["best"][i], i, -1]
        assert np.array_equal(a, b), (i, best[i], ref["best"][i])


@pytest.mark.parametrize("S,T,sizes", [
    (1, 12, [1, 2, 57, 300]), (20, 12, [1, 2, 57, 300]), (20, 3, [2, 57, 1, 300]), (1, 3, [300, 57]),
    (20, 12, [3000]), (20, 12, [57] * 40 + [2] * 90 + [1] * 7),
])
def test_tensor_form_matches_restatement(dev, ops, S, T, sizes):
    from eigentrajectory_amd import utils
    rng = np.random.default_rng(S * 1000 + T + len(sizes))
    n = sum(sizes)
    gt = np.cumsum(rng.normal(0, 0.3, (n, T, 2)), axis=1).astype(np.float32) + rng.uniform(-3, 3, (n, 1, 2)).astype(np.float32)
    pred = (gt[None] + rng.normal(0, 0.3, (S, n, T, 2))).astype(np.float32)
    got = ops.traj_metrics(T_(pred, dev), T_(gt, dev), scene_sizes=sizes)
    ref = R.metrics(pred, gt, sizes)
    bits = None
    if S > 1 and n <= 500:  # per-(sample, pedestrian) bits: the kernel on one sample at a time
        bits = np.stack([N_(ops.traj_metrics(T_(pred[s:s + 1], dev), T_(gt, dev), sizes, metrics=("COL",))["COL"]) > 0
                         for s in range(S)])
    _compare_to_restatement(got, ref, pred, bits)
    np.testing.assert_allclose(N_(got["ADE"]), N_(utils.compute_batch_ade(T_(pred, dev), T_(gt, dev))), rtol=1e-6, atol=0)
    np.testing.assert_allclose(N_(got["FDE"]), N_(utils.compute_batch_fde(T_(pred, dev), T_(gt, dev))), rtol=1e-6, atol=0)
    # the reference's entry points (4-D gt accepted, return order ADE, FDE, COL, TCC)
    a, f, c, t = utils.compute_batch_metric(T_(pred, dev), T_(gt[None], dev), scene_sizes=sizes)
    for x, key in ((a, "ADE"), (f, "FDE"), (c, "COL"), (t, "TCC")):
        assert torch.equal(x, got[key])
    assert torch.equal(utils.compute_batch_tcc(T_(pred, dev), T_(gt, dev)), got["TCC"])
    assert torch.equal(utils.compute_batch_col(T_(pred, dev), T_(gt, dev), scene_sizes=sizes), got["COL"])


@pytest.mark.parametrize("case", [str(c) for c in Z16["cases"]])
def test_tensor_form_matches_reference_g16a(dev, ops, case):
    """G16 (a), one scene per case: COL bits per (sample, pedestrian), TCC (exact 0 where the reference has 0; NaN rows and
    motionless rows as in the reference), best sample, ADE / FDE."""
    pred, gt = Z16[f"a.{case}.pred"], Z16[f"a.{case}.gt"]
    got = ops.traj_metrics(T_(pred, dev), T_(gt, dev))
    bits = np.stack([N_(ops.traj_metrics(T_(pred[s:s + 1], dev), T_(gt, dev), metrics=("COL",))["COL"]) > 0
                     for s in range(pred.shape[0])])
    assert np.array_equal(bits, Z16[f"a.{case}.col_bits"].astype(bool))
    assert np.array_equal(N_(got["COL"]), Z16[f"a.{case}.col"])
    noise, ref_tcc = Z16[f"a.{case}.noise"], Z16[f"a.{case}.tcc"]
    tcc = N_(got["TCC"])
    np.testing.assert_allclose(tcc[~noise], ref_tcc[~noise], rtol=0, atol=1e-6)
    assert np.all(tcc[ref_tcc == 0] == 0)
    assert np.array_equal(N_(got["best"]), Z16[f"a.{case}.best"])
    np.testing.assert_allclose(N_(got["ADE"]), Z16[f"a.{case}.ade"], rtol=1e-6, atol=0)
    np.testing.assert_allclose(N_(got["FDE"]), Z16[f"a.{case}.fde"], rtol=1e-6, atol=0)
    assert np.array_equal(np.isnan(N_(got["FDE"])), np.isnan(Z16[f"a.{case}.fde"]))


def _descriptor_setup(rng, n, S, k, T_pred, mode, dev, ops):
    from eigentrajectory_amd.synth import synthetic_trajectories_np
    obs, pred = synthetic_trajectories_np(n, seed=int(rng.integers(1 << 30)))
    obs, pred = obs[:, -8:], pred[:, :T_pred]
    U = [torch.from_numpy(np.linalg.qr(rng.normal(size=(2 * t, k)))[0].astype(np.float32)).to(dev)
         for t in (8, T_pred, 8, T_pred)]
    A = [torch.from_numpy(rng.normal(0, 0.5, (k, S)).astype(np.float32)).to(dev) for _ in range(2)]
    C = torch.from_numpy(rng.normal(0, 0.5, (k, n, S)).astype(np.float32)).to(dev)
    o, p = T_(obs, dev), T_(pred, dev)
    _, _, nrm, _, pose = ops.norm_project(o, None, U[0], None, U[2], None, mode, 0.3, want_pose=True)
    return o, p, U, A, C, nrm, pose


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("form", ["nrm", "pose"])
def test_fused_form_matches_tensor_form(dev, ops, mode, form):
    """The fused form reconstructs every sample with anchor_reconstruct's arithmetic: COL and best bit-equal to the tensor
    form on ops.anchor_reconstruct's output, TCC within 1e-6; ADE / FDE within 1e-6 relative of the existing fused
    ADE / FDE epilogue.  (pose: the rotation is recovered as (c sca) / sca -- within an ulp or two for moving rows, so the
    comparison there is the restatement's, with threshold and tie exemptions.)"""
    rng = np.random.default_rng(7 + mode)
    sizes = [1, 2, 57, 300, 26, 26, 40]
    n, S, k = sum(sizes), 20, 6
    for T_pred, kk in ((12, k), (12, 10), (5, 3)):
        o, p, U, A, C, nrm, pose = _descriptor_setup(rng, n, S, kk, T_pred, mode, dev, ops)
        rec = ops.anchor_reconstruct(C, A[0], A[1], U[1], U[3], mode, 0.3, nrm=nrm)
        ref = ops.traj_metrics(rec, p, sizes)
        kw = dict(nrm=nrm) if form == "nrm" else dict(pose=pose)
        got = ops.anchor_reconstruct_metrics_scenes(C, p, A[0], A[1], U[1], U[3], mode, 0.3, scene_sizes=sizes, **kw)
        exact = form == "nrm" or mode in (0, 3)  # static / identity rows: pose carries c and s exactly
        if exact:
            assert torch.equal(got["COL"], ref["COL"]) and torch.equal(got["best"], ref["best"])
            np.testing.assert_allclose(N_(got["TCC"]), N_(ref["TCC"]), rtol=0, atol=1e-6)
        else:
            # (an ulp in the rotation moves a 5-step correlation by up to ~1e-6)
            _compare_to_restatement(got, R.metrics(N_(rec), N_(p), sizes), N_(rec), tcc_atol=1e-5)
        a0, f0 = ops.anchor_reconstruct_metrics(C, p, A[0], A[1], U[1], U[3], mode, 0.3, nrm=nrm)
        # (the existing epilogue: within 1e-6 relative to the largest, utils' matrix-core form)
        np.testing.assert_allclose(N_(got["ADE"]), N_(a0), rtol=1e-6, atol=1e-6 * float(a0.abs().max()))
        np.testing.assert_allclose(N_(got["FDE"]), N_(f0), rtol=1e-6, atol=1e-6 * float(f0.abs().max()))


@pytest.mark.parametrize("scene", G.SCENES)
def test_whole_split_replay_g16b(dev, ops, scene):
    """G14's network outputs replayed through this build's wrapper (scene by scene, evaluate_metrics: the reference's test
    loop) and, for the whole split in ONE launch, the tensor form on the concatenated recon_traj with the split's scene
    sizes -- against the reference's compute_batch_tcc / compute_batch_col (tests/golden/g16 (b))."""
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    from .test_bridges import ReplaySGCN
    z = G.load("g14_sgcn_full_splits.npz")
    g2 = G.load("g2_fit_all_scenes.npz")
    obs, pred, sse = G.dataset(scene, "test")
    net = ReplaySGCN(None, None, None, 2e-5)
    model = EigenTrajectory(net, get_hook_func("sgcn"), default_hyper_params(static_dist=float(z[f"{scene}.static_dist"])))
    sd = model.state_dict()
    for key in list(sd):
        if key.startswith("ET_"):
            sd[key] = torch.from_numpy(g2[f"{scene}.{key}"])
    model.load_state_dict(sd)
    model = model.to(dev).eval()
    v_all, out_all = torch.from_numpy(z[f"{scene}.v"]), torch.from_numpy(z[f"{scene}.net_out"]).to(dev)
    sizes = [int(v) for v in z[f"{scene}.scene_size"]]
    per_scene, recs, gts, at = [], [], [], 0
    with torch.no_grad():
        for i, n in zip(z[f"{scene}.scene_index"], sizes):
            s, e = sse[int(i)]
            net.expect = v_all[:, at:at + n].reshape(1, -1, n, 1)
            net.eye_shapes = np.asarray([[1, n, n], [n, 1, 1]])
            net.answer = out_all[:, at:at + n].contiguous()
            o, p = T_(obs[s:e], dev), T_(pred[s:e], dev)
            per_scene.append(model.evaluate_metrics(o, p))
            recs.append(model(o)["recon_traj"])
            gts.append(p)
            at += n
    split = ops.traj_metrics(torch.cat(recs, dim=1), torch.cat(gts, dim=0), scene_sizes=sizes)
    fused = {key: torch.cat([m[key] for m in per_scene]) for key in ("ADE", "FDE", "TCC", "COL")}
    ref_tcc, ref_col, noise = Z16[f"b.{scene}.tcc"], Z16[f"b.{scene}.col"], Z16[f"b.{scene}.noise"]
    mind = Z16[f"b.{scene}.min_dist"]
    S = mind.shape[0]
    near = np.abs(mind - np.float32(0.2)) <= 1e-4
    col_ok = ~near.any(axis=0)
    n_tot = len(ref_tcc)
    # how far the exempt rows can move the split means: each near sample 100 / S of its row's COL, each noise row 2 of TCC
    col_bound = near.sum() * 100.0 / S / n_tot + 1e-6
    tcc_bound = 2.0 * noise.sum() / n_tot + 1e-4
    for got in (split, fused):
        tcc, col = N_(got["TCC"]), N_(got["COL"])
        assert np.array_equal(col[col_ok], ref_col[col_ok]), np.nonzero(col[col_ok] != ref_col[col_ok])
        np.testing.assert_allclose(tcc[~noise], ref_tcc[~noise], rtol=0, atol=1e-4)
        assert abs(col.mean(dtype=np.float64) - Z16[f"b.{scene}.tcc_col_mean"][1]) <= col_bound
        assert abs(tcc.mean(dtype=np.float64) - Z16[f"b.{scene}.tcc_col_mean"][0]) <= tcc_bound
        np.testing.assert_allclose(N_(got["ADE"]), z[f"{scene}.ade"], rtol=0, atol=1e-5)
        np.testing.assert_allclose(N_(got["FDE"]), z[f"{scene}.fde"], rtol=0, atol=1e-5)


def test_trainer_test_all_metrics(dev):
    """ETTrainer.test(metrics="all"): the reference's four keys, each the pedestrian mean of evaluate_metrics; the default
    call still returns exactly ADE and FDE."""
    tr, data = _trainer_for(dev, "sequenced", 4)
    default = tr.test()
    assert set(default) == {"ADE", "FDE"}
    res = tr.test(metrics="all")
    assert set(res) == {"ADE", "FDE", "TCC", "COL"}
    sums, n = {k: 0.0 for k in res}, 0
    with torch.no_grad():
        for idx in range(len(data)):
            obs, pred, addl = tr._scene(data, idx)
            out = tr.model.evaluate_metrics(obs.to(dev), pred.to(dev), addl)
            for key in sums:
                sums[key] += float(out[key].double().sum())
            n += out["ADE"].numel()
    for key in res:
        assert res[key] == pytest.approx(sums[key] / n, rel=1e-9, abs=1e-12), key
    assert res["ADE"] == pytest.approx(default["ADE"], rel=1e-5) and res["FDE"] == pytest.approx(default["FDE"], rel=1e-5)
    assert 0.0 <= res["COL"] <= 100.0 and -1.0 <= res["TCC"] <= 1.0


def test_scene_sizes_are_checked(dev, ops):
    pred = torch.zeros((2, 5, 12, 2), device=dev)
    gt = torch.zeros((5, 12, 2), device=dev)
    with pytest.raises(ValueError):
        ops.traj_metrics(pred, gt, scene_sizes=[2, 2])
    with pytest.raises(ValueError):
        ops.traj_metrics(pred, gt, scene_sizes=[6, -1])
    out = ops.traj_metrics(pred, gt, scene_sizes=[0, 5, 0])  # empty scenes are allowed
    assert torch.all(out["COL"] == 100)  # five pedestrians on one spot: every one collides in every sample


def T_(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
