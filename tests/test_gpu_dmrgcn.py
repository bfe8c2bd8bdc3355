"""Native DMRGCN on the GPU (csrc/et_dmrgcn.hip): the graph form against the reference's recorded network outputs
(tests/golden/g23_dmrgcn.npz), the scene form against the fp64 restatement (tests/_dmrgcn_np.py) fed the fp32 input the
kernel reports, moved split values, the scene form against the graph form through the bridge, whole splits end to end
against the reference's per-pedestrian ADE / FDE, determinism, errors, empty inputs and graph capture.

Measured on the MI355X (figures in DESIGN §4): every comparison below is within its bound.
Other members of the family (K from 3 to 34, S 1 to 64, up to 4 st and 8 tpcnn blocks, scenes up to 512, 300 scenes, a given
a no bridge builds): tests/test_gpu_dmrgcn_shapes.py."""
import numpy as np
import pytest
import torch

from . import _dmrgcn_np as DN
from . import _golden as G
from ._gpu_common import *  # noqa: F401,F403 -- fixtures (dev, ops) and helpers

pytestmark = pytest.mark.gpu
Z = G.load("g23_dmrgcn.npz")
G2 = G.load("g2_fit_all_scenes.npz")
PICKS = sorted({k.split(".")[0] for k in Z.files if k.startswith("pick")}, key=lambda t: int(t[4:]))
TOL = 1e-5
LDS_MAX_N = 26  # S = 20, k = 6: 576 floats per pedestrian in a 60 KiB arena


def state(prefix):
    return {k[len(prefix):]: torch.from_numpy(np.array(Z[k])) for k in Z.files
            if k.startswith(prefix) and not k[len(prefix):].startswith("net_out")}


SD = {k: v.numpy() for k, v in state("net.").items()}


def net(dev, prefix="net.", **kw):
    from eigentrajectory_amd.dmrgcn import SocialDMRGCN
    args = dict(n_stgcn=1, n_tpcnn=4, input_feat=1, output_feat=20, seq_len=8, pred_seq_len=6, kernel_size=3)
    args.update(kw)
    m = SocialDMRGCN(**args)
    m.load_state_dict(state(prefix), strict=True)
    return m.to(dev).eval()


def scale_err(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def wrapper(dev, scene, predictor):
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    hp = default_hyper_params(lr=1e-3, weight_decay=1e-4, static_dist=float(Z[f"{scene}.static_dist"]))
    model = EigenTrajectory(predictor, get_hook_func("dmrgcn"), hp)
    sd = model.state_dict()
    for k in sd:
        if k.startswith("ET_"):
            sd[k] = torch.from_numpy(G2[f"{scene}.{k}"])
    model.load_state_dict(sd)
    return model.to(dev).eval()


def split(scene, dev):
    obs, pred, sse = G.dataset(scene, "test")
    return T(obs, dev), T(pred, dev), np.asarray(sse)


def _synthetic(n, seed, k=6):
    """coefficients with equal values in every row, a few identical columns, positions around the origin"""
    rng = np.random.default_rng(seed)
    C_obs = rng.normal(0, 1, (k, n)).astype(np.float32)
    C_obs[:, : n // 8] = np.round(C_obs[:, : n // 8], 1)
    nrm = rng.normal(0, 5, (4, n)).astype(np.float32)
    for i in range(0, n - 1, 5):  # coincident columns: the same pedestrian twice
        C_obs[:, i + 1], nrm[:, i + 1] = C_obs[:, i], nrm[:, i]
    return C_obs, nrm


def _check_scenes(ops, m, C_obs, nrm, sizes, tol=TOL, sd=None, label="scenes", **fw):
    """the scene form on (C_obs, nrm, sizes) against the restatement (of the state dict ``sd``, default the fixture's ET
    weights; ``fw``: its block counts and split values) fed the returned graph_inputs; graph_inputs itself: the C_obs rows
    bit for bit, the obs_ori rows within 2 ulp (at the scale of the scene's positions: both sides are a fp32 mean in their
    own summation order, subtracted once) of the numpy fp32 value"""
    sd = SD if sd is None else sd
    dev = next(m.parameters()).device
    out, det = ops.dmrgcn_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=sizes, want_details=True)
    out, gin = N_(out), N_(det["graph_inputs"])
    k = C_obs.shape[0]
    assert np.array_equal(gin[:k], C_obs)
    lo, worst = 0, 0.0
    for n in ([C_obs.shape[1]] if sizes is None else sizes):
        if n == 0:
            continue
        u = gin[:, lo:lo + n]
        ulp = np.spacing(np.abs(nrm[:2, lo:lo + n]).max().astype(np.float32))
        assert np.abs(u[k:].astype(np.float64) - DN.scene_input(C_obs, nrm, lo, lo + n)[k:]).max() <= 2 * ulp, (lo, n)
        err = scale_err(out[:, lo:lo + n], DN.c_pred_refine(DN.forward(sd, u, **fw)))
        worst = max(worst, err)
        assert err <= tol, (lo, n, err)
        lo += n
    print(f"{label} {sizes if sizes is None or len(sizes) <= 12 else f'{len(sizes)} scenes'}: {worst:.2e}")
    return out


def test_graph_form_equals_the_reference(dev):
    """no exclusions: the bins are exact comparisons of the given fp32 a"""
    m = net(dev)
    for t in PICKS + ["grid", "single"]:
        v, a = T(Z[f"{t}.v"], dev), T(Z[f"{t}.a"], dev)
        out, a_back = m(v, a)
        assert a_back is a and out.shape == Z[f"{t}.net_out"].shape
        err = scale_err(N_(out), Z[f"{t}.net_out"])
        print(f"{t} n={v.shape[-1]}: {err:.2e}")
        assert err <= TOL, t
    gen = net(dev, "gen.", n_stgcn=2, n_tpcnn=2, output_feat=12)
    for i, t in enumerate(PICKS[:2]):
        out, _ = gen(T(Z[f"{t}.v"], dev), T(Z[f"{t}.a"], dev))
        err = scale_err(N_(out), Z[f"gen.net_out{i}"])
        print(f"gen {t}: {err:.2e}")
        assert err <= TOL, t


@pytest.mark.parametrize("sizes", [[1, 2, 3, 63, 64, 65, 130], [LDS_MAX_N, LDS_MAX_N + 1], [0, 3, 0, 4, 0],
                                   [2, 1000, 2, 2, 1000, 2]], ids=["odd", "lds-switch", "empties", "ragged"])
def test_scene_form_matches_the_restatement(dev, ops, sizes):
    from eigentrajectory_amd import _lib
    C_obs, nrm = _synthetic(sum(sizes), len(sizes))
    m = net(dev)
    _check_scenes(ops, m, C_obs, nrm, sizes)
    if sizes[0] == LDS_MAX_N:  # the two sizes are either side of the switch
        p, _ = m.et_params()
        ws = lambda mx: int(_lib.lib().et_dmrgcn_workspace_bytes(_lib.C.byref(p), 100, mx))
        assert ws(LDS_MAX_N) == 0 and ws(LDS_MAX_N + 1) > 0


def test_one_large_scene_matches_the_restatement(dev, ops):
    C_obs, nrm = _synthetic(4096, 0)
    _check_scenes(ops, net(dev), C_obs, nrm, None, tol=1e-4)  # fp32 sums over 4 096 pedestrians against fp64


def test_generic_weights_scene_form(dev, ops):
    """two st_dmrgcn blocks (C_in = S, identity residual, chunked contraction), two tpcnn blocks, in LDS and in the workspace"""
    gen = net(dev, "gen.", n_stgcn=2, n_tpcnn=2, output_feat=12)
    sd = {k: v.numpy() for k, v in state("gen.").items()}
    sizes = [7, 40, 1]
    C_obs, nrm = _synthetic(sum(sizes), 5)
    out, det = ops.dmrgcn_forward_scenes(gen, T(C_obs, dev), T(nrm, dev), scene_sizes=sizes, want_details=True)
    gin, lo = N_(det["graph_inputs"]), 0
    for n in sizes:
        ref = DN.c_pred_refine(DN.forward(sd, gin[:, lo:lo + n], n_stgcn=2, n_tpcnn=2))
        assert scale_err(N_(out)[:, lo:lo + n], ref) <= TOL, (lo, n)
        lo += n


def _quarter_grid(n, seed):
    """every coefficient and position a multiple of 0.25; n a power of two, so the scene mean and obs_ori are exact"""
    rng = np.random.default_rng(seed)
    C_obs = (rng.integers(-12, 13, size=(6, n)) * 0.25).astype(np.float32)
    nrm = (rng.integers(-12, 13, size=(4, n)) * 0.25).astype(np.float32)
    return C_obs, nrm


@pytest.mark.parametrize("splits", [[[0.25, 0.75, 1.25, 2.5, 3.0], [0.5, 1.5, 1.75, 3.25, 5.0]],
                                    [[0.125, 0.375, 0.875, 1.625, 2.875], [0.125, 0.625, 1.125, 2.375, 4.125]]],
                         ids=["on-values", "in-gaps"])
def test_moved_splits(dev, ops, splits):
    """split values exactly on distances present in the input (those pairs are in no bin) and in the gaps between them"""
    m = net(dev)
    m.split = splits
    C_obs, nrm = _quarter_grid(32, 3)
    sizes = [16, 16]
    out = _check_scenes(ops, m, C_obs, nrm, sizes, split=splits)
    m.split = [list(s) for s in DN.SPLIT]
    assert not np.array_equal(out, N_(ops.dmrgcn_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=sizes)))
    u = DN.scene_input(C_obs, nrm, 0, 16)
    a = DN.adjacency(u)
    on = [bool((a[r] == np.float32(s)).any()) for r in range(2) for s in splits[r]]
    assert all(on) if splits[0][0] == 0.25 else not any(on)


@pytest.mark.parametrize("scene", G.SCENES)
def test_scene_form_equals_graph_form_through_the_bridge(dev, ops, scene):
    """every scene (every 7th of univ): the distances computed where they are used vs read from the bridge's a; both see
    the same u"""
    model = wrapper(dev, scene, net(dev))
    obs, pred, sse = split(scene, dev)
    U_obs_m, _, U_obs_s, _ = model._U()
    C_obs, _, nrm, _ = ops.norm_project(obs, None, U_obs_m, None, U_obs_s, None, ops.MODE_SPLIT, model.static_dist,
                                        want_flag=False)
    sizes = (sse[:, 1] - sse[:, 0]).tolist()
    Cc, det = ops.dmrgcn_forward_scenes(model.baseline_model, C_obs, nrm, scene_sizes=sizes, want_details=True)
    gin, k = det["graph_inputs"], C_obs.shape[0]
    assert torch.equal(gin[:k], C_obs)
    errs = []
    for s, e in sse[::1 if scene != "univ" else 7]:
        ref = model._predict(gin[:k, s:e], gin[k:, s:e], None)
        errs.append((Cc[:, s:e] - ref).abs().max() / ref.abs().max())
    worst = float(torch.stack(errs).max())
    print(f"{scene}: {len(errs)} scenes, {worst:.2e}")
    assert worst <= TOL


@pytest.mark.parametrize("scene", ["eth", "zara1", "zara2"])
def test_split_end_to_end(dev, scene):
    """evaluate_split (3 launches) against the reference's per-pedestrian ADE / FDE on the robust scenes (those on which
    an input a few ulp away decides every bin alike, tools/make_golden_dmrgcn.py), the split means over ALL scenes;
    ETTrainer.test's default per-scene path gives the same means."""
    model = wrapper(dev, scene, net(dev))
    obs, pred, sse = split(scene, dev)
    res = model.evaluate_split(obs, pred, sse)
    rows = np.repeat(Z[f"{scene}.robust"], Z[f"{scene}.scene_size"])
    assert rows.mean() >= 0.9
    for key in ("ADE", "FDE"):
        ref = Z[f"{scene}.{key.lower()}"]
        err = np.abs(N_(res[key]).astype(np.float64) - ref) / np.abs(ref).max()
        print(f"{scene} {key}: robust rows {err[rows].max():.2e}, all rows {err.max():.2e}, beyond {int((err > TOL).sum())}, "
              f"means {abs(float(N_(res[key]).mean(dtype=np.float64)) - float(ref.mean(dtype=np.float64))):.2e}")
        assert err[rows].max() <= TOL, key
        assert abs(float(N_(res[key]).mean(dtype=np.float64)) - float(ref.mean(dtype=np.float64))) <= 3e-4
    if scene == "eth":
        from eigentrajectory_amd.data import TrajectoryData
        from eigentrajectory_amd.trainer import ETTrainer
        data = TrajectoryData.from_arrays(N_(obs), N_(pred), sse)
        tr = ETTrainer(model, model.hyper_params, data, data, data, mode="sequenced", device=dev)
        means = tr.test()
        for key in ("ADE", "FDE"):
            mine = float(N_(res[key]).mean(dtype=np.float64))
            ref = float(Z[f"{scene}.{key.lower()}"].mean(dtype=np.float64))
            print(f"ETTrainer.test {key}: {abs(means[key] - mine):.2e} from evaluate_split, {abs(means[key] - ref):.2e} from the "
                  "reference")
            assert abs(means[key] - mine) <= 1e-5 and abs(means[key] - ref) <= 1e-5


def test_a_scene_alone_equals_the_scene_inside_a_split(dev, ops):
    """bit for bit, with the arena in LDS (5, 26) and in the workspace (27, 63)"""
    m = net(dev)
    sizes = [5, 63, LDS_MAX_N, 0, LDS_MAX_N + 1, 1]
    C_obs, nrm = _synthetic(sum(sizes), 9)
    whole = N_(ops.dmrgcn_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=sizes))
    again = N_(ops.dmrgcn_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=sizes))
    assert np.array_equal(whole, again) and np.isfinite(whole).all()
    lo = 0
    for n in sizes:
        if n:
            c, r = np.ascontiguousarray(C_obs[:, lo:lo + n]), np.ascontiguousarray(nrm[:, lo:lo + n])
            assert np.array_equal(N_(ops.dmrgcn_forward_scenes(m, T(c, dev), T(r, dev))), whole[:, lo:lo + n]), (lo, n)
        lo += n


def test_errors_and_empty_inputs(dev, ops):
    from eigentrajectory_amd._lib import ETLibraryError
    from eigentrajectory_amd.dmrgcn import SocialDMRGCN
    wide = net(dev)
    bad = SocialDMRGCN(n_stgcn=1, n_tpcnn=4, input_feat=1, output_feat=65, seq_len=8, pred_seq_len=6).to(dev).eval()
    with pytest.raises(ETLibraryError, match="status 3"):
        ops.dmrgcn_forward_graph(bad, torch.zeros((1, 1, 8, 3), device=dev), torch.zeros((1, 2, 8, 3, 3), device=dev))
    bad = SocialDMRGCN(n_stgcn=1, n_tpcnn=4, input_feat=1, output_feat=20, seq_len=9, pred_seq_len=6).to(dev).eval()
    with pytest.raises(ETLibraryError, match="status 3"):
        ops.dmrgcn_forward_scenes(bad, torch.zeros((6, 3), device=dev), torch.zeros((4, 3), device=dev))
    bad = net(dev)
    bad.split = [[0, 0.25, 0.5, 0.75, 1], [4, 2, 1, 0.5, 0]]
    with pytest.raises(ETLibraryError, match="status 3"):
        ops.dmrgcn_forward_scenes(bad, torch.zeros((6, 3), device=dev), torch.zeros((4, 3), device=dev))
    with pytest.raises(ValueError):
        ops.dmrgcn_forward_graph(wide, torch.zeros((1, 1, 8, 3), device=dev), torch.zeros((8, 3, 3), device=dev))
    # no scenes, and empty scenes among others
    out = ops.dmrgcn_forward_scenes(wide, torch.zeros((6, 0), device=dev), torch.zeros((4, 0), device=dev), scene_sizes=[])
    assert out.shape == (6, 0, 20)
    out, _ = wide(torch.zeros((1, 1, 8, 0), device=dev), torch.zeros((1, 2, 8, 0, 0), device=dev))
    assert out.shape == (1, 20, 6, 0)
    C_obs, nrm = _synthetic(7, 2)
    a = N_(ops.dmrgcn_forward_scenes(wide, T(C_obs, dev), T(nrm, dev), scene_sizes=[0, 3, 0, 4, 0]))
    b = N_(ops.dmrgcn_forward_scenes(wide, T(C_obs, dev), T(nrm, dev), scene_sizes=[3, 4]))
    assert np.array_equal(a, b) and np.isfinite(a).all()


def test_hook_path_captured_and_replayed(dev):
    model = wrapper(dev, "eth", net(dev))
    obs, pred, sse = split("eth", dev)
    s, e = (int(v) for v in sse[np.argmax(sse[:, 1] - sse[:, 0])])
    o = obs[s:e].contiguous()
    eager = model.forward(o)["recon_traj"].clone()
    rep = model.forward_replayed(o)["recon_traj"].clone()
    assert torch.equal(rep, eager)
    new = {k: v + 0.05 * torch.randn_like(v) for k, v in model.baseline_model.state_dict().items()}
    model.baseline_model.load_state_dict(new)  # in place: the captured graph sees the new weights
    eager2 = model.forward(o)["recon_traj"].clone()
    rep2 = model.forward_replayed(o)["recon_traj"].clone()
    assert not torch.equal(eager2, eager)
    assert torch.equal(rep2, eager2)
