"""Native Graph-TERN on the GPU (csrc/et_graphtern.hip): the graph form against the reference's recorded network outputs
(tests/golden/g27_graphtern.npz), the scene form against the fp64 restatement (tests/_graphtern_np.py) fed the fp32 input
the kernel reports, the scene form against the graph form through the bridge, a scene alone against the same scene inside
a split, a NaN coefficient, errors, empty inputs, graph capture, and whole splits end to end.

The network's graphs hold inverse distances, so its output is not stable under a 1-ulp change of a coefficient (the
reference's own output moves by per cent on most scenes of some splits, tools/make_golden_graphtern.py): every strict
comparison below is made on ONE fp32 network input, where the network is well conditioned (the reference's fp32 run against
its fp64 run: 4.4e-7), with no exclusions.  End to end only the split means are compared, within the spread the reference
shows against itself; there is no per-pedestrian comparison against the reference's ADE / FDE.

Measured on the MI355X (figures in DESIGN §4 "Graph-TERN"): graph form against the reference <= 3.8e-7 of the largest
entry, scene form against the restatement <= 7.3e-7, scene form against graph form bit-equal; the device's C_obs is within
2.0 of the draws' units of the reference's on eth; the split means are within 1.4e-8 / 5.9e-9 (eth ADE / FDE), 1.3e-8 /
2.9e-8 (zara1), 3.6e-6 / 2.8e-5 (zara2) of the reference's.

Other members of the supported family (ranks 1 to 32, S 1 to 64, the block counts' limits, chunked later blocks, a rel no
bridge builds, guard bands, the "fits nowhere" branch): tests/test_gpu_graphtern_shapes.py."""
import numpy as np
import pytest
import torch

from . import _golden as G
from . import _graphtern_np as GN
from ._gpu_common import *  # noqa: F401,F403 -- fixtures (dev, ops) and helpers

pytestmark = pytest.mark.gpu
Z = G.load("g27_graphtern.npz")
G2 = G.load("g2_fit_all_scenes.npz")
PICKS = sorted({k.split(".")[0] for k in Z.files if k.startswith("pick")}, key=lambda t: int(t[4:]))
HAND = ["grid", "single", "pair", "edge"]
TOL = 1e-5
LDS_MAX_N = 35  # S = 20, k = 6: 6 * 8 + 3 * 128 = 432 floats per pedestrian in a 60 KiB arena
GEN = dict(n_epgcn=2, n_epcnn=3, n_smpl=12)


def state(prefix):
    return {k[len(prefix):]: torch.from_numpy(np.array(Z[k])) for k in Z.files
            if k.startswith(prefix) and not k[len(prefix):].startswith("net_out")}


SD = {k: v.numpy() for k, v in state("net.").items()}
SD_GEN = {k: v.numpy() for k, v in state("gen.").items()}


def net(dev, prefix="net.", **kw):
    from eigentrajectory_amd.graphtern import GraphTERNLight
    args = dict(n_epgcn=1, n_epcnn=6, input_feat=1, seq_len=8, pred_seq_len=6, n_smpl=20)
    args.update(kw)
    m = GraphTERNLight(**args)
    m.load_state_dict(state(prefix), strict=True)
    return m.to(dev).eval()


def scale_err(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def wrapper(dev, scene, predictor):
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    hp = default_hyper_params(lr=1e-3, weight_decay=1e-4, static_dist=G.static_dist(scene))
    model = EigenTrajectory(predictor, get_hook_func("graphtern"), hp)
    sd = model.state_dict()
    for k in sd:
        if k.startswith("ET_"):
            sd[k] = torch.from_numpy(G2[f"{scene}.{k}"])
    model.load_state_dict(sd)
    return model.to(dev).eval()


def split(scene, dev):
    obs, pred, sse = G.dataset(scene, "test")
    return T(obs, dev), T(pred, dev), np.asarray(sse)


_synthetic = GN.synthetic_split  # (n or the scene sizes, seed, k = 6): the split generator, shared with the shapes file


def _check_scenes(ops, m, sd, C_obs, nrm, sizes, tol=TOL):
    """the scene form on (C_obs, nrm, sizes) against the restatement fed the returned graph_inputs; graph_inputs itself:
    the C_obs rows bit for bit, the obs_ori rows within 2 ulp (at the scale of the scene's positions: both sides are a
    fp32 mean in their own summation order, subtracted once) of the numpy fp32 value"""
    dev = next(m.parameters()).device
    out, det = ops.graphtern_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=sizes, want_details=True)
    out, gin = N_(out), N_(det["graph_inputs"])
    k = C_obs.shape[0]
    assert np.array_equal(gin[:k], C_obs)
    lo, worst = 0, 0.0
    for n in ([C_obs.shape[1]] if sizes is None else sizes):
        if n == 0:
            continue
        u = gin[:, lo:lo + n]
        ulp = np.spacing(np.abs(nrm[:2, lo:lo + n]).max().astype(np.float32))
        assert np.abs(u[k:].astype(np.float64) - GN.scene_input(C_obs, nrm, lo, lo + n)[k:]).max() <= 2 * ulp, (lo, n)
        err = scale_err(out[:, lo:lo + n], GN.forward(sd, u))
        worst = max(worst, err)
        assert err <= tol, (lo, n, err)
        lo += n
    print(f"scenes {sizes}: {worst:.2e}")
    return out


def test_graph_form_equals_the_reference(dev):
    """every eth scene, all picks, the hand-built scenes and the generic weights; no exclusions: the input is the
    reference's own fp32 network input"""
    m = net(dev)
    s_all, lo, worst = Z["eth.s_obs"], 0, 0.0
    for i, n in enumerate(Z["eth.scene_size"].tolist()):
        s_obs = T(s_all[:, :, lo:lo + n][None, :, :, :, None], dev)
        out = m(s_obs)
        assert out.shape == (1, 6, n, 20)
        err = scale_err(N_(out)[0], Z["eth.net_out"][:, lo:lo + n])
        worst = max(worst, err)
        assert err <= TOL, ("eth", i, n, err)
        lo += n
    print(f"eth, {len(Z['eth.scene_size'])} scenes: {worst:.2e}")
    for t in PICKS + HAND:
        out = m(T(Z[f"{t}.s_obs"], dev))
        assert out.shape == Z[f"{t}.net_out"].shape
        err = scale_err(N_(out), Z[f"{t}.net_out"])
        print(f"{t} n={out.shape[2]}: {err:.2e}")
        assert err <= TOL, t
    gen = net(dev, "gen.", **GEN)
    for i, t in enumerate(PICKS[:2]):
        err = scale_err(N_(gen(T(Z[f"{t}.s_obs"], dev))), Z[f"gen.net_out{i}"])
        print(f"gen {t}: {err:.2e}")
        assert err <= TOL, t


@pytest.mark.parametrize("sizes", [[1, 2, 3, 12, 13, 14, 63, 64, 65, 130], [LDS_MAX_N, LDS_MAX_N + 1], [0, 3, 0, 4, 0],
                                   [2, 600, 2]], ids=["halo-and-wave", "lds-switch", "empties", "ragged"])
def test_scene_form_matches_the_restatement(dev, ops, sizes):
    from eigentrajectory_amd import _lib
    C_obs, nrm = _synthetic(sum(sizes), len(sizes))
    m = net(dev)
    _check_scenes(ops, m, SD, C_obs, nrm, sizes)
    if sizes[0] == LDS_MAX_N:  # the two sizes are either side of the switch
        p, _ = m.et_params()
        ws = lambda mx: int(_lib.lib().et_graphtern_workspace_bytes(_lib.C.byref(p), 100, mx))
        assert ws(LDS_MAX_N) == 0 and ws(LDS_MAX_N + 1) > 0


def test_synthetic_inputs_have_exact_zeros_off_the_diagonal():
    C_obs, nrm = _synthetic(65, 1)
    u = GN.scene_input(C_obs, nrm, 0, 65)
    off = ~np.eye(65, dtype=bool)
    assert ((GN.distances(u) == 0) & off).any(axis=(1, 2))[:6].all()       # coincident columns, rounded values, zeros
    assert ((GN.distances(GN.rel_of(u)) == 0) & off).any(axis=(1, 2))[1:6].all()
    assert (C_obs == 0).all(axis=0).any()


def test_generic_weights_scene_form(dev, ops):
    """two st_mrgcn blocks (C_in = 16, identity residual, chunked contraction), three epcnn blocks (first / middle / last),
    S = 12, in LDS and in the workspace"""
    gen = net(dev, "gen.", **GEN)
    sizes = [7, 70, 1]
    C_obs, nrm = _synthetic(sum(sizes), 5)
    _check_scenes(ops, gen, SD_GEN, C_obs, nrm, sizes)


def test_a_scene_alone_equals_the_scene_inside_a_split(dev, ops):
    """bit for bit, with the arena in LDS and in the workspace: a replicate clamp taken at the split's ends instead of the
    scene's, or a sum that depends on where the arena lies, shows here"""
    m = net(dev)
    sizes = [5, 63, LDS_MAX_N, 0, LDS_MAX_N + 1, 1, 2]
    C_obs, nrm = _synthetic(sum(sizes), 9)
    whole = N_(ops.graphtern_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=sizes))
    again = N_(ops.graphtern_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=sizes))
    assert np.array_equal(whole, again) and np.isfinite(whole).all()
    lo = 0
    for n in sizes:
        if n:
            c, r = np.ascontiguousarray(C_obs[:, lo:lo + n]), np.ascontiguousarray(nrm[:, lo:lo + n])
            assert np.array_equal(N_(ops.graphtern_forward_scenes(m, T(c, dev), T(r, dev))), whole[:, lo:lo + n]), (lo, n)
        lo += n


@pytest.mark.parametrize("scene", ["eth", "hotel"])
def test_scene_form_equals_graph_form_through_the_bridge(dev, ops, scene):
    """every scene, on the device's own C_obs: rel and the distances formed in the kernel vs the bridge's S_obs; both see
    the same u"""
    model = wrapper(dev, scene, net(dev))
    obs, pred, sse = split(scene, dev)
    U_obs_m, _, U_obs_s, _ = model._U()
    C_obs, _, nrm, _ = ops.norm_project(obs, None, U_obs_m, None, U_obs_s, None, ops.MODE_SPLIT, model.static_dist,
                                        want_flag=False)
    sizes = (sse[:, 1] - sse[:, 0]).tolist()
    Cc, det = ops.graphtern_forward_scenes(model.baseline_model, C_obs, nrm, scene_sizes=sizes, want_details=True)
    gin, k = det["graph_inputs"], C_obs.shape[0]
    assert torch.equal(gin[:k], C_obs)
    errs = []
    for s, e in sse:
        ref = model._predict(gin[:k, s:e], gin[k:, s:e], None)
        assert ref.shape == (k, e - s, 20)
        errs.append((Cc[:, s:e] - ref).abs().max() / ref.abs().max())
    worst = float(torch.stack(errs).max())
    print(f"{scene}: {len(errs)} scenes, {worst:.2e}")
    assert worst <= TOL


def test_nan_stays_in_its_scene(dev, ops):
    m = net(dev)
    sizes = [4, 9, 40, 3]
    C_obs, nrm = _synthetic(sum(sizes), 4)
    clean = N_(ops.graphtern_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=sizes))
    bad = C_obs.copy()
    bad[2, 6] = np.nan  # scene 1
    out = N_(ops.graphtern_forward_scenes(m, T(bad, dev), T(nrm, dev), scene_sizes=sizes))
    torch.cuda.synchronize()
    assert np.isnan(out[:, 4:13]).any() and np.isnan(out[:, 6]).all()
    with np.errstate(invalid="ignore"):  # the restatement (and the reference's arithmetic): the whole scene is NaN
        ref = GN.forward(SD, GN.scene_input(bad, nrm, 4, 13))
    assert np.isnan(ref).all() and np.array_equal(np.isnan(out[:, 4:13]), np.isnan(ref))
    keep = np.r_[0:4, 13:56]
    assert np.array_equal(out[:, keep], clean[:, keep]) and np.isfinite(clean).all()


def test_errors_and_empty_inputs(dev, ops):
    from eigentrajectory_amd._lib import ETLibraryError
    from eigentrajectory_amd.graphtern import GraphTERNLight
    good = net(dev)
    for kw in (dict(n_smpl=65), dict(seq_len=9), dict(input_feat=2), dict(n_epgcn=5), dict(n_epcnn=1), dict(n_epcnn=9)):
        args = dict(n_epgcn=1, n_epcnn=6, input_feat=1, seq_len=8, pred_seq_len=6, n_smpl=20)
        args.update(kw)
        bad = GraphTERNLight(**args).to(dev).eval()
        with pytest.raises(ETLibraryError, match="status 3"):
            ops.graphtern_forward_graph(bad, torch.zeros((1, 2, args["seq_len"], 3, 1), device=dev))
        with pytest.raises(ETLibraryError, match="status 3"):
            ops.graphtern_forward_scenes(bad, torch.zeros((6, 3), device=dev), torch.zeros((4, 3), device=dev))
    for shape in ((1, 2, 8, 3), (1, 1, 8, 3, 1), (1, 2, 7, 3, 1), (2, 8, 3, 1)):
        with pytest.raises(ValueError):
            ops.graphtern_forward_graph(good, torch.zeros(shape, device=dev))
    with pytest.raises(ValueError):
        ops.graphtern_forward_scenes(good, torch.zeros((5, 3), device=dev), torch.zeros((4, 3), device=dev))
    with pytest.raises(ValueError):
        ops.graphtern_forward_scenes(good, torch.zeros((6, 3), device=dev), torch.zeros((4, 2), device=dev))
    with pytest.raises(ValueError):
        ops.graphtern_forward_scenes(good, torch.zeros((6, 3), device=dev), torch.zeros((4, 3), device=dev), scene_sizes=[])
    # no scenes, and empty scenes among others
    out = ops.graphtern_forward_scenes(good, torch.zeros((6, 0), device=dev), torch.zeros((4, 0), device=dev), scene_sizes=[])
    assert out.shape == (6, 0, 20)
    assert ops.graphtern_forward_scenes(good, torch.zeros((6, 0), device=dev), torch.zeros((4, 0), device=dev)).shape == (6, 0, 20)
    assert good(torch.zeros((1, 2, 8, 0, 1), device=dev)).shape == (1, 6, 0, 20)
    C_obs, nrm = _synthetic(7, 2)
    a = N_(ops.graphtern_forward_scenes(good, T(C_obs, dev), T(nrm, dev), scene_sizes=[0, 3, 0, 4, 0]))
    b = N_(ops.graphtern_forward_scenes(good, T(C_obs, dev), T(nrm, dev), scene_sizes=[3, 4]))
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


@pytest.mark.parametrize("scene", ["eth", "zara1", "zara2"])
def test_split_end_to_end(dev, ops, scene):
    """evaluate_split (3 launches: projection, et_graphtern_forward_scenes, reconstruction + metrics) against the
    reference's split means, within 8 x the spread the reference's own means show under
    1-ulp draws of its input (+ 1e-5 of the mean): a wiring check (descriptors, static_dist, layout) -- the strict checks
    are the ones above.  ETTrainer.test's default per-scene path gives the same means."""
    model = wrapper(dev, scene, net(dev))
    obs, pred, sse = split(scene, dev)
    res = model.evaluate_split(obs, pred, sse)
    if scene == "eth":
        U_obs_m, _, U_obs_s, _ = model._U()
        C_obs, _, _, _ = ops.norm_project(obs, None, U_obs_m, None, U_obs_s, None, ops.MODE_SPLIT, model.static_dist,
                                          want_flag=False)
        mine, ref, lo, worst = N_(C_obs), Z["eth.c_obs"], 0, 0.0
        for n in Z["eth.scene_size"].tolist():  # in the draws' unit: 2^-23 of the scene's largest |C_obs|
            worst = max(worst, float(np.abs(mine[:, lo:lo + n].astype(np.float64) - ref[:, lo:lo + n]).max()
                                     / (np.abs(ref[:, lo:lo + n]).max() * 2.0 ** -23)))
            lo += n
        print(f"eth: the device's C_obs is within {worst:.1f} ulp (of the scene's largest coefficient) of the reference's")
    for key in ("ADE", "FDE"):
        got = float(N_(res[key]).mean(dtype=np.float64))
        ref, spread = float(Z[f"{scene}.{key.lower()}_mean"]), float(Z[f"{scene}.{key.lower()}_spread"])
        print(f"{scene} {key}: mean {got:.6f}, reference {ref:.6f}, apart {abs(got - ref):.2e}, bound "
              f"{8 * spread + 1e-5 * ref:.2e} (spread {spread:.1e})")
        assert abs(got - ref) <= 8 * spread + 1e-5 * ref, key
    if scene == "eth":
        from eigentrajectory_amd.data import TrajectoryData
        from eigentrajectory_amd.trainer import ETTrainer
        data = TrajectoryData.from_arrays(N_(obs), N_(pred), sse)
        tr = ETTrainer(model, model.hyper_params, data, data, data, mode="sequenced", device=dev)
        means = tr.test()
        for key in ("ADE", "FDE"):
            mine = float(N_(res[key]).mean(dtype=np.float64))
            print(f"ETTrainer.test {key}: {abs(means[key] - mine):.2e} from evaluate_split")
            assert abs(means[key] - mine) <= 1e-5
