"""Native AgentFormer on the GPU (csrc/et_agentformer.hip): the module form through the agentformer hooks against the
reference's recorded network outputs (tests/golden/g26_agentformer_net.npz), the scene form against the fp64 restatement
(tests/_agentformer_np.py) fed the fp32 input the kernels report and bit for bit against the module form, the
128-pedestrian scene, isolation of scenes, in-place weight edits, whole splits end to end against the reference's
per-pedestrian ADE / FDE, determinism, capture and replay, the scene limit, errors and empty inputs.

TOL = 1e-5 of the largest entry is the bound the other predictor tests use for a fp32 result (about ten times the
reference's own fp32 error against its float64 run, <= 9.6e-7 on these scenes).  Measured on the MI355X (DESIGN §4
"AgentFormer"): module form against the reference <= 1.15e-6 (ET, the scene of 128) and <= 5.6e-7 (generic); scene form
against the restatement 9.0e-7 / 4.2e-7, the scene of 128 9.0e-7, before / after weight edits 5.5e-7 / 4.0e-7; end to end per pedestrian ADE /
FDE <= 7.4e-7 / 1.2e-6 of the split's largest, means within 9.0e-8; every bit-equality below holds."""
import ctypes as C

import numpy as np
import pytest
import torch

from . import _agentformer_np as AN
from . import _golden as G
from ._gpu_common import *  # noqa: F401,F403 -- fixtures (dev, ops) and helpers

pytestmark = pytest.mark.gpu
Z = G.load("g26_agentformer_net.npz")
G2 = G.load("g2_fit_all_scenes.npz")
ET_SCENES = ["univ57", "univ_mid", "n1", "n2", "n16", "n17", "n128"]
GEN_SCENES = ["n1", "n2", "n16", "n17"]
GEN = dict(tf_model_dim=64, tf_nhead=4, tf_ff_dim=96, context_encoder={"nlayer": 1}, future_decoder={"nlayer": 3})
TOL = 1e-5
SIZES = [3, 1, 5, 17, 2, 16, 1]  # scene boundaries inside 16-token tiles (24, 32, 72, ...), 17 and 16 span several tiles


def net(dev, tag="et"):
    from eigentrajectory_amd.agentformer import AgentFormerLight, et_config
    m = AgentFormerLight(et_config(6, 20) if tag == "et" else et_config(4, 3, **GEN))
    own = m.state_dict()
    m.load_state_dict({k: own[k] if v is None else torch.from_numpy(v) for k, v in AN.fixture_weights(Z, tag).items()},
                      strict=True)
    return m.to(dev).eval()


def state_np(m):
    return {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}


def scale_err(got, ref):
    """largest difference over the largest entry; the NaNs must be in the same places"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref))
    return float(np.nanmax(np.abs(got - ref)) / max(np.nanmax(np.abs(ref)), 1e-30))


def through_the_hooks(m, u):
    """pre-hook, forward and post-hook of the agentformer bridge on u (T, n) = [C_obs; obs_ori] -> (k, n, S), and the data"""
    from eigentrajectory_amd.bridges import BRIDGES
    pre, fwd, post = BRIDGES["agentformer"]
    data = fwd(pre(u[:-2], u[-2:]), m)
    return post(data), data


def wrapper(dev, scene, predictor):
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    hp = default_hyper_params(lr=1e-3, weight_decay=1e-4, static_dist=float(Z[f"{scene}.static_dist"]))
    model = EigenTrajectory(predictor, get_hook_func("agentformer"), hp)
    sd = model.state_dict()
    for k in sd:
        if k.startswith("ET_"):
            sd[k] = torch.from_numpy(G2[f"{scene}.{k}"])
    model.load_state_dict(sd)
    return model.to(dev).eval()


def synthetic(sizes, seed, k=6):
    rng = np.random.default_rng(seed)
    n = sum(sizes)
    return rng.normal(0, 1, (k, n)).astype(np.float32), rng.normal(0, 5, (4, n)).astype(np.float32)


@pytest.mark.parametrize("tag", ["et", "gen"])
def test_module_form_equals_the_reference(dev, tag):
    m = net(dev, tag)
    for s in (ET_SCENES if tag == "et" else GEN_SCENES):
        u = T(Z[f"{tag}.{s}.u"], dev)
        out, data = through_the_hooks(m, u)
        ref = Z[f"{tag}.{s}.seq_out"]
        err = scale_err(N_(out), ref)
        print(f"{tag}.{s} n={u.shape[1]}: {err:.2e}")
        assert err <= TOL, s
        assert data["_dec_motion"].shape == (u.shape[1], ref.shape[0], ref.shape[2]) and data["_dec_motion"].is_contiguous()
        assert torch.equal(data["_seq_out"], out) and data["agent_num"] == data["batch_size"] == u.shape[1]
        assert data["pre_motion"].shape == (u.shape[0], u.shape[1], 1) and data["context_enc"] is None


def check_scenes(ops, m, tag, C_obs, nrm, sizes):
    """the scene form against the restatement fed the returned graph_inputs, and bit for bit against the module form;
    graph_inputs itself: the C_obs rows bit for bit, the obs_ori rows within 2 ulp (at the scale of the scene's positions:
    both sides are a fp32 mean in their own summation order, subtracted once) of the numpy fp32 value"""
    dev = next(m.parameters()).device
    out, det = ops.agentformer_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=sizes, want_details=True)
    gin_dev = det["graph_inputs"]
    out_np, gin = N_(out), N_(gin_dev)
    k = C_obs.shape[0]
    assert np.array_equal(gin[:k], C_obs) and out_np.shape == (k, C_obs.shape[1], m.forecast_dim)
    sd, nhead = state_np(m), m.nhead
    lo, worst = 0, 0.0
    for n in sizes:
        if n == 0:
            continue
        u = gin[:, lo:lo + n]
        ulp = np.spacing(np.abs(nrm[:2, lo:lo + n]).max().astype(np.float32))
        assert np.abs(u[k:].astype(np.float64) - AN.scene_input(C_obs, nrm, lo, lo + n)[k:]).max() <= 2 * ulp, (lo, n)
        err = scale_err(out_np[:, lo:lo + n], AN.c_pred_refine(AN.forward(sd, u, nhead)))
        worst = max(worst, err)
        assert err <= TOL, (lo, n, err)
        alone, _ = through_the_hooks(m, gin_dev[:, lo:lo + n].contiguous())
        assert torch.equal(alone, out[:, lo:lo + n]), (lo, n)
        lo += n
    print(f"{tag} scenes {sizes}: {worst:.2e}")
    return out_np


@pytest.mark.parametrize("tag", ["et", "gen"])
def test_scene_form_matches_the_restatement_and_the_module_form(dev, ops, tag):
    m = net(dev, tag)
    C_obs, nrm = synthetic(SIZES, 3, k=m.future_frames)
    check_scenes(ops, m, tag, C_obs, nrm, SIZES)


def test_the_largest_scene(dev, ops):
    """128 pedestrians: 1024 encoder and 768 decoder tokens, 64 key blocks per query tile"""
    m = net(dev)
    C_obs, nrm = synthetic([128], 5)
    check_scenes(ops, m, "et", C_obs, nrm, [128])


def test_scenes_do_not_see_each_other(dev, ops):
    """a NaN in one scene makes that scene NaN and leaves every other scene bit-equal; the scenes in reverse order give the
    same rows bit for bit; two calls agree bit for bit"""
    m = net(dev)
    C_obs, nrm = synthetic(SIZES, 7)
    run = lambda c, r, s: N_(ops.agentformer_forward_scenes(m, T(c, dev), T(r, dev), scene_sizes=s))
    whole = run(C_obs, nrm, SIZES)
    assert np.isfinite(whole).all() and np.array_equal(whole, run(C_obs, nrm, SIZES))
    off = np.concatenate([[0], np.cumsum(SIZES)])
    bad = C_obs.copy()
    bad[2, off[3] + 4] = np.nan  # one coefficient of one pedestrian of the scene of 17
    got = run(bad, nrm, SIZES)
    assert np.isnan(got[:, off[3]:off[4]]).all()
    keep = np.r_[0:off[3], off[4]:off[-1]]
    assert np.array_equal(got[:, keep], whole[:, keep])
    order = np.concatenate([np.arange(off[i], off[i + 1]) for i in reversed(range(len(SIZES)))])
    rev = run(np.ascontiguousarray(C_obs[:, order]), np.ascontiguousarray(nrm[:, order]), SIZES[::-1])
    assert np.array_equal(rev, whole[:, order])
    padded = run(C_obs, nrm, [0] + SIZES[:3] + [0, 0] + SIZES[3:] + [0])  # empty scenes among the others
    assert np.array_equal(padded, whole)


def test_weights_are_read_in_place(dev, ops):
    """an edit of one tensor of layer 1 and of one bias changes the next call to what the restatement gives"""
    m = net(dev, "gen")
    sizes = [5, 17, 2]
    C_obs, nrm = synthetic(sizes, 9, k=4)
    before = check_scenes(ops, m, "gen", C_obs, nrm, sizes)
    with torch.no_grad():
        m.future_decoder.tf_decoder.layers[1].multihead_attn.in_proj_weight_self.mul_(1.5)
        m.context_encoder.tf_encoder.layers[0].self_attn.in_proj_bias.add_(0.25)
    after = check_scenes(ops, m, "gen", C_obs, nrm, sizes)
    assert np.abs(after - before).max() / np.abs(before).max() > 1e-3


@pytest.mark.parametrize("scene", ["eth", "hotel", "univ"])
def test_split_end_to_end(dev, scene):
    """evaluate_split against the reference's per-pedestrian ADE / FDE (every test scene of eth and hotel, every tenth of
    univ) on the robust scenes, the means over all of them"""
    model = wrapper(dev, scene, net(dev))
    obs, pred, sse = G.dataset(scene, "test")
    sse = np.asarray(sse)[Z[f"{scene}.scene_index"]]
    rows = np.concatenate([np.arange(s, e) for s, e in sse])
    sizes = sse[:, 1] - sse[:, 0]
    assert np.array_equal(sizes, Z[f"{scene}.scene_size"])
    ends = np.cumsum(sizes)
    new_sse = np.stack([ends - sizes, ends], axis=1)
    res = model.evaluate_split(T(obs[rows], dev), T(pred[rows], dev), new_sse)
    robust = np.repeat(Z[f"{scene}.robust"], sizes)
    assert robust.mean() >= 0.9
    for key in ("ADE", "FDE"):
        ref = Z[f"{scene}.{key.lower()}"]
        got = N_(res[key]).astype(np.float64)
        err = np.abs(got - ref) / np.abs(ref).max()
        print(f"{scene} {key}: {len(sizes)} scenes, robust rows {err[robust].max():.2e}, all rows {err.max():.2e}, means "
              f"{abs(float(got.mean()) - float(ref.mean(dtype=np.float64))):.2e}")
        assert err[robust].max() <= TOL, key
        assert abs(float(got.mean()) - float(ref.mean(dtype=np.float64))) <= 3e-4


def test_hook_path_captured_and_replayed(dev):
    """capture and replay equals eager, and the replay sees an in-place edit of the weights"""
    model = wrapper(dev, "eth", net(dev))
    obs, _, sse = G.dataset("eth", "test")
    s, e = (int(v) for v in sse[np.argmax(np.asarray(sse)[:, 1] - np.asarray(sse)[:, 0])])
    o = T(obs[s:e], dev)
    eager = model.forward(o)["recon_traj"].clone()
    rep = model.forward_replayed(o)["recon_traj"].clone()
    assert torch.equal(rep, eager)
    new = {k: v + 0.05 * torch.randn_like(v) for k, v in model.baseline_model.state_dict().items() if not k.endswith(".pe")}
    model.baseline_model.load_state_dict(new, strict=False)  # in place: the captured graph sees the new weights
    eager2 = model.forward(o)["recon_traj"].clone()
    rep2 = model.forward_replayed(o)["recon_traj"].clone()
    assert not torch.equal(eager2, eager)
    assert torch.equal(rep2, eager2)


def test_a_scene_beyond_the_scene_limit_is_not_computed(dev, ops):
    from eigentrajectory_amd._lib import AGENTFORMER_MAX_SCENE_N
    m = net(dev, "gen")
    sizes = [3, AGENTFORMER_MAX_SCENE_N + 1, 4]
    C_obs, nrm = synthetic(sizes, 6, k=4)
    out, det = ops.agentformer_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=sizes, want_details=True)
    out = N_(out)
    assert np.isnan(out[:, 3:-4]).all() and np.isnan(N_(det["graph_inputs"])[:, 3:-4]).all()
    for lo, hi in ((0, 3), (sum(sizes) - 4, sum(sizes))):
        c, r = np.ascontiguousarray(C_obs[:, lo:hi]), np.ascontiguousarray(nrm[:, lo:hi])
        assert np.array_equal(N_(ops.agentformer_forward_scenes(m, T(c, dev), T(r, dev))), out[:, lo:hi])
        assert np.isfinite(out[:, lo:hi]).all()
    with pytest.raises(ValueError):  # one scene, no offsets: refused on the host like the module form
        ops.agentformer_forward_scenes(m, T(C_obs, dev), T(nrm, dev))
    with pytest.raises(ValueError):
        ops.agentformer_forward_graph(m, torch.zeros((6, AGENTFORMER_MAX_SCENE_N + 1, 1), device=dev))


def test_errors_and_empty_inputs(dev, ops):
    from eigentrajectory_amd import _lib as L
    m = net(dev, "gen")
    params, _ = m.et_params()
    u = torch.zeros((6, 3), device=dev)
    out = torch.zeros((4, 3, 3), device=dev)
    nbytes = L.lib().et_agentformer_workspace_bytes(C.byref(params), 3, 3)
    ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    with pytest.raises(L.ETLibraryError, match="status 4"):  # ET_ERR_WORKSPACE
        L.call("et_agentformer_forward_graph", C.byref(params), L.ptr(u), 3, L.ptr(out), L.ptr(ws), nbytes - 1, L.stream(dev))
    params.dec[2].norm_bias[2] = None
    with pytest.raises(ValueError):  # ET_ERR_INVALID_ARG: a NULL tensor
        L.call("et_agentformer_forward_graph", C.byref(params), L.ptr(u), 3, L.ptr(out), L.ptr(ws), nbytes, L.stream(dev))
    with pytest.raises(ValueError):
        ops.agentformer_forward_graph(m, torch.zeros((8, 3, 1), device=dev))
    with pytest.raises(ValueError):
        ops.agentformer_forward_scenes(m, torch.zeros((6, 3), device=dev), torch.zeros((4, 3), device=dev))
    with pytest.raises(ValueError):
        ops.agentformer_forward_scenes(m, torch.zeros((4, 3), device=dev), torch.zeros((4, 3), device=dev), scene_sizes=[2, 2])
    m.train()
    m.set_data({"pre_motion": torch.zeros((6, 3, 1), device=dev)})
    with pytest.raises(RuntimeError, match="training"):
        m()
    m.eval()
    # no pedestrians, no scenes
    res, det = ops.agentformer_forward_scenes(m, torch.zeros((4, 0), device=dev), torch.zeros((4, 0), device=dev),
                                              scene_sizes=[], want_details=True)
    assert res.shape == (4, 0, 3) and det["graph_inputs"].shape == (6, 0)
    assert ops.agentformer_forward_scenes(m, torch.zeros((4, 0), device=dev), torch.zeros((4, 0), device=dev)).shape == (4, 0, 3)
    m.set_data({"pre_motion": torch.zeros((6, 0, 1), device=dev)})
    assert m()["_dec_motion"].shape == (0, 4, 3)
