"""Native PECNet / LBEBM on the GPU (csrc/et_mlp.hip): the module form against the reference's recorded ``predict`` outputs
(tests/golden/g24_pecnet.npz), the scene form against the fp64 restatement (tests/_pecnet_np.py) fed the fp32 inputs the
call reports, row independence bit for bit, the mask's semantics, whole splits end to end against the reference's
per-pedestrian ADE / FDE, weights read in place, determinism, graph capture, empty inputs and unsupported shapes.

TOL = 1e-5 of the largest entry is the project's bar for a native predictor; the reference's own fp32 output is within
3.8e-7 of its float64 run on the recorded calls (``ref_fp32_err``).  The one larger bound is 1e-4 for a scene of 1 024
pedestrians."""
import numpy as np
import pytest
import torch

from . import _golden as G
from . import _pecnet_np as PN
from ._gpu_common import *  # noqa: F401,F403 -- fixtures (dev, ops) and helpers
from .test_pecnet_cpu import TAGS, call_inputs, module, scale_err

pytestmark = pytest.mark.gpu
Z = G.load("g24_pecnet.npz")
G2 = G.load("g2_fit_all_scenes.npz")
TOL = 1e-5
CFGS = ["pecnet", "lbebm", "pecnet_gen", "lbebm_gen"]
POOLS = {"pecnet": 3, "pecnet_gen": 2, "lbebm": 0, "lbebm_gen": 0}
_SD, _NET = {}, {}


def sd_of(cfg):
    """the configuration's weights, generated once"""
    if cfg not in _SD:
        _SD[cfg] = PN.weights(Z, cfg)
    return _SD[cfg]


def net(dev, cfg):
    """the native module with the fixture's weights, built once per configuration (tests that edit it make their own)"""
    if cfg not in _NET:
        _NET[cfg] = fresh(dev, cfg)
    return _NET[cfg]


def fresh(dev, cfg):
    m = module(cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd_of(cfg).items()}, strict=True)
    return m.to(dev).eval()


def kind(cfg):
    return cfg.split("_")[0]


def predict(m, cfg, dev, past, ori, mask=None):
    past, ori = T(past, dev), T(ori, dev)
    if kind(cfg) == "pecnet":
        n = past.shape[0]
        mask = torch.ones((n, n), dtype=torch.bool, device=dev) if mask is None else T(mask, dev)
        return N_(m.predict(past, ori, mask, ori))
    return N_(m.predict(past, ori))


def scenes(ops, m, cfg, dev, C_obs, nrm, sizes, **kw):
    fn = ops.pecnet_forward_scenes if kind(cfg) == "pecnet" else ops.lbebm_forward_scenes
    return fn(m, T(C_obs, dev), T(nrm, dev), scene_sizes=sizes, **kw)


def _synthetic(n, seed, k):
    rng = np.random.default_rng(seed)
    C_obs = rng.normal(0, 1, (k, n)).astype(np.float32)
    nrm = rng.normal(0, 5, (4, n)).astype(np.float32)
    for i in range(0, n - 1, 5):  # coincident pedestrians
        C_obs[:, i + 1], nrm[:, i + 1] = C_obs[:, i], nrm[:, i]
    return C_obs, nrm


@pytest.mark.parametrize("cfg", CFGS)
def test_module_form_equals_the_reference(dev, cfg):
    """every recorded call: the picks, n = 1, the collated three-scene call, the mask with an all-zero row; no exclusions"""
    m = net(dev, cfg)
    for tag in TAGS:
        past, ori, mask = call_inputs(cfg, tag)
        out = predict(m, cfg, dev, past, ori, mask)
        ref = Z[f"{cfg}.{tag}.out"]
        assert out.shape == ref.shape
        err = scale_err(out, ref)
        print(f"{cfg} {tag} n={past.shape[0]}: {err:.2e}")
        assert err <= TOL, tag


def _check_scenes(ops, dev, cfg, sizes, seed, tol=TOL):
    """the scene form on synthetic rows against the restatement fed the reported inputs; the reported C_obs rows bit for
    bit, the obs_ori rows within 2 ulp (at the scale of the scene's positions) of the numpy fp32 value"""
    m, k, S = net(dev, cfg), int(Z[f"{cfg}.k"]), int(Z[f"{cfg}.S"])
    C_obs, nrm = _synthetic(sum(sizes), seed, k)
    out, det = scenes(ops, m, cfg, dev, C_obs, nrm, sizes, want_details=True)
    out, gin = N_(out), N_(det["net_inputs"])
    assert out.shape == (k, sum(sizes), S) and np.array_equal(gin[:k], C_obs)
    lo, worst = 0, 0.0
    for n in sizes:
        if n == 0:
            continue
        u = gin[:, lo:lo + n]
        ulp = np.spacing(np.abs(nrm[:2, lo:lo + n]).max().astype(np.float32))
        assert np.abs(u[k:].astype(np.float64) - PN.scene_input(C_obs, nrm, lo, lo + n)[k:]).max() <= 2 * ulp, (lo, n)
        err = scale_err(out[:, lo:lo + n], PN.scene_forward(kind(cfg), sd_of(cfg), u, POOLS[cfg], S))
        worst = max(worst, err)
        assert err <= tol, (lo, n, err)
        lo += n
    print(f"{cfg} scenes {sizes}: {worst:.2e}")


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("sizes", [[1, 2, 15, 16, 17, 31, 33, 64, 65], [0, 3, 0, 4, 0], [2, 300, 2]], ids=["tiles", "empty", "300"])
def test_scene_form_equals_the_restatement(dev, ops, cfg, sizes):
    _check_scenes(ops, dev, cfg, sizes, seed=len(sizes))


@pytest.mark.parametrize("cfg", ["pecnet", "lbebm"])
def test_one_scene_of_1024(dev, ops, cfg):
    _check_scenes(ops, dev, cfg, [1024], seed=7, tol=1e-4)


@pytest.mark.parametrize("cfg", ["lbebm", "lbebm_gen"])
def test_lbebm_rows_do_not_depend_on_their_place(dev, ops, cfg):
    """a row alone, in a call of 100 at positions 0, 15, 16, 99, and in the scene form: identical bits"""
    m, k, S = net(dev, cfg), int(Z[f"{cfg}.k"]), int(Z[f"{cfg}.S"])
    rng = np.random.default_rng(5)
    past, ori = rng.normal(0, 1, (100, k)).astype(np.float32), rng.normal(0, 2, (100, 2)).astype(np.float32)
    whole = predict(m, cfg, dev, past, ori)
    for i in (0, 15, 16, 99):
        assert np.array_equal(predict(m, cfg, dev, past[i:i + 1], ori[i:i + 1]), whole[i:i + 1]), i
    moved = predict(m, cfg, dev, past[::-1], ori[::-1])
    assert np.array_equal(moved[::-1], whole)
    # the scene form on the same rows: obs_ori = nrm - mean is what the call reports; feed THAT to the module form
    sizes = [7, 1, 60, 32]
    nrm = np.vstack([ori.T, np.zeros((2, 100), np.float32)])
    out, det = scenes(ops, m, cfg, dev, past.T, nrm, sizes, want_details=True)
    gin = N_(det["net_inputs"])
    again = predict(m, cfg, dev, gin[:k].T, gin[k:].T)
    assert np.array_equal(N_(out), PN.post_hook(again, S))


@pytest.mark.parametrize("cfg", ["pecnet", "pecnet_gen"])
def test_pecnet_scene_form_equals_module_form_bit_for_bit(dev, ops, cfg):
    m, k, S = net(dev, cfg), int(Z[f"{cfg}.k"]), int(Z[f"{cfg}.S"])
    sizes = [5, 1, 33, 0, 16, 70]
    C_obs, nrm = _synthetic(sum(sizes), 11, k)
    out, det = scenes(ops, m, cfg, dev, C_obs, nrm, sizes, want_details=True)
    out, gin = N_(out), N_(det["net_inputs"])
    lo = 0
    for n in sizes:
        if n:
            u = gin[:, lo:lo + n]
            one = predict(m, cfg, dev, u[:k].T, u[k:].T)
            assert np.array_equal(out[:, lo:lo + n], PN.post_hook(one, S)), (lo, n)
        lo += n


@pytest.mark.parametrize("cfg", ["pecnet", "lbebm"])
def test_a_nan_stays_in_its_scene(dev, ops, cfg):
    m, k = net(dev, cfg), int(Z[f"{cfg}.k"])
    sizes = [9, 20, 1, 18]
    C_obs, nrm = _synthetic(sum(sizes), 13, k)
    clean = N_(scenes(ops, m, cfg, dev, C_obs, nrm, sizes))
    bad = C_obs.copy()
    bad[2, 12] = np.nan  # a pedestrian of the second scene
    got = N_(scenes(ops, m, cfg, dev, bad, nrm, sizes))
    rows = np.ones(sum(sizes), bool)
    if kind(cfg) == "pecnet":
        rows[9:29] = False  # the pooling spreads it over the scene, and no further
        assert np.isnan(got[:, 9:29]).all()
    else:
        rows[12] = False  # every other ROW stays
        assert np.isnan(got[:, 12]).all()
    assert np.array_equal(got[:, rows], clean[:, rows]) and np.isfinite(clean).all()


@pytest.mark.parametrize("cfg", ["pecnet", "pecnet_gen"])
def test_mask_semantics(dev, cfg):
    m = net(dev, cfg)
    past, ori, mask = call_inputs(cfg, "block")
    whole = predict(m, cfg, dev, past, ori, mask)
    lo = 0
    for n in Z["block.sizes"]:
        part = predict(m, cfg, dev, past[lo:lo + n], ori[lo:lo + n])
        err = scale_err(whole[lo:lo + n], part)
        print(f"{cfg} block rows {lo}..{lo + n}: {err:.2e}")
        assert err <= TOL
        lo += n
    for tag in ("block", "zerorow"):
        past, ori, mask = call_inputs(cfg, tag)
        assert mask.dtype == np.bool_
        assert np.array_equal(predict(m, cfg, dev, past, ori, mask), predict(m, cfg, dev, past, ori, mask.astype(np.float32)))
    # an all-zero row takes no part in anybody's pooling but its own: feat + 0
    past, ori, mask = call_inputs(cfg, "zerorow")
    assert not mask[2].any()
    out = predict(m, cfg, dev, past, ori, mask)
    sd = sd_of(cfg)
    feat = np.concatenate([PN.mlp(sd, "encoder_past", past[2:3]), PN.mlp(sd, "encoder_dest", ori[2:3]), ori[2:3]], axis=1)
    assert scale_err(out[2:3], PN.mlp(sd, "predictor", feat)) <= TOL


def wrapper(dev, scene, cfg):
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    hp = default_hyper_params(lr=1e-3, weight_decay=1e-4, static_dist=float(Z[f"{scene}.static_dist"]))
    model = EigenTrajectory(net(dev, cfg), get_hook_func(kind(cfg)), hp)
    sd = model.state_dict()
    for k in sd:
        if k.startswith("ET_"):
            sd[k] = torch.from_numpy(G2[f"{scene}.{k}"])
    model.load_state_dict(sd)
    return model.to(dev).eval()


@pytest.mark.parametrize("cfg", ["pecnet", "lbebm"])
@pytest.mark.parametrize("scene", ["eth", "hotel", "zara1"])
def test_split_end_to_end(dev, scene, cfg):
    """evaluate_split against the reference's per-pedestrian ADE / FDE of every test scene, and against evaluate() scene by
    scene through the hooks with addl_info, every scene"""
    model = wrapper(dev, scene, cfg)
    obs, pred, sse = G.dataset(scene, "test")
    obs, pred, sse = T(obs, dev), T(pred, dev), np.asarray(sse)
    res = model.evaluate_split(obs, pred, sse)
    for key in ("ADE", "FDE"):
        ref = Z[f"{cfg}.{scene}.{key.lower()}"]
        err = scale_err(N_(res[key]), ref)
        print(f"{cfg} {scene} {key}: {err:.2e}")
        assert err <= TOL, key
    worst = 0.0
    for s, e in sse:
        info = {"scene_mask": torch.ones((e - s, e - s), dtype=torch.bool, device=dev), "num_samples": 20}
        ade, fde = model.evaluate(obs[s:e], pred[s:e], addl_info=info)
        for key, val in (("ADE", ade), ("FDE", fde)):
            worst = max(worst, float((res[key][s:e] - val).abs().max() / res[key].abs().max()))
    print(f"{cfg} {scene}: evaluate_split against scene by scene {worst:.2e}")
    assert worst <= TOL


@pytest.mark.parametrize("cfg", ["pecnet_gen", "lbebm_gen"])
def test_weights_in_place_determinism_and_graph_capture(dev, cfg):
    m = fresh(dev, cfg)
    past, ori, _ = call_inputs(cfg, "pick3")
    a = predict(m, cfg, dev, past, ori)
    assert np.array_equal(a, predict(m, cfg, dev, past, ori))
    with torch.no_grad():
        m.predictor.layers[1].bias[3] += 0.5
    b = predict(m, cfg, dev, past, ori)
    assert not np.array_equal(a, b)
    # captured once, replayed after the input changed in place
    p, o = T(past, dev), T(ori, dev)
    n = p.shape[0]
    args = (p, o, torch.ones((n, n), device=dev), o) if kind(cfg) == "pecnet" else (p, o)
    m.predict(*args)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            captured = m.predict(*args)
    p.mul_(0.5)
    o.add_(0.25)
    graph.replay()
    torch.cuda.synchronize()
    eager = m.predict(*args)
    assert torch.equal(captured, eager) and not np.array_equal(N_(eager), b)


def test_empty_inputs_and_unsupported_shapes(dev, ops):
    from eigentrajectory_amd import PECNet
    from eigentrajectory_amd._lib import ETLibraryError
    for cfg in ("pecnet_gen", "lbebm_gen"):
        m, k, S = net(dev, cfg), int(Z[f"{cfg}.k"]), int(Z[f"{cfg}.S"])
        assert predict(m, cfg, dev, np.zeros((0, k), np.float32), np.zeros((0, 2), np.float32)).shape == (0, k * S)
        out, det = scenes(ops, m, cfg, dev, np.zeros((k, 0), np.float32), np.zeros((4, 0), np.float32), [], want_details=True)
        assert out.shape == (k, 0, S) and det["net_inputs"].shape == (k + 2, 0)
        with pytest.raises(ValueError):
            scenes(ops, m, cfg, dev, np.zeros((k, 3), np.float32), np.zeros((4, 3), np.float32), [])
        with pytest.raises(ValueError):
            scenes(ops, m, cfg, dev, np.zeros((k + 1, 3), np.float32), np.zeros((4, 3), np.float32), [3])
    g = [24, 12]
    zeros = lambda *s: torch.zeros(s, device=dev)
    for sizes in ([2048], [8, 8, 8, 8, 8]):  # a width of 2048, five hidden layers
        bad = PECNet(g, g, g, g, sizes, g, g, g, 5, 3, 2, 7, 1.3, 2, 7, False).to(dev).eval()
        with pytest.raises(ETLibraryError, match="status 3"):
            bad.predict(zeros(3, 4), zeros(3, 2), torch.ones((3, 3), device=dev), zeros(3, 2))
        with pytest.raises(ETLibraryError, match="status 3"):
            ops.pecnet_forward_scenes(bad, zeros(4, 3), zeros(4, 3), scene_sizes=[3])
    from eigentrajectory_amd._lib import MLP_MAX_RANGE
    big = MLP_MAX_RANGE + 1  # a scene beyond the pooling range is refused on the host; LBEBM has no such range
    with pytest.raises(ValueError, match="range"):
        ops.pecnet_forward_scenes(net(dev, "pecnet_gen"), zeros(4, big + 2), zeros(4, big + 2), scene_sizes=[2, big])
    with pytest.raises(ValueError, match="range"):
        ops.pecnet_forward_scenes(net(dev, "pecnet_gen"), zeros(4, big), zeros(4, big))
    with pytest.raises(ETLibraryError, match="status 3"):
        net(dev, "pecnet_gen").predict(zeros(big, 4), zeros(big, 2), None, zeros(big, 2))
    assert ops.lbebm_forward_scenes(net(dev, "lbebm_gen"), zeros(4, big), zeros(4, big)).shape == (4, big, 3)
    ok = PECNet(g, g, g, g, [8, 8, 8, 8], g, g, g, 5, 3, 0, 7, 1.3, 2, 7, False).to(dev).eval()  # four hidden, no pooling
    assert ok.predict(zeros(3, 4), zeros(3, 2), None, zeros(3, 2)).shape == (3, 12)
