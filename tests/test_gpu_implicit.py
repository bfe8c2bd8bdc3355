"""Native Social-Implicit on the GPU (csrc/et_implicit.hip): the graph form against the reference's recorded network outputs
(tests/golden/g25_implicit.npz), the scene form against the fp64 restatement (tests/_implicit_np.py) fed the fp32 input the
kernel reports, moved bins, the scene form against the graph form through the bridge, whole splits end to end against the
reference's per-pedestrian ADE / FDE, determinism, errors, empty inputs and graph capture.

Measured on the MI355X (figures in DESIGN §4): every comparison below is within its bound."""
import numpy as np
import pytest
import torch

from . import _golden as G
from . import _implicit_np as IN
from ._gpu_common import *  # noqa: F401,F403 -- fixtures (dev, ops) and helpers

pytestmark = pytest.mark.gpu
Z = G.load("g25_implicit.npz")
G2 = G.load("g2_fit_all_scenes.npz")
PICKS = sorted({k.split(".")[0] for k in Z.files if k.startswith("pick")}, key=lambda t: int(t[4:]))
HAND = ["single", "edges", "lonely", "nan"]
GEN = dict(spatial_input=1, spatial_output=12, temporal_input=10, temporal_output=5, bins=[0, 0.5, 2],
           noise_weight=[0.05, 1, 4])
TOL = 1e-5


def state(prefix):
    return {k[len(prefix):]: torch.from_numpy(np.array(Z[k])) for k in Z.files if k.startswith(prefix + "implicit_cells.")}


SD = {k: v.numpy() for k, v in state("net.").items()}


def net(dev, prefix="net.", **kw):
    from eigentrajectory_amd.implicit import SocialImplicitLight
    args = dict(spatial_input=1, spatial_output=20, temporal_input=8, temporal_output=6, bins=[0, 0.01, 0.1, 1.2],
                noise_weight=[0.05, 1, 4, 8])
    args.update(kw)
    m = SocialImplicitLight(**args)
    m.load_state_dict(state(prefix), strict=True)
    return m.to(dev).eval()


def scale_err(got, ref):
    """largest difference over the largest entry; the NaNs must be in the same places"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    return float(np.nanmax(np.abs(got - ref)) / max(np.nanmax(np.abs(ref)), 1e-30))


def wrapper(dev, scene, predictor):
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    hp = default_hyper_params(lr=1e-3, weight_decay=1e-4, static_dist=float(Z[f"{scene}.static_dist"]))
    model = EigenTrajectory(predictor, get_hook_func("implicit"), hp)
    sd = model.state_dict()
    for k in sd:
        if k.startswith("ET_"):
            sd[k] = torch.from_numpy(G2[f"{scene}.{k}"])
    model.load_state_dict(sd)
    return model.to(dev).eval()


def split(scene, dev):
    obs, pred, sse = G.dataset(scene, "test")
    return T(obs, dev), T(pred, dev), np.asarray(sse)


ZONE_RANGE = ((0.001, 0.009), (0.02, 0.09), (0.2, 1.1), (1.3, 3.0))  # inside the default bins' zones


def _with_zones(zone, seed, k=6):
    """coefficients whose first row puts pedestrian i in ``zone[i]`` (either sign), positions around the origin"""
    rng = np.random.default_rng(seed)
    n = len(zone)
    C_obs = rng.normal(0, 1, (k, n)).astype(np.float32)
    lo, hi = np.asarray(ZONE_RANGE, np.float64)[np.asarray(zone, np.int64)].T.reshape(2, n)
    C_obs[0] = (rng.uniform(lo, hi) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    return C_obs, rng.normal(0, 5, (4, n)).astype(np.float32)


def _synthetic(sizes, seed):
    """random zones; around every scene boundary the last two pedestrians of the scene before it and the first two of the
    scene after it share ONE zone, so a neighbour table that looks across a boundary finds a neighbour there"""
    rng = np.random.default_rng(100 + seed)
    zone = rng.integers(0, 4, size=sum(sizes))
    off = np.concatenate([[0], np.cumsum(sizes)])
    for b, at in enumerate(off[1:-1]):
        zone[max(at - 2, 0):at + 2] = b % 4
    return _with_zones(zone, seed)


def _check_scenes(ops, m, C_obs, nrm, sizes, sd=SD, tol=TOL, **fw):
    """the scene form on (C_obs, nrm, sizes) against the restatement fed the returned graph_inputs, the zones exactly;
    graph_inputs itself: the C_obs rows bit for bit, the obs_ori rows within 2 ulp (at the scale of the scene's positions:
    both sides are a fp32 mean in their own summation order, subtracted once) of the numpy fp32 value"""
    dev = next(m.parameters()).device
    out, det = ops.implicit_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=sizes, want_details=True)
    out, gin, zone = N_(out), N_(det["graph_inputs"]), N_(det["zone"])
    k = C_obs.shape[0]
    assert np.array_equal(gin[:k], C_obs) and zone.dtype == np.int32 and zone.shape == (C_obs.shape[1],)
    lo, worst, crossing, ends = 0, 0.0, 0, []
    for n in ([C_obs.shape[1]] if sizes is None else sizes):
        if n == 0:
            continue
        u = gin[:, lo:lo + n]
        ulp = np.spacing(np.abs(nrm[:2, lo:lo + n]).max().astype(np.float32))
        assert np.abs(u[k:].astype(np.float64) - IN.scene_input(C_obs, nrm, lo, lo + n)[k:]).max() <= 2 * ulp, (lo, n)
        z = IN.zones(u, **{key: val for key, val in fw.items() if key == "bins"})
        assert np.array_equal(zone[lo:lo + n], z), (lo, n)
        crossing += bool(ends and ends[-1] == z[0] and z[0] >= 0)
        ends.append(z[-1])
        err = scale_err(out[:, lo:lo + n], IN.c_pred_refine(IN.forward(sd, u, **fw)))
        worst = max(worst, err)
        assert err <= tol, (lo, n, err)
        lo += n
    print(f"scenes {sizes}: {worst:.2e}, boundaries with one zone on both sides {crossing}")
    return out, crossing


def test_graph_form_equals_the_reference(dev):
    """no exclusions: the zones are exact comparisons of the given fp32 v; the NaN scene's NaNs in the same places"""
    m = net(dev)
    for t in PICKS + HAND:
        v = T(Z[f"{t}.v"], dev)
        out = m(v)
        assert out.shape == Z[f"{t}.net_out"].shape
        err = scale_err(N_(out), Z[f"{t}.net_out"])
        print(f"{t} n={v.shape[-1]}: {err:.2e}")
        assert err <= TOL, t
    assert np.isnan(Z["nan.net_out"]).any()
    gen = net(dev, "gen.", **GEN)
    for i in range(2):
        err = scale_err(N_(gen(T(Z[f"gen.v{i}"], dev))), Z[f"gen.net_out{i}"])
        print(f"gen {i}: {err:.2e}")
        assert err <= TOL, i


# the last list: every pedestrian in one zone; two zones alternating; zone 1 with a single member; then a scene that
# starts in the zone the one before it ends in
ZONED = ([7, 8, 7, 5], [3] * 7 + [0, 2] * 4 + [2, 3, 2, 1, 3, 2, 3] + [3, 3, 0, 1, 2])


@pytest.mark.parametrize("sizes", [[1, 2, 3, 63, 64, 65, 130], [0, 3, 0, 4, 0], [2, 1000, 2, 2, 1000, 2], ZONED[0]],
                         ids=["odd", "empties", "ragged", "zoned"])
def test_scene_form_matches_the_restatement(dev, ops, sizes):
    C_obs, nrm = _with_zones(ZONED[1], 4) if sizes is ZONED[0] else _synthetic(sizes, len(sizes))
    _, crossing = _check_scenes(ops, net(dev), C_obs, nrm, sizes)
    assert crossing >= 1  # same-zone pedestrians at the end of one scene and the start of the next


def test_generic_weights_scene_form(dev, ops):
    """S = 12, T = 10, T_out = 5, three bins: nothing in the kernel is tied to the ET shape"""
    gen = net(dev, "gen.", **GEN)
    sd = {k: v.numpy() for k, v in state("gen.").items()}
    sizes = [7, 40, 1]
    rng = np.random.default_rng(5)
    C_obs, nrm = rng.normal(0, 1.5, (8, sum(sizes))).astype(np.float32), rng.normal(0, 5, (4, sum(sizes))).astype(np.float32)
    C_obs[0, 5:9] = [1.0, -1.5, 0.75, -1.25]  # zone 1 on both sides of the first boundary
    C_obs[0, 45:] = [0.25, -0.125, 0.375]     # zone 0 on both sides of the second
    _, crossing = _check_scenes(ops, gen, C_obs, nrm, sizes, sd=sd, bins=GEN["bins"])
    assert crossing == 2


def test_largest_shape_reads_the_weights_in_place(dev, ops):
    """S = 64, T = T_out = 16, 8 bins: 38k floats of weights do not fit LDS next to a pedestrian's planes, so the kernel
    reads them from the module's tensors, three pedestrians to a tile; seeded weights against the restatement"""
    from eigentrajectory_amd.implicit import SocialImplicitLight
    torch.manual_seed(7)
    bins = [0, 0.1, 0.3, 0.6, 1.0, 1.5, 2.0, 2.5]
    big = SocialImplicitLight(spatial_input=1, spatial_output=64, temporal_input=16, temporal_output=16, bins=bins,
                              noise_weight=[1.0] * 8)
    with torch.no_grad():
        for cell in big.implicit_cells:
            cell.global_w.fill_(0.5 + float(torch.rand(1)))
            cell.local_w.fill_(-0.5 - float(torch.rand(1)))
    sd = {k: v.numpy().copy() for k, v in big.state_dict().items()}
    big = big.to(dev).eval()
    sizes = [5, 9, 1]
    rng = np.random.default_rng(11)
    C_obs = rng.normal(0, 1.2, (14, sum(sizes))).astype(np.float32)
    nrm = rng.normal(0, 5, (4, sum(sizes))).astype(np.float32)
    C_obs[0, 3:7] = [0.7, -0.8, 0.9, -0.65]  # zone 3 on both sides of the first boundary (two tiles apart)
    C_obs[0, 12:] = [1.2, -1.1, 1.4]         # zone 4 on both sides of the second
    _, crossing = _check_scenes(ops, big, C_obs, nrm, sizes, sd=sd, bins=bins)
    assert crossing == 2
    v = T(IN.scene_input(C_obs, nrm, 5, 14)[None, None], dev)
    assert scale_err(N_(big(v))[0], IN.forward(sd, N_(v)[0, 0], bins=bins)) <= TOL


def _quarter_grid(n, seed):
    """every coefficient and position a multiple of 0.25; n a power of two, so the scene mean and obs_ori are exact"""
    rng = np.random.default_rng(seed)
    C_obs = (rng.integers(-12, 13, size=(6, n)) * 0.25).astype(np.float32)
    nrm = (rng.integers(-12, 13, size=(4, n)) * 0.25).astype(np.float32)
    return C_obs, nrm


@pytest.mark.parametrize("bins", [[0.25, 0.75, 1.5, 2.5], [0.125, 0.625, 1.125, 2.375]], ids=["on-values", "in-gaps"])
def test_moved_bins(dev, ops, bins):
    """bin values exactly on first coefficients present in the input (such a pedestrian is in the zone the value opens)
    and in the gaps between them; a first coefficient below bins[0] is in no zone and its output is 0"""
    m = net(dev)
    m.bins = bins
    C_obs, nrm = _quarter_grid(64, 3)
    sizes = [32, 32]
    C_obs[0, 30:34] = [1.0, -1.0, -1.0, 1.0]  # on the grid, zone 1 of both bin sets, on both sides of the boundary
    out, crossing = _check_scenes(ops, m, C_obs, nrm, sizes, bins=bins)
    assert crossing == 1
    first = np.abs(C_obs[0])
    assert (first < bins[0]).any() and not out[:, first < bins[0]].any() and out[:, first >= bins[0]].any(axis=(0, 2)).all()
    m.bins = list(IN.BINS)
    assert not np.array_equal(out, N_(ops.implicit_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=sizes)))
    on = [bool((first == np.float32(b)).any()) for b in bins]
    assert all(on) if bins[0] == 0.25 else not any(on)


@pytest.mark.parametrize("scene", G.SCENES)
def test_scene_form_equals_graph_form_through_the_bridge(dev, ops, scene):
    """every scene (every 7th of univ): the whole split's two launches vs the bridge + forward(v) per scene; both see the
    same u"""
    model = wrapper(dev, scene, net(dev))
    obs, pred, sse = split(scene, dev)
    U_obs_m, _, U_obs_s, _ = model._U()
    C_obs, _, nrm, _ = ops.norm_project(obs, None, U_obs_m, None, U_obs_s, None, ops.MODE_SPLIT, model.static_dist,
                                        want_flag=False)
    sizes = (sse[:, 1] - sse[:, 0]).tolist()
    Cc, det = ops.implicit_forward_scenes(model.baseline_model, C_obs, nrm, scene_sizes=sizes, want_details=True)
    gin, k = det["graph_inputs"], C_obs.shape[0]
    assert torch.equal(gin[:k], C_obs)
    errs, same = [], []
    for s, e in sse[::1 if scene != "univ" else 7]:
        ref = model._predict(gin[:k, s:e], gin[k:, s:e], None)
        errs.append((Cc[:, s:e] - ref).abs().max() / ref.abs().max())
        same.append(torch.equal(Cc[:, s:e], ref))
    worst = float(torch.stack(errs).max())
    print(f"{scene}: {len(errs)} scenes, {worst:.2e}, bit-equal {sum(same)}")
    assert worst <= TOL
    assert all(same)  # every pedestrian is the same chain of fmaf over the same five columns in both forms


@pytest.mark.parametrize("scene", G.SCENES)
def test_split_end_to_end(dev, scene):
    """evaluate_split (4 launches) against the reference's per-pedestrian ADE / FDE on the robust scenes (those on which
    an input a few ulp away decides every zone alike, tools/make_golden_implicit.py), the split means over ALL scenes;
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
    """bit for bit, wherever the scene's pedestrians fall in the tiles; two runs agree bit for bit"""
    m = net(dev)
    sizes = [5, 63, 26, 0, 27, 1]
    C_obs, nrm = _synthetic(sizes, 9)
    whole = N_(ops.implicit_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=sizes))
    again = N_(ops.implicit_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=sizes))
    assert np.array_equal(whole, again) and np.isfinite(whole).all()
    lo = 0
    for n in sizes:
        if n:
            c, r = np.ascontiguousarray(C_obs[:, lo:lo + n]), np.ascontiguousarray(nrm[:, lo:lo + n])
            assert np.array_equal(N_(ops.implicit_forward_scenes(m, T(c, dev), T(r, dev))), whole[:, lo:lo + n]), (lo, n)
        lo += n


def test_a_scene_beyond_the_scene_limit_is_not_computed(dev, ops):
    """the neighbour scan is linear in the scene: a scene of more than ET_SCENE_MAX_N pedestrians gets NaN rows and zone -2,
    the scenes around it are computed as if alone"""
    from eigentrajectory_amd._lib import SCENE_MAX_N
    m = net(dev)
    sizes = [3, SCENE_MAX_N + 1, 4]
    zone = np.resize(np.asarray([3, 2, 3, 1, 0, 3], np.int64), sum(sizes))
    C_obs, nrm = _with_zones(zone, 6)
    out, det = ops.implicit_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=sizes, want_details=True)
    out, z = N_(out), N_(det["zone"])
    assert np.isnan(out[:, 3:-4]).all() and (z[3:-4] == -2).all() and np.isnan(N_(det["graph_inputs"])[:, 3:-4]).all()
    for lo, hi in ((0, 3), (sum(sizes) - 4, sum(sizes))):
        c, r = np.ascontiguousarray(C_obs[:, lo:hi]), np.ascontiguousarray(nrm[:, lo:hi])
        assert np.array_equal(N_(ops.implicit_forward_scenes(m, T(c, dev), T(r, dev))), out[:, lo:hi])
        assert np.isfinite(out[:, lo:hi]).all() and np.array_equal(z[lo:hi], zone[lo:hi])
    with pytest.raises(ValueError):  # one scene, no offsets: refused on the host like the graph form
        ops.implicit_forward_scenes(m, T(C_obs, dev), T(nrm, dev))


def test_errors_and_empty_inputs(dev, ops):
    from eigentrajectory_amd._lib import ETLibraryError
    from eigentrajectory_amd.implicit import SocialImplicitLight
    wide = net(dev)
    ET = dict(spatial_input=1, spatial_output=20, temporal_input=8, temporal_output=6)
    bad = SocialImplicitLight(**{**ET, "spatial_output": 65}).to(dev).eval()
    with pytest.raises(ETLibraryError, match="status 3"):
        ops.implicit_forward_graph(bad, torch.zeros((1, 1, 8, 3), device=dev))
    bad = SocialImplicitLight(**{**ET, "temporal_input": 17}).to(dev).eval()
    with pytest.raises(ETLibraryError, match="status 3"):
        ops.implicit_forward_scenes(bad, torch.zeros((15, 3), device=dev), torch.zeros((4, 3), device=dev))
    bad = SocialImplicitLight(**{**ET, "spatial_input": 2}).to(dev).eval()
    with pytest.raises(ETLibraryError, match="status 3"):
        ops.implicit_forward_graph(bad, torch.zeros((1, 1, 8, 3), device=dev))
    bad = net(dev)
    bad.bins = [1.2, 0.1, 0.01, 0]
    with pytest.raises(ETLibraryError, match="status 3"):
        ops.implicit_forward_scenes(bad, torch.zeros((6, 3), device=dev), torch.zeros((4, 3), device=dev))
    with pytest.raises(ValueError):
        ops.implicit_forward_graph(wide, torch.zeros((8, 3), device=dev))
    with pytest.raises(ValueError):
        ops.implicit_forward_scenes(wide, torch.zeros((8, 3), device=dev), torch.zeros((4, 3), device=dev))
    with pytest.raises(ValueError):
        ops.implicit_forward_scenes(wide, torch.zeros((6, 3), device=dev), torch.zeros((4, 3), device=dev), scene_sizes=[2, 2])
    with pytest.raises(RuntimeError, match="training"):
        net(dev).train()(torch.zeros((1, 1, 8, 3), device=dev))
    # no scenes, and empty scenes among others
    out, det = ops.implicit_forward_scenes(wide, torch.zeros((6, 0), device=dev), torch.zeros((4, 0), device=dev),
                                           scene_sizes=[], want_details=True)
    assert out.shape == (6, 0, 20) and det["graph_inputs"].shape == (8, 0) and det["zone"].shape == (0,)
    assert ops.implicit_forward_scenes(wide, torch.zeros((6, 0), device=dev), torch.zeros((4, 0), device=dev)).shape == (6, 0, 20)
    assert wide(torch.zeros((1, 1, 8, 0), device=dev)).shape == (1, 20, 6, 0)
    C_obs, nrm = _synthetic([3, 4], 2)
    a = N_(ops.implicit_forward_scenes(wide, T(C_obs, dev), T(nrm, dev), scene_sizes=[0, 3, 0, 4, 0]))
    b = N_(ops.implicit_forward_scenes(wide, T(C_obs, dev), T(nrm, dev), scene_sizes=[3, 4]))
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
