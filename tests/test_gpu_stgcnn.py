"""Native Social-STGCNN on the GPU (csrc/et_stgcnn.hip): the graph form against the reference's recorded network outputs
(tests/golden/g19_stgcnn.npz), the scene form against the graph form through the bridge, whole splits end to end against
the reference's per-pedestrian ADE / FDE, large scenes (workspace path) against tests/_stgcnn_np.py, the generic loop
structure, errors, empty inputs and graph capture.

Below those: the kernels across layer counts, widths and arena edges (the configurations of tests/_stgcnn_np.py: CONFIGS,
seeded weights with nothing left at its default) against the fp64 restatement -- the scene form in LDS and in the workspace
in one launch on inputs whose scene mean is exact (SN.exact_split), any order of scenes and a scene alone bit for bit, the
graph form with a non-symmetric a, the recorded generic calls of g19b_stgcnn_generic.npz, another BatchNorm eps, a NaN that
stays in its scene, a scene beyond the scene limit, and every limit accepted and refused.  Every comparison is within TOL
of the largest entry, no scene or row excluded; the largest errors measured on the MI355X are in DESIGN §4."""
import ctypes as C

import numpy as np
import pytest
import torch

from . import _golden as G
from . import _stgcnn_np as SN
from ._gpu_common import *  # noqa: F401,F403 -- fixtures (dev, ops) and helpers

pytestmark = pytest.mark.gpu
Z = G.load("g19_stgcnn.npz")
PICKS = sorted({k.split(".")[0] for k in Z.files if k.startswith("pick")}, key=lambda t: int(t[4:]))
TOL = 1e-5
# end to end against the reference: rows of each split whose ADE / FDE differ by more than TOL of the split's
# maximum, and the largest such difference, as measured on the MI355X
BEYOND = {"eth": {"ADE": 0, "FDE": 0}, "hotel": {"ADE": 1, "FDE": 5}, "univ": {"ADE": 417, "FDE": 685},
          "zara1": {"ADE": 0, "FDE": 2}, "zara2": {"ADE": 1319, "FDE": 1384}}
MAX_REL = {"eth": TOL, "hotel": 3e-5, "univ": 1e-3, "zara1": 2e-5, "zara2": 2.5e-2}


def state(prefix):
    return {k[len(prefix):]: torch.from_numpy(np.array(Z[k])) for k in Z.files
            if k.startswith(prefix) and not k[len(prefix):].startswith("net_out")}


def net(dev, prefix="net.", **kw):
    from eigentrajectory_amd.stgcnn import SocialSTGCNN
    args = dict(n_stgcnn=1, n_txpcnn=5, input_feat=1, output_feat=20, seq_len=8, pred_seq_len=6, kernel_size=3)
    args.update(kw)
    m = SocialSTGCNN(**args)
    m.load_state_dict(state(prefix))
    return m.to(dev).eval()


def scale_err(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def wrapper(dev, scene, predictor):
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    hp = default_hyper_params(lr=1e-3, weight_decay=1e-4, static_dist=float(Z[f"{scene}.static_dist"]))
    model = EigenTrajectory(predictor, get_hook_func("stgcnn"), hp)
    sd = model.state_dict()
    for k in sd:
        if k.startswith("ET_"):
            sd[k] = torch.from_numpy(Z[f"{scene}.ET.{k}"])
    model.load_state_dict(sd)
    return model.to(dev).eval()


def split(scene, dev):
    obs, pred, sse = G.dataset(scene, "test")
    return T(obs, dev), T(pred, dev), np.asarray(sse)


def test_graph_form_equals_the_reference(dev):
    m = net(dev)
    for t in PICKS:
        out = m(T(Z[f"{t}.v"], dev), T(Z[f"{t}.a"], dev))
        assert out.shape == Z[f"{t}.net_out"].shape
        assert scale_err(N_(out), Z[f"{t}.net_out"]) <= TOL, t


def test_generic_weights_equal_the_reference(dev):
    m = net(dev, "gen.", n_stgcnn=2, n_txpcnn=3, output_feat=12)
    for i, t in enumerate(PICKS[:2]):
        out = m(T(Z[f"{t}.v"], dev), T(Z[f"{t}.a"], dev))
        assert scale_err(N_(out), Z[f"gen.net_out{i}"]) <= TOL


@pytest.mark.parametrize("scene", G.SCENES)
def test_split_end_to_end(dev, ops, scene):
    """evaluate_split (3 launches) against the reference's per-pedestrian ADE / FDE; the scene form against the graph
    form called scene by scene through the bridge; ETTrainer.test's default per-scene path gives the same means."""
    model = wrapper(dev, scene, net(dev))
    obs, pred, sse = split(scene, dev)
    res = model.evaluate_split(obs, pred, sse)
    for key in ("ADE", "FDE"):  # rows beyond 1e-5 of the split's max, measured (inverse-distance kernel)
        ref = Z[f"{scene}.{key.lower()}"]
        err = np.abs(N_(res[key]).astype(np.float64) - ref) / np.abs(ref).max()
        assert int((err > TOL).sum()) <= BEYOND[scene][key], (key, int((err > TOL).sum()))
        assert err.max() <= MAX_REL[scene], (key, float(err.max()))
        assert abs(float(N_(res[key]).mean(dtype=np.float64)) - float(ref.mean(dtype=np.float64))) <= 3e-4
    # scene form vs graph form through the bridge (the adjacency computed vs read)
    U_obs_m, _, U_obs_s, _ = model._U()
    C_obs, _, nrm, _ = ops.norm_project(obs, None, U_obs_m, None, U_obs_s, None, ops.MODE_SPLIT, model.static_dist,
                                        want_flag=False)
    sizes = (sse[:, 1] - sse[:, 0]).tolist()
    Cc = N_(ops.stgcnn_forward_scenes(model.baseline_model, C_obs, nrm, scene_sizes=sizes))
    step = 1 if scene != "univ" else 7
    for s, e in sse[::step]:
        o = nrm[:2, s:e] - nrm[:2, s:e].mean(dim=1, keepdim=True)
        ref = model._predict(C_obs[:, s:e], o, None)
        assert scale_err(Cc[:, s:e], N_(ref)) <= TOL, (s, e)
    if scene in ("eth", "hotel"):
        from eigentrajectory_amd.data import TrajectoryData
        from eigentrajectory_amd.trainer import ETTrainer
        data = TrajectoryData.from_arrays(N_(obs), N_(pred), sse)
        tr = ETTrainer(model, model.hyper_params, data, data, data, mode="sequenced", device=dev)
        means = tr.test()
        assert abs(means["ADE"] - float(Z[f"{scene}.ade"].mean(dtype=np.float64))) <= 1e-5
        assert abs(means["FDE"] - float(Z[f"{scene}.fde"].mean(dtype=np.float64))) <= 1e-5


def _synthetic(n, seed, k=6):
    rng = np.random.default_rng(seed)
    C_obs = rng.normal(0, 1, (k, n)).astype(np.float32)
    C_obs[:, : n // 8] = np.round(C_obs[:, : n // 8], 1)  # coincident values in every row
    nrm = rng.normal(0, 5, (4, n)).astype(np.float32)
    return C_obs, nrm


def test_large_scenes_match_numpy(dev, ops):
    m = net(dev)
    sd = {k: v.numpy() for k, v in state("net.").items()}
    C_obs, nrm = _synthetic(4096, 0)
    out = N_(ops.stgcnn_forward_scenes(m, T(C_obs, dev), T(nrm, dev)))
    ref = SN.c_pred_refine(SN.forward(sd, SN.scene_input(C_obs, nrm, 0, 4096)))
    assert scale_err(out, ref) <= 1e-4  # fp32 sums over 4 096 pedestrians against fp64 (2.9e-5 measured)
    sizes = [2, 1000, 2, 2, 1000, 2]
    C_obs, nrm = _synthetic(sum(sizes), 1)
    out = N_(ops.stgcnn_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=sizes))
    lo = 0
    for n in sizes:
        ref = SN.c_pred_refine(SN.forward(sd, SN.scene_input(C_obs, nrm, lo, lo + n)))
        assert scale_err(out[:, lo:lo + n], ref) <= TOL, (lo, n)
        lo += n


def test_errors_and_empty_inputs(dev, ops):
    from eigentrajectory_amd._lib import ETLibraryError
    from eigentrajectory_amd.stgcnn import SocialSTGCNN
    wide = net(dev)
    bad = SocialSTGCNN(n_stgcnn=1, n_txpcnn=5, input_feat=1, output_feat=65, seq_len=8, pred_seq_len=6).to(dev).eval()
    with pytest.raises(ETLibraryError, match="status 3"):
        ops.stgcnn_forward_graph(bad, torch.zeros((1, 1, 8, 3), device=dev), torch.zeros((8, 3, 3), device=dev))
    bad = SocialSTGCNN(n_stgcnn=1, n_txpcnn=5, input_feat=1, output_feat=20, seq_len=9, pred_seq_len=6).to(dev).eval()
    with pytest.raises(ETLibraryError, match="status 3"):
        ops.stgcnn_forward_scenes(bad, torch.zeros((6, 3), device=dev), torch.zeros((4, 3), device=dev))
    # no scenes, and empty scenes among others
    out = ops.stgcnn_forward_scenes(wide, torch.zeros((6, 0), device=dev), torch.zeros((4, 0), device=dev), scene_sizes=[])
    assert out.shape == (6, 0, 20)
    C_obs, nrm = _synthetic(7, 2)
    a = N_(ops.stgcnn_forward_scenes(wide, T(C_obs, dev), T(nrm, dev), scene_sizes=[0, 3, 0, 4, 0]))
    b = N_(ops.stgcnn_forward_scenes(wide, T(C_obs, dev), T(nrm, dev), scene_sizes=[3, 4]))
    assert np.array_equal(a, b) and np.isfinite(a).all()


def test_hook_path_captured_and_replayed(dev):
    model = wrapper(dev, "eth", net(dev))
    obs, pred, sse = split("eth", dev)
    s, e = (int(v) for v in sse[np.argmax(sse[:, 1] - sse[:, 0])])
    o = obs[s:e].contiguous()
    eager = model.forward(o)["recon_traj"].clone()
    rep = model.forward_replayed(o)["recon_traj"].clone()
    assert torch.equal(rep, eager)
    new = {k: v + 0.05 * torch.randn_like(v) if v.is_floating_point() and "running_var" not in k else v
           for k, v in model.baseline_model.state_dict().items()}
    model.baseline_model.load_state_dict(new)  # in place: the captured graph sees the new weights
    eager2 = model.forward(o)["recon_traj"].clone()
    rep2 = model.forward_replayed(o)["recon_traj"].clone()
    assert not torch.equal(eager2, eager)
    assert torch.equal(rep2, eager2)


# ------------------------------------------------------------------ layer counts, widths and arena edges
ZB = G.load("g19b_stgcnn_generic.npz")
CFG = SN.CONFIGS
_NETS, _REFS = {}, {}


def gnet(dev, name, eps=None):
    """-> (module on the GPU, its state_dict as numpy): configuration `name` with SN.random_state's weights (seed 0), every
    BatchNorm's eps set to `eps` if given.  Shared between the tests, which leave it unchanged."""
    if (name, eps) not in _NETS:
        from eigentrajectory_amd.stgcnn import SocialSTGCNN
        m = SocialSTGCNN(**SN.module_kw(*CFG[name]))
        sd = SN.random_state(m, 0)
        for bn in m.modules():
            if eps is not None and isinstance(bn, torch.nn.BatchNorm2d):
                bn.eps = eps
        _NETS[name, eps] = (m.to(dev).eval(), sd)
    return _NETS[name, eps]


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def scene_refs(name, sd, C_obs, nrm, sizes, key=None, **fw):
    """the fp64 restatement of every non-empty scene of a split (None for an empty one), computed once per `key`"""
    if key is None or (name, key) not in _REFS:
        n_st, n_tp = CFG[name][:2]
        off = offsets(sizes)
        refs = [SN.c_pred_refine(SN.forward(sd, SN.scene_input(C_obs, nrm, off[i], off[i + 1]), n_stgcnn=n_st,
                                            n_txpcnn=n_tp, **fw)) if n else None for i, n in enumerate(sizes)]
        if key is None:
            return refs
        _REFS[name, key] = refs
    return _REFS[name, key]


def run_scenes(ops, m, dev, C_obs, nrm, sizes):
    return N_(ops.stgcnn_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=sizes))


def run_alone(ops, m, dev, C_obs, nrm, lo, hi):
    c, r = np.ascontiguousarray(C_obs[:, lo:hi]), np.ascontiguousarray(nrm[:, lo:hi])
    return N_(ops.stgcnn_forward_scenes(m, T(c, dev), T(r, dev)))


@pytest.mark.parametrize("name", list(CFG))
def test_arena_arithmetic_agrees_with_the_library(dev, name):
    """tests/_stgcnn_np.py restates the arena formula; the library takes no workspace up to the LDS limit and 4 per N bytes
    one pedestrian above it"""
    from eigentrajectory_amd import _lib as L
    per, lim = SN.arena_per_ped(*CFG[name]), SN.lds_max_n(*CFG[name])
    assert (per, lim) == SN.ARENA[name]
    p, _ = gnet(dev, name)[0].et_params()
    N = 3 * lim + 7
    assert L.lib().et_stgcnn_workspace_bytes(C.byref(p), L.i64(N), L.i64(lim)) == 0
    assert L.lib().et_stgcnn_workspace_bytes(C.byref(p), L.i64(N), L.i64(lim + 1)) == 4 * per * N


@pytest.mark.parametrize("name", list(CFG))
def test_scene_form_matches_the_restatement_in_both_arenas(dev, ops, name):
    """one launch over scenes of 1, 2, 3, L-1, L, L+1, 0, 2L+5 and 2 pedestrians (L the LDS limit; `max`: up to 17), LDS
    and workspace scenes side by side, every scene against the fp64 restatement fed exactly the same input; the scenes in
    another order, and each scene alone, give the same bits"""
    n_st, n_tp, S, k = CFG[name]
    m, sd = gnet(dev, name)
    sizes = SN.split_sizes(name)
    off = offsets(sizes)
    C_obs, nrm = SN.exact_split(sizes, k, 1)
    refs = scene_refs(name, sd, C_obs, nrm, sizes, key="split")
    out = run_scenes(ops, m, dev, C_obs, nrm, sizes)
    assert out.shape == (k, off[-1], S)
    errs = {(i, n): scale_err(out[:, off[i]:off[i + 1]], refs[i]) for i, n in enumerate(sizes) if n}
    print(f"{name} scene form, (scene, n): error {({key: float(f'{e:.2e}') for key, e in errs.items()})}")
    print(f"{name} scene form: largest error {max(errs.values()):.2e}")
    assert np.isfinite(out).all() and max(errs.values()) <= TOL, errs
    order = list(range(len(sizes)))[::-1]
    order[1], order[3] = order[3], order[1]
    cols = np.concatenate([np.arange(off[i], off[i + 1]) for i in order])
    moved = run_scenes(ops, m, dev, C_obs[:, cols], nrm[:, cols], [sizes[i] for i in order])
    assert np.array_equal(moved, out[:, cols])  # column for column
    for i, n in enumerate(sizes):
        if n:
            assert np.array_equal(run_alone(ops, m, dev, C_obs, nrm, off[i], off[i + 1]), out[:, off[i]:off[i + 1]]), (i, n)


@pytest.mark.parametrize("name", ["et", "gen", "tp1"])
def test_graph_form_takes_any_adjacency_in_both_arenas(dev, name):
    """a dense non-symmetric normal a at n = 1, L, L+1 and 70; with a transposed over its last two axes the output is the
    restatement's of THAT a and far from the first (n = 1 has nothing to transpose)"""
    n_st, n_tp, S, k = CFG[name]
    m, sd = gnet(dev, name)
    lim = SN.lds_max_n(*CFG[name])
    rng = np.random.default_rng(17)
    errs = {}
    for n in (1, lim, lim + 1, 70):
        v = rng.normal(0, 1, (1, 1, k + 2, n)).astype(np.float32)
        a = rng.normal(0, 1, (k + 2, n, n)).astype(np.float32)
        at = np.ascontiguousarray(np.swapaxes(a, 1, 2))
        out, out_t = N_(m(T(v, dev), T(a, dev))), N_(m(T(v, dev), T(at, dev)))
        assert out.shape == (1, S, k, n)
        ref, ref_t = (SN.forward(sd, v[0, 0], x, n_stgcnn=n_st, n_txpcnn=n_tp) for x in (a, at))
        errs[n] = (scale_err(out[0], ref), scale_err(out_t[0], ref_t), scale_err(out_t[0], ref))
    print(f"{name} graph form, n: (error, error with a transposed, change by transposing) "
          f"{({n: tuple(float(f'{e:.2e}') for e in es) for n, es in errs.items()})}")
    print(f"{name} graph form: largest error {max(max(es[:2]) for es in errs.values()):.2e}")
    for n, (err, err_t, change) in errs.items():
        assert err <= TOL and err_t <= TOL, (n, err, err_t)
        assert n == 1 or change > 1e-3, (n, change)


def test_recorded_generic_calls_through_the_module(dev):
    """g19b: n_txpcnn = 1, 2, 8, three and eight st_gcn layers, k = 1; the bridge's a and a non-symmetric one; against the
    reference's float64 output and its float32 output"""
    from eigentrajectory_amd.stgcnn import SocialSTGCNN
    worst = {}
    for i in range(4):
        cfg = tuple(int(c) for c in ZB[f"c{i}.cfg"])
        pre = f"c{i}.sd."
        m = SocialSTGCNN(**SN.module_kw(*cfg))
        m.load_state_dict({key[len(pre):]: torch.from_numpy(np.array(ZB[key])) for key in ZB.files if key.startswith(pre)})
        m = m.to(dev).eval()
        for call in ("s3", "s11", "ns"):
            out = N_(m(T(ZB[f"c{i}.{call}.v"], dev), T(ZB[f"c{i}.{call}.a"], dev)))
            assert out.shape == ZB[f"c{i}.{call}.out"].shape
            worst[cfg, call] = (scale_err(out, ZB[f"c{i}.{call}.out64"]), scale_err(out, ZB[f"c{i}.{call}.out"]))
    print("g19b (float64 reference, float32 reference): "
          f"{({key: tuple(float(f'{e:.2e}') for e in es) for key, es in worst.items()})}")
    print(f"g19b: largest error {max(max(es) for es in worst.values()):.2e}")
    assert all(max(es) <= TOL for es in worst.values()), worst


def test_batchnorm_eps_is_read_from_the_module(dev, ops):
    name, eps = "gen", 1e-3
    m, sd = gnet(dev, name, eps=eps)
    lim = SN.lds_max_n(*CFG[name])
    sizes = [3, lim, lim + 1]
    off = offsets(sizes)
    C_obs, nrm = SN.exact_split(sizes, CFG[name][3], 2)
    out = run_scenes(ops, m, dev, C_obs, nrm, sizes)
    refs = scene_refs(name, sd, C_obs, nrm, sizes, eps=eps)
    errs = [scale_err(out[:, off[i]:off[i + 1]], refs[i]) for i in range(len(sizes))]
    usual = run_scenes(ops, gnet(dev, name)[0], dev, C_obs, nrm, sizes)
    print(f"{name} eps {eps}: errors {[float(f'{e:.2e}') for e in errs]}, from the eps 1e-5 result {scale_err(out, usual):.2e}")
    assert max(errs) <= TOL
    assert scale_err(out, usual) > 10 * TOL


@pytest.mark.parametrize("poisoned", ["lds", "workspace"])
@pytest.mark.parametrize("name", ["et", "gen"])
def test_a_nan_stays_in_its_scene(dev, ops, name, poisoned):
    """an LDS scene and a workspace scene on either side of a scene with one NaN coefficient: they are what they are
    without the NaN, bit for bit; the poisoned scene is NaN where the restatement of the same input is"""
    m, sd = gnet(dev, name)
    lim = SN.lds_max_n(*CFG[name])
    sizes = [5, lim + 1, 7 if poisoned == "lds" else lim + 2, 4, lim + 3]
    off = offsets(sizes)
    C_obs, nrm = SN.exact_split(sizes, CFG[name][3], 3)
    clean = run_scenes(ops, m, dev, C_obs, nrm, sizes)
    bad = C_obs.copy()
    bad[2, off[2] + 1] = np.nan
    out = run_scenes(ops, m, dev, bad, nrm, sizes)
    assert np.isfinite(clean).all()
    for i in (0, 1, 3, 4):
        assert np.array_equal(out[:, off[i]:off[i + 1]], clean[:, off[i]:off[i + 1]]), i
    with np.errstate(invalid="ignore"):
        ref = SN.c_pred_refine(SN.forward(sd, SN.scene_input(bad, nrm, off[2], off[3]), n_stgcnn=CFG[name][0],
                                          n_txpcnn=CFG[name][1]))
    assert np.isnan(ref).any()
    assert np.array_equal(np.isnan(out[:, off[2]:off[3]]), np.isnan(ref))


def test_a_scene_beyond_the_scene_limit_is_not_computed(dev, ops):
    """a scene of more than ET_SCENE_MAX_N pedestrians gets NaN columns, the scenes around it are computed as if alone; the
    same rows as ONE scene without offsets are refused.  A scene that fits neither LDS nor the workspace given (here: none)
    takes the same branch."""
    from eigentrajectory_amd import _lib as L
    m, _ = gnet(dev, "et")
    sizes = [3, L.SCENE_MAX_N + 1, 4]
    C_obs, nrm = _synthetic(sum(sizes), 6)
    out = run_scenes(ops, m, dev, C_obs, nrm, sizes)
    assert np.isnan(out[:, 3:-4]).all()
    for lo, hi in ((0, 3), (sum(sizes) - 4, sum(sizes))):
        assert np.array_equal(run_alone(ops, m, dev, C_obs, nrm, lo, hi), out[:, lo:hi]) and np.isfinite(out[:, lo:hi]).all()
    with pytest.raises(ValueError):
        ops.stgcnn_forward_scenes(m, T(C_obs, dev), T(nrm, dev))
    lim = SN.lds_max_n(*CFG["et"])
    sizes = [3, lim + 1, lim]
    C_obs, nrm = _synthetic(sum(sizes), 7)
    whole = run_scenes(ops, m, dev, C_obs, nrm, sizes)
    p, _ = m.et_params()
    c, r, off = T(C_obs, dev), T(nrm, dev), ops.scene_offsets(sizes, sum(sizes), dev)
    got = torch.full((6, sum(sizes), 20), 7.0, device=dev)
    L.call("et_stgcnn_forward_scenes", C.byref(p), L.ptr(c), L.ptr(r), sum(sizes), L.ptr(off), len(sizes), L.ptr(got), None, 0,
           L.stream(dev))
    got = N_(got)
    assert np.isnan(got[:, 3:3 + lim + 1]).all()
    assert np.array_equal(got[:, :3], whole[:, :3]) and np.array_equal(got[:, -lim:], whole[:, -lim:])


REFUSED = {"S = 65": dict(output_feat=65), "k = 33": dict(pred_seq_len=33, seq_len=35), "n_stgcnn = 9": dict(n_stgcnn=9),
           "n_txpcnn = 9": dict(n_txpcnn=9), "seq_len != k + 2": dict(seq_len=7), "input_feat = 2": dict(input_feat=2),
           "kernel_size = 5": dict(kernel_size=5)}


def test_limits_refused(dev, ops):
    """one step outside each limit of the family (the accepted side: `wide`, `max`, `deep_tp`, `deep_st` above): status 3;
    BatchNorms that disagree on eps, a module on the CPU, and a workspace that is missing or short"""
    from eigentrajectory_amd import _lib as L
    from eigentrajectory_amd.stgcnn import SocialSTGCNN
    for what, kw in REFUSED.items():
        args = dict(SN.module_kw(*CFG["et"]), **kw)
        bad = SocialSTGCNN(**args).to(dev).eval()
        K = args["seq_len"]
        with pytest.raises(L.ETLibraryError, match="status 3"):
            ops.stgcnn_forward_graph(bad, torch.zeros((1, 1, K, 3), device=dev), torch.zeros((K, 3, 3), device=dev))
    v, a = torch.zeros((1, 1, 8, 3), device=dev), torch.zeros((8, 3, 3), device=dev)
    two = SocialSTGCNN(**SN.module_kw(*CFG["et"])).to(dev).eval()
    two.st_gcns[0].tcn[3].eps = 1e-3
    with pytest.raises(L.ETLibraryError, match="eps"):
        two(v, a)
    with pytest.raises(L.ETLibraryError, match="HIP"):
        SocialSTGCNN(**SN.module_kw(*CFG["et"])).eval()(v.cpu(), a.cpu())
    m, _ = gnet(dev, "et")
    p, _ = m.et_params()
    n = SN.lds_max_n(*CFG["et"]) + 1
    v, a = torch.zeros((1, 1, 8, n), device=dev), torch.zeros((8, n, n), device=dev)
    out = torch.full((1, 20, 6, n), 7.0, device=dev)
    short = torch.empty((4 * SN.arena_per_ped(*CFG["et"]) * n - 4,), device=dev, dtype=torch.uint8)
    for ws in (None, short):
        rc = L.lib().et_stgcnn_forward_graph(C.byref(p), L.ptr(v), L.ptr(a), n, L.ptr(out), L.ptr(ws),
                                             0 if ws is None else ws.numel(), L.stream(dev))
        assert rc == 4  # ET_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing was launched
