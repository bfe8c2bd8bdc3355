"""GPU checks of the native GP-Graph-STGCNN predictor (csrc/et_gpgraph_stgcnn.hip through eigentrajectory_amd/gpgraph.py and
ops.py) against the fp64 restatement (tests/_gpgraph_stgcnn_np.py) and the reference's recorded runs
(tests/golden/g22_gpgraph_stgcnn_net.npz).

The restatement of passes 1 and 2 is fed the device's own fp32 inputs (``graph_inputs``: the group means and v' exactly as
the second kernel reads them), which are checked on their own against the bounds fp32 arithmetic gives them
(_gpgraph_stgcnn_np.check_inputs); a recorded output is compared with directly where the reference's own fp32 run is within
1e-6 of its fp64 run, its exact ties are robust and the device's tie pattern is the reference's.

Measured on one MI355X: largest distance error 1.3e-7 of the scene's largest distance (the univ scene of 57), largest
output error against the restatement 4.6e-7 of the largest entry, 11 of the 11 picks compared with the reference's output
directly (largest error 3.8e-7); eth end to end: 178 of 181 pedestrians compared, ADE within 3.3e-7 and FDE within 4.6e-7 of
the split's maximum."""
import ctypes as C

import numpy as np
import pytest
import torch

from . import _golden as G
from . import _gpgraph_np as GN
from . import _gpgraph_stgcnn_np as GS
from . import _sgcn_np as SN
from ._gpu_common import *  # noqa: F401,F403 -- fixtures (dev, ops) and helpers
from .test_gpgraph_stgcnn_cpu import PICKS, Z, direct_picks, et_module, gen_module, net_state

pytestmark = pytest.mark.gpu
RAGGED = (1, 2, 3, 17, 33, 34, 64, 130)   # 33 / 34: the last scene whose arena fits LDS and the first that does not


def net(dev, prefix="net."):
    m = et_module() if prefix == "net." else gen_module()
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in net_state(prefix).items()})
    return m.to(dev).eval()


def run_graph(ops, m, dev, v, v_rel=None):
    """v = v_abs (T, N) numpy, ``v_rel`` (T, N) or None: the same tensor, as the bridge hands it over -> the device's results:
    out (S, k, N), indices, dist, graph_inputs [v_rel, group means, v']"""
    a = T(v[None, None], dev)
    r = a if v_rel is None else T(v_rel[None, None], dev)
    out, idx, det = ops.gpgraph_stgcnn_forward_graph(m, a, r, want_details=True)
    plain, idx2 = m(a, r)  # forward is the graph form; asking for the details changes nothing; runs are bit-identical
    assert torch.equal(plain, out) and torch.equal(idx2, idx) and idx.dtype == torch.int64
    assert det["n_groups"] == int(idx.max()) + 1
    return {"out": N_(out)[0], "indices": N_(idx), "dist": N_(det["dist"]), "gin": [N_(x) for x in det["graph_inputs"]]}


def check(sd, v, got, th=None, v_rel=None):
    """the device's results against the restatement: distances, indices (no undecided pair -> equal), the fp32 bounds on the
    inputs of passes 1 and 2, the output against the restatement fed THOSE inputs -> figures.  v = v_abs (the distances and
    the decisions), ``v_rel`` (pass 0, v' and the group means; None: v_abs); every shape is the inputs' own (T = v.shape[0])"""
    rest = GN.split_state(sd)[1]
    th = GN.threshold(rest) if th is None else th
    rel = v if v_rel is None else v_rel
    own = GS.forward(sd, v, v_rel=v_rel)
    fig = {"n": v.shape[1], "dist_err": GS.rel_err(got["dist"], own["dist"]), "margin": GN.pair_margin(own["dist"], abs(th))}
    assert fig["dist_err"] <= GS.TOL_D, fig
    if fig["margin"] > GS.BAND_D:
        assert np.array_equal(got["indices"], own["indices"]), fig
    assert np.array_equal(got["gin"][0], rel)
    g = int(np.max(got["indices"])) + 1
    assert got["gin"][1].shape == (v.shape[0], g) and got["gin"][2].shape == v.shape
    fig["vprime"], fig["means"] = GS.check_inputs(rel, got["gin"][2], got["gin"][1], got["indices"])
    assert fig["vprime"] <= 1.0 and fig["means"] <= 1.0, fig
    ref = GS.forward(sd, v, inputs=(got["gin"][1], got["gin"][2]), indices=got["indices"], v_rel=v_rel)
    fig["out_err"] = GS.rel_err(got["out"], ref["out"])
    fig["n_groups"] = ref["n_groups"]
    print(f"gpgraph-stgcnn check: {fig}")
    assert fig["out_err"] <= GS.TOL, fig
    return fig


def same_ties(gin, ref):
    return all(a.shape == b.shape and np.array_equal(GS.ties(a), GS.ties(b)) for a, b in zip(gin, ref))


def wrapper(dev, predictor):
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    g2 = G.load("g2_fit_all_scenes.npz")
    hp = default_hyper_params(lr=1e-3, weight_decay=1e-4, static_dist=float(Z["eth.static_dist"]))
    model = EigenTrajectory(predictor, get_hook_func("gpgraphstgcnn"), hp)
    sd = model.state_dict()
    for k in sd:
        if k.startswith("ET_"):
            sd[k] = torch.from_numpy(g2[f"eth.{k}"])
    model.load_state_dict(sd)
    return model.to(dev).eval()


def test_graph_form_on_the_recorded_and_hand_built_scenes(dev, ops):
    m, sd = net(dev), net_state()
    direct, figs = [], []
    for t in PICKS:
        v = Z[f"{t}.v"]
        got = run_graph(ops, m, dev, v)
        figs.append(check(sd, v, got))
        assert np.array_equal(got["indices"], Z[f"{t}.indices"]), t
        assert GS.rel_err(got["dist"], Z[f"{t}.dist"]) <= GS.TOL_D
        if t in direct_picks() and same_ties(got["gin"], [v, Z[f"{t}.v_group"], Z[f"{t}.v_intra"]]):
            err = GS.rel_err(got["out"], Z[f"{t}.out"][0])
            print(f"{t}: against the reference's output directly {err:.3e}")
            assert err <= GS.TOL, (t, err)
            direct.append(t)
    print(f"gpgraph-stgcnn: largest distance error {max(f['dist_err'] for f in figs):.3e}, largest output error "
          f"{max(f['out_err'] for f in figs):.3e}, compared directly {len(direct)} of {len(PICKS)}")
    must = [t for t in PICKS if str(Z[f"{t}.split"]) == "hand" or Z[f"{t}.v"].shape[1] <= 2]
    assert set(must) <= set(direct), (must, direct)


def test_generic_loop_counts(dev, ops):
    m, sd = net(dev, "gen."), net_state("gen.")
    for i in range(2):
        t = str(Z[f"gen.pick{i}"])
        v = Z[f"{t}.v"]
        got = run_graph(ops, m, dev, v)
        assert got["out"].shape == (12, 6, v.shape[1])
        check(sd, v, got)
        assert np.array_equal(got["indices"], Z[f"gen.indices{i}"])
        if same_ties(got["gin"], [v, Z[f"gen.v_group{i}"], Z[f"gen.v_intra{i}"]]):
            assert GS.rel_err(got["out"], Z[f"gen.out{i}"][0]) <= GS.TOL


@pytest.mark.parametrize("n", RAGGED)
def test_ragged_sizes(dev, ops, n):
    m, sd = net(dev), net_state()
    v = SN.synthetic_v(n)
    got = run_graph(ops, m, dev, v)
    fig = check(sd, v, got)
    if n == 1:
        assert got["indices"].tolist() == [0] and got["dist"].shape == (1, 1)
    if n == 34:
        assert fig["n_groups"] <= 33  # the group pass sits in LDS, the other two in the workspace


def test_threshold_extremes_and_th_is_read_in_place(dev, ops):
    m, sd = net(dev), dict(net_state())
    n = 17
    v = SN.synthetic_v(n)
    d = GN.distances(GN.split_state(sd)[1], v)
    low = d[np.tril(np.ones((n, n), bool), -1)]
    outs = {}
    with torch.no_grad():
        for name, th in (("below", 0.5 * low.min()), ("above", 2.0 * low.max())):
            m.group_gen.th.fill_(float(th))  # in place: seen by the next call
            sd["group_gen.th"] = N_(m.group_gen.th)
            got = run_graph(ops, m, dev, v)
            # below: identity indices, the same-group matrix is I, the pass-2 Laplacian I - I = 0 (the restatement's, which
            # the output is compared with); above: one group, pass 1 runs on a single node
            assert got["indices"].tolist() == (list(range(n)) if name == "below" else [0] * n)
            assert got["gin"][1].shape == ((8, n) if name == "below" else (8, 1))
            fig = check(sd, v, got)
            assert fig["n_groups"] == (n if name == "below" else 1) and np.isfinite(got["out"]).all()
            outs[name] = got["out"]
    assert GS.rel_err(outs["below"], outs["above"]) > 1e-3


def test_hook_path_captured_and_replayed_sees_th(dev):
    model = wrapper(dev, net(dev))
    obs, pred, sse = G.dataset("eth", "test")
    obs = T(obs, dev)
    s, e = (int(v) for v in sse[np.argmax(sse[:, 1] - sse[:, 0])])
    o = obs[s:e].contiguous()
    eager = model.forward(o)["recon_traj"].clone()
    rep = model.forward_replayed(o)["recon_traj"].clone()
    assert torch.equal(rep, eager)
    with torch.no_grad():
        model.baseline_model.group_gen.th.fill_(1e-3)  # nobody groups any more; the captured graph reads th on the device
    eager2 = model.forward(o)["recon_traj"].clone()
    rep2 = model.forward_replayed(o)["recon_traj"].clone()
    assert not torch.equal(eager2, eager)
    assert torch.equal(rep2, eager2)


def test_scenes_form(dev, ops):
    model = wrapper(dev, net(dev))
    m = model.baseline_model
    sizes = list(SN.SPLIT_SIZES)
    n_all = sum(sizes)
    C_obs, nrm = SN.synthetic_split(sizes, SN.SPLIT_SEED)
    Cd, nd = T(C_obs, dev), T(nrm, dev)
    Cc, det = ops.gpgraph_stgcnn_forward_scenes(m, Cd, nd, scene_sizes=sizes, want_details=True)
    assert Cc.shape == (6, n_all, 20) and Cc.is_contiguous()
    assert torch.equal(ops.gpgraph_stgcnn_forward_scenes(m, Cd, nd, scene_sizes=sizes), Cc)  # run to run, bit for bit
    Cc, gi, dist, gin = N_(Cc), N_(det["group_index"]), N_(det["dist"]), N_(det["graph_inputs"])
    T_ = m.obs_seq_len  # graph_inputs is (3, T N): pass p of a scene is a (T, n_p) block at T (p N + first row)
    assert gin.shape == (3, T_ * n_all)
    lo = sq = compared = 0
    for i, n in enumerate(sizes):
        # the graph form through the bridge
        o = nd[:2, lo:lo + n] - nd[:2, lo:lo + n].mean(dim=1, keepdim=True)
        net_in = model.hook_func.model_forward_pre_hook(Cd[:, lo:lo + n], o, None)
        ref, idx, d = ops.gpgraph_stgcnn_forward_graph(m, *net_in, want_details=True)
        assert np.array_equal(N_(idx), gi[lo:lo + n]), (lo, n)
        assert int(det["n_groups"][i]) == d["n_groups"]
        assert GS.rel_err(dist[sq:sq + n * n].reshape(n, n), N_(d["dist"])) <= GS.TOL_D
        mine = [gin[p, T_ * lo:T_ * (lo + nm)].reshape(T_, nm) for p, nm in enumerate((n, d["n_groups"], n))]
        if same_ties(mine, [N_(x) for x in d["graph_inputs"]]):
            compared += 1
            assert GS.rel_err(Cc[:, lo:lo + n], N_(ref)[0].transpose(1, 2, 0)) <= GS.TOL, (lo, n)
        else:
            diff = [p for p, (x, y) in enumerate(zip(mine, d["graph_inputs"])) if not same_ties([x], [N_(y)])]
            print(f"scenes form: scene {i} (n = {n}, rows {lo}..) not compared with the graph form: the tie patterns of the "
                  f"inputs of passes {diff} differ; output difference {GS.rel_err(Cc[:, lo:lo + n], N_(ref)[0].transpose(1, 2, 0)):.3e}")
        assert torch.equal(model._predict(Cd[:, lo:lo + n], o, None), ref[0].permute(1, 2, 0))
        lo, sq = lo + n, sq + n * n
    assert compared >= len(sizes) - 1, compared
    # a scene's result does not depend on its neighbours or on the order of the scenes: bit for bit
    order = [3, 0, 6, 5, 1, 4, 2]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    cols = np.concatenate([np.arange(starts[i], starts[i + 1]) for i in order])
    Pc = N_(ops.gpgraph_stgcnn_forward_scenes(m, T(C_obs[:, cols], dev), T(nrm[:, cols], dev),
                                               scene_sizes=[sizes[i] for i in order]))
    assert np.array_equal(Pc, Cc[:, cols])
    lo = sum(sizes[:3])
    alone = N_(ops.gpgraph_stgcnn_forward_scenes(m, Cd[:, lo:lo + 64].contiguous(), nd[:, lo:lo + 64].contiguous()))
    assert np.array_equal(alone, Cc[:, lo:lo + 64])


def test_split_end_to_end(dev):
    """evaluate_split on eth with G2's descriptors and G22's weights against the reference's per-pedestrian ADE / FDE on the
    scenes that are decided, ties_robust and well conditioned in the reference's run; the split means over ALL scenes"""
    model = wrapper(dev, net(dev))
    obs, pred, sse = G.dataset("eth", "test")
    res = model.evaluate_split(T(obs, dev), T(pred, dev), np.asarray(sse))
    good = (Z["eth.margin"] > GS.BAND_D) & Z["eth.ties_robust"] & (Z["eth.cond"] <= GS.COND)
    assert good.mean() >= 0.90
    rows = np.repeat(good, Z["eth.scene_size"])
    for key in ("ADE", "FDE"):
        ref = Z[f"eth.{key.lower()}"]
        got = N_(res[key]).astype(np.float64)
        err = np.abs(got - ref) / np.abs(ref).max()
        print(f"gpgraph-stgcnn eth {key}: compared rows {int(rows.sum())} of {rows.size}, max {err[rows].max():.3e}; other rows "
              f"max {err[~rows].max() if (~rows).any() else 0:.3e}; mean diff {abs(got.mean() - ref.mean(dtype=np.float64)):.3e}")
        assert err[rows].max() <= GS.TOL, (key, float(err[rows].max()))
        assert abs(float(got.mean()) - float(ref.mean(dtype=np.float64))) <= 1e-5


def test_errors_and_empty_inputs(dev, ops):
    from eigentrajectory_amd import _lib as L
    m = net(dev)
    a = T(SN.synthetic_v(3)[None, None], dev)
    good, idx = m(a, a)
    assert good.shape == (1, 20, 6, 3) and torch.isfinite(good).all()
    # N = 0: empty in, empty out
    e = torch.zeros((1, 1, 8, 0), device=dev)
    out, idx0 = m(e, e)
    assert out.shape == (1, 20, 6, 0) and idx0.shape == (0,) and idx0.dtype == torch.int64
    out, det = ops.gpgraph_stgcnn_forward_scenes(m, torch.zeros((6, 0), device=dev), torch.zeros((4, 0), device=dev),
                                                 scene_sizes=[], want_details=True)
    assert out.shape == (6, 0, 20) and sorted(det) == ["dist", "graph_inputs", "group_index", "n_groups"]
    assert det["graph_inputs"].shape == (3, 0) and det["n_groups"].shape == (0,)
    C_obs, nrm = SN.synthetic_split([7], 2)
    x = N_(ops.gpgraph_stgcnn_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=[0, 3, 0, 4, 0]))
    y = N_(ops.gpgraph_stgcnn_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=[3, 4]))
    assert np.array_equal(x, y) and np.isfinite(x).all()
    # a workspace that is too small
    params, _ = m.et_params()
    nbytes = L.lib().et_gpgraph_stgcnn_workspace_bytes(C.byref(params), 3, 9, 1)
    assert nbytes > 0
    ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    out = torch.empty((1, 20, 6, 3), device=dev)
    with pytest.raises(L.ETLibraryError, match="status 4"):
        L.call("et_gpgraph_stgcnn_forward_graph", C.byref(params), L.ptr(a), L.ptr(a), 3, L.ptr(out), None, None, None,
               L.ptr(ws), nbytes - 4, L.stream(dev))
    L.call("et_gpgraph_stgcnn_forward_graph", C.byref(params), L.ptr(a), L.ptr(a), 3, L.ptr(out), None, None, None,
           L.ptr(ws), nbytes, L.stream(dev))
    assert torch.equal(out, good)
    # a scene above ET_SGCN_MAX_N: NaN rows, the other scenes intact
    big = L.SGCN_MAX_N + 1
    C_obs, nrm = SN.synthetic_split([3, big, 4], 5)
    z = N_(ops.gpgraph_stgcnn_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=[3, big, 4]))
    keep = np.r_[0:3, 3 + big:7 + big]
    w = N_(ops.gpgraph_stgcnn_forward_scenes(m, T(C_obs[:, keep], dev), T(nrm[:, keep], dev), scene_sizes=[3, 4]))
    assert np.isnan(z[:, 3:3 + big]).all() and np.array_equal(z[:, keep], w) and np.isfinite(w).all()
    zb = torch.zeros((1, 1, 8, big), device=dev)
    with pytest.raises(ValueError, match="exceeds"):
        m(zb, zb)
    with pytest.raises(ValueError, match="exceeds"):
        ops.gpgraph_stgcnn_forward_scenes(m, torch.zeros((6, big), device=dev), torch.zeros((4, big), device=dev))
    # inputs the kernels read in place: shapes, contiguous, on the model's device
    with pytest.raises(ValueError, match="are not"):
        m(a, torch.zeros((1, 2, 8, 3), device=dev))
    with pytest.raises(ValueError, match="contiguous float32 tensor on"):
        m(a.cpu(), a.cpu())
    with pytest.raises(L.ETLibraryError, match="no CPU path"):
        net("cpu")(a.cpu(), a.cpu())
    with pytest.raises(L.ETLibraryError, match="status 3"):  # outside the native family: the reference's defaults
        from eigentrajectory_amd import get_GPGraph_STGCNN_model
        get_GPGraph_STGCNN_model().to(dev).eval()(a, a)
    with pytest.raises(NotImplementedError, match="SocialSTGCNN base"):
        from .test_gpgraph_cpu import et_module as sgcn_based
        ops.gpgraph_stgcnn_forward_graph(sgcn_based().to(dev).eval(), a, a)
    with pytest.raises(RuntimeError, match="training"):
        net(dev).train()(a, a)
    half = net(dev)
    half.baseline_model.train()  # the wrapper in eval mode, its base put back into training mode
    with pytest.raises(RuntimeError, match="training"):
        half(a, a)
    assert torch.equal(m(a, a)[0], good)  # nothing faulted: the device still answers, bit for bit
