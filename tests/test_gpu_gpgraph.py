"""Native GP-Graph-SGCN on the GPU (csrc/et_gpgraph.hip).  The network takes two kinds of hard decision -- sigmoid(logit) > 0.5
on every entry of the interaction masks of its three passes, d <= th on every pair of pedestrians -- so every comparison
with the fp64 restatement (tests/_gpgraph_np.py: check_against) has these parts: the device's distances are within 1e-6 of
the scene's largest; without an undecided pair (|d - th| <= 1e-5 th) its group indices are exactly the restatement's; its
logits are within DELTA = 1e-5, outside that band its decisions are the restatement's, the band holds at most 0.5 % of the
scene's entries; and its output equals the restatement run with the device's decisions inside the bands within 1e-5 of the
largest entry.  Checked: the graph form on the reference's recorded and hand-built scenes
(tests/golden/g21_gpgraph_sgcn_net.npz) and on the generic layer counts, ragged sizes, the scenes form (against the graph
form, scene order, run to run), the mask and the threshold read in place (eagerly and replayed), a whole split end to end
against the reference's per-pedestrian ADE / FDE, errors and empty inputs."""
import ctypes as C

import numpy as np
import pytest
import torch

from . import _golden as G
from . import _gpgraph_np as GN
from . import _sgcn_np as SN
from ._gpu_common import *  # noqa: F401,F403 -- fixtures (dev, ops) and helpers
from .test_gpgraph_cpu import PICKS, Z, et_module, gen_module, net_state

pytestmark = pytest.mark.gpu


def net(dev, prefix="net."):
    m = et_module() if prefix == "net." else gen_module()
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in net_state(prefix).items()})
    return m.to(dev).eval()


def scale_err(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def run_graph(ops, m, dev, va, vr):
    """v_abs (T, N), v_rel (2, T, N) as numpy -> the device's results in check_against's form"""
    a, r = T(va[None, None], dev), T(vr[None], dev)
    out, idx, det = ops.gpgraph_sgcn_forward_graph(m, a, r, want_details=True)
    plain, idx2 = m(a, r)  # forward is the graph form; asking for the details changes nothing; runs are bit-identical
    assert torch.equal(plain, out) and torch.equal(idx2, idx) and idx.dtype == torch.int64
    return {"out": N_(out)[0], "indices": N_(idx), "dist": N_(det["dist"]), "logit_s": [N_(x) for x in det["logit_s"]],
            "logit_t": [N_(x) for x in det["logit_t"]]}


def same_decisions(got, t):
    if f"{t}.logit_s0" not in Z.files:
        return False
    return all(np.array_equal(SN.decisions_fp32(got[f"logit_{k}"][m]), SN.decisions_fp32(Z[f"{t}.logit_{k}{m}"]))
               for m in range(3) for k in ("s", "t"))


def wrapper(dev, scene, predictor):
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    g2 = G.load("g2_fit_all_scenes.npz")
    hp = default_hyper_params(lr=1e-3, weight_decay=1e-4, static_dist=float(Z[f"{scene}.static_dist"]))
    model = EigenTrajectory(predictor, get_hook_func("gpgraphsgcn"), hp)
    sd = model.state_dict()
    for k in sd:
        if k.startswith("ET_"):
            sd[k] = torch.from_numpy(g2[f"{scene}.{k}"])
    model.load_state_dict(sd)
    return model.to(dev).eval()


def test_graph_form_on_the_recorded_and_hand_built_scenes(dev, ops):
    m, sd = net(dev), net_state()
    direct = 0
    for t in PICKS:
        va, vr = Z[f"{t}.v_abs"][0, 0], Z[f"{t}.v_rel"][0]
        got = run_graph(ops, m, dev, va, vr)
        fig = GN.check_against(sd, va, vr, got, ref_out=Z[f"{t}.out"][0])
        assert fig["compared"] and not fig["pair_undecided"], t   # none of the recorded scenes has an undecided pair
        assert np.array_equal(got["indices"], Z[f"{t}.indices"]), t
        assert scale_err(got["dist"], Z[f"{t}.dist"]) <= GN.TOL_D
        if same_decisions(got, t):
            direct += 1  # the same decisions as the reference on every entry: its output directly
            assert fig["ref_err"] <= SN.TOL, (t, fig)
    print(f"gpgraph recorded scenes with the reference's decisions on every entry: {direct} of {len(PICKS)}")
    assert direct >= len(PICKS) - 3  # (the large pick's logits are not stored; two picks may carry an undecided entry)


def test_generic_layer_counts(dev, ops):
    m, sd = net(dev, "gen."), net_state("gen.")
    for i in range(2):
        t = str(Z[f"gen.pick{i}"])
        va, vr = Z[f"{t}.v_abs"][0, 0], Z[f"{t}.v_rel"][0]
        got = run_graph(ops, m, dev, va, vr)
        assert got["out"].shape == (12, 6, va.shape[1])
        fig = GN.check_against(sd, va, vr, got, ref_out=Z[f"gen.out{i}"][0])
        assert fig["compared"] and np.array_equal(got["indices"], Z[f"gen.indices{i}"])


@pytest.mark.parametrize("n", SN.RAGGED)
def test_ragged_sizes(dev, ops, n):
    m, sd = net(dev), net_state()
    va, vr = GN.bridge_input(SN.synthetic_v(n))
    got = run_graph(ops, m, dev, va, vr)
    fig = GN.check_against(sd, va, vr, got)
    assert fig["compared"] and not fig["pair_undecided"]
    if n == 1:
        assert got["indices"].tolist() == [0] and got["dist"].shape == (1, 1)


def test_scenes_form(dev, ops):
    model = wrapper(dev, "eth", net(dev))
    m = model.baseline_model
    sizes = list(SN.SPLIT_SIZES)
    n_all, s2 = sum(sizes), sum(s * s for s in sizes)
    C_obs, nrm = SN.synthetic_split(sizes, SN.SPLIT_SEED)
    Cd, nd = T(C_obs, dev), T(nrm, dev)
    Cc, det = ops.gpgraph_sgcn_forward_scenes(m, Cd, nd, scene_sizes=sizes, want_details=True)
    assert Cc.shape == (6, n_all, 20) and Cc.is_contiguous()
    assert torch.equal(ops.gpgraph_sgcn_forward_scenes(m, Cd, nd, scene_sizes=sizes), Cc)  # run to run, bit for bit
    Cc, gi, dist, ls, lt = N_(Cc), N_(det["group_index"]), N_(det["dist"]), N_(det["logit_s"]), N_(det["logit_t"])
    lo = sq = 0
    for n in sizes:
        # the graph form through the bridge: the same decisions wherever the logits agree on them
        o = nd[:2, lo:lo + n] - nd[:2, lo:lo + n].mean(dim=1, keepdim=True)
        net_in = model.hook_func.model_forward_pre_hook(Cd[:, lo:lo + n], o, None)
        ref, idx, d = ops.gpgraph_sgcn_forward_graph(m, *net_in, want_details=True)
        assert np.array_equal(N_(idx), gi[lo:lo + n]), (lo, n)
        assert scale_err(dist[sq:sq + n * n].reshape(n, n), N_(d["dist"])) <= GN.TOL_D
        same = True
        g = d["n_groups"]
        for p, nm in enumerate((n, g, n)):
            a = ls[32 * (p * s2 + sq):32 * (p * s2 + sq + nm * nm)].reshape(8, 4, nm, nm)
            b = lt[256 * (p * n_all + lo):256 * (p * n_all + lo + nm)].reshape(nm, 4, 8, 8)
            assert np.abs(a - N_(d["logit_s"][p])).max() <= SN.DELTA and np.abs(b - N_(d["logit_t"][p])).max() <= SN.DELTA
            same = (same and np.array_equal(SN.decisions_fp32(a), SN.decisions_fp32(N_(d["logit_s"][p])))
                    and np.array_equal(SN.decisions_fp32(b), SN.decisions_fp32(N_(d["logit_t"][p]))))
        if same:
            assert scale_err(Cc[:, lo:lo + n], N_(ref)[0].transpose(1, 2, 0)) <= SN.TOL, (lo, n)
        assert torch.equal(model._predict(Cd[:, lo:lo + n], o, None), ref[0].permute(1, 2, 0))
        lo, sq = lo + n, sq + n * n
    # a scene's result does not depend on its neighbours or on the order of the scenes: bit for bit
    order = [3, 0, 6, 5, 1, 4, 2]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    cols = np.concatenate([np.arange(starts[i], starts[i + 1]) for i in order])
    Pc = N_(ops.gpgraph_sgcn_forward_scenes(m, T(C_obs[:, cols], dev), T(nrm[:, cols], dev),
                                             scene_sizes=[sizes[i] for i in order]))
    assert np.array_equal(Pc, Cc[:, cols])
    lo = sum(sizes[:3])
    alone = N_(ops.gpgraph_sgcn_forward_scenes(m, Cd[:, lo:lo + 64].contiguous(), nd[:, lo:lo + 64].contiguous()))
    assert np.array_equal(alone, Cc[:, lo:lo + 64])


def test_the_mask_matters_and_th_is_read_in_place(dev, ops):
    m = net(dev)
    n = 17
    va, vr = GN.bridge_input(SN.synthetic_v(n))
    a, r = T(va[None, None], dev), T(vr[None], dev)
    d = GN.distances(GN.split_state(net_state())[1], va)
    low = d[np.tril(np.ones((n, n), bool), -1)]
    outs = {}
    with torch.no_grad():
        for name, th in (("below", 0.5 * low.min()), ("above", 2.0 * low.max())):
            m.group_gen.th.fill_(float(th))  # in place: seen by the next call
            outs[name], idx = m(a, r)
            assert N_(idx).tolist() == (list(range(n)) if name == "below" else [0] * n)
    assert scale_err(N_(outs["below"]), N_(outs["above"])) > 1e-3


def test_hook_path_captured_and_replayed_sees_th(dev):
    model = wrapper(dev, "eth", net(dev))
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


def test_split_end_to_end(dev):
    """evaluate_split on eth with G2's descriptors and G21's weights against the reference's per-pedestrian ADE / FDE on the
    scenes without an undecided pair or sigmoid entry in the reference's run; the split means over ALL scenes"""
    scene = "eth"
    model = wrapper(dev, scene, net(dev))
    obs, pred, sse = G.dataset(scene, "test")
    res = model.evaluate_split(T(obs, dev), T(pred, dev), np.asarray(sse))
    decided_scene = (Z[f"{scene}.min_abs_logit"] >= SN.DELTA) & (Z[f"{scene}.margin"] > GN.BAND_D)
    assert decided_scene.mean() >= 0.90
    rows = np.repeat(decided_scene, Z[f"{scene}.scene_size"])
    for key in ("ADE", "FDE"):
        ref = Z[f"{scene}.{key.lower()}"]
        got = N_(res[key]).astype(np.float64)
        err = np.abs(got - ref) / np.abs(ref).max()
        print(f"gpgraph {scene} {key}: decided rows {int(rows.sum())} of {rows.size}, max {err[rows].max():.3e}; undecided rows max "
              f"{err[~rows].max() if (~rows).any() else 0:.3e}; mean diff {abs(got.mean() - ref.mean(dtype=np.float64)):.3e}")
        assert err[rows].max() <= SN.TOL, (key, float(err[rows].max()))
        assert abs(float(got.mean()) - float(ref.mean(dtype=np.float64))) <= 1e-5


def test_errors_and_empty_inputs(dev, ops):
    from eigentrajectory_amd import _lib as L
    m = net(dev)
    va, vr = GN.bridge_input(SN.synthetic_v(3))
    a, r = T(va[None, None], dev), T(vr[None], dev)
    good, idx = m(a, r)
    assert good.shape == (1, 20, 6, 3) and torch.isfinite(good).all()
    # N = 0: empty in, empty out
    out, idx0 = m(torch.zeros((1, 1, 8, 0), device=dev), torch.zeros((1, 2, 8, 0), device=dev))
    assert out.shape == (1, 20, 6, 0) and idx0.shape == (0,) and idx0.dtype == torch.int64
    out = ops.gpgraph_sgcn_forward_scenes(m, torch.zeros((6, 0), device=dev), torch.zeros((4, 0), device=dev), scene_sizes=[])
    assert out.shape == (6, 0, 20)
    C_obs, nrm = SN.synthetic_split([7], 2)
    x = N_(ops.gpgraph_sgcn_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=[0, 3, 0, 4, 0]))
    y = N_(ops.gpgraph_sgcn_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=[3, 4]))
    assert np.array_equal(x, y) and np.isfinite(x).all()
    # a workspace that is too small
    params, _ = m.et_params()
    nbytes = L.lib().et_gpgraph_sgcn_workspace_bytes(C.byref(params), 3, 9, 1)
    assert nbytes > 0
    ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    out = torch.empty((1, 20, 6, 3), device=dev)
    with pytest.raises(L.ETLibraryError, match="status 4"):
        L.call("et_gpgraph_sgcn_forward_graph", C.byref(params), L.ptr(a), L.ptr(r), 3, L.ptr(out), None, None, None, None,
               L.ptr(ws), nbytes - 4, L.stream(dev))
    L.call("et_gpgraph_sgcn_forward_graph", C.byref(params), L.ptr(a), L.ptr(r), 3, L.ptr(out), None, None, None, None,
           L.ptr(ws), nbytes, L.stream(dev))
    assert torch.equal(out, good)
    # a scene above ET_SGCN_MAX_N: NaN rows, the other scenes intact
    big = L.SGCN_MAX_N + 1
    C_obs, nrm = SN.synthetic_split([3, big, 4], 5)
    z = N_(ops.gpgraph_sgcn_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=[3, big, 4]))
    keep = np.r_[0:3, 3 + big:7 + big]
    w = N_(ops.gpgraph_sgcn_forward_scenes(m, T(C_obs[:, keep], dev), T(nrm[:, keep], dev), scene_sizes=[3, 4]))
    assert np.isnan(z[:, 3:3 + big]).all() and np.array_equal(z[:, keep], w) and np.isfinite(w).all()
    with pytest.raises(ValueError, match="exceeds"):
        m(torch.zeros((1, 1, 8, big), device=dev), torch.zeros((1, 2, 8, big), device=dev))
    with pytest.raises(ValueError, match="exceeds"):
        ops.gpgraph_sgcn_forward_scenes(m, torch.zeros((6, big), device=dev), torch.zeros((4, big), device=dev))
    # inputs the kernels read in place: shapes, contiguous, on the model's device
    with pytest.raises(ValueError, match="are not"):
        m(a, a)
    with pytest.raises(ValueError, match="contiguous float32 tensor on"):
        m(a.cpu(), r.cpu())
    with pytest.raises(L.ETLibraryError, match="no CPU path"):
        net("cpu")(a.cpu(), r.cpu())
    with pytest.raises(L.ETLibraryError, match="status 3"):  # outside the native family: the reference's defaults
        from eigentrajectory_amd import get_GPGraph_SGCN_model
        get_GPGraph_SGCN_model().to(dev).eval()(a, r)
    with pytest.raises(RuntimeError, match="training"):
        net(dev).train()(a, r)
    assert torch.equal(m(a, r)[0], good)  # nothing faulted: the device still answers, bit for bit
