"""Native SGCN on the GPU (csrc/et_sgcn.hip).  The network takes a hard decision, sigmoid(logit) > 0.5, on every entry of
its interaction masks, so every comparison with the fp64 restatement (tests/_sgcn_np.py: check_against) has three parts:
(a) the device's logits are within DELTA = 1e-5 of the restatement's, (b) outside that band the device's decisions equal
the restatement's, (c) the device's output equals the restatement run with the device's decisions inside the band, within
1e-5 of the largest entry -- and the band may hold at most 0.5 % of a scene's entries (1e-4 of a split's).  Checked: the
graph form on the reference's recorded scenes (tests/golden/g20_sgcn_net.npz) and on the generic layer counts, the
identities' broadcast forms, ragged sizes, the scenes form, whole splits end to end against the reference's
per-pedestrian ADE / FDE, the hook path eagerly and replayed, errors and empty inputs.
Other members of the family (T from 3 to 34, 1 to 8 layers, S 1 to 64, scenes up to 512, 300 scenes): tests/test_gpu_sgcn_shapes.py."""
import numpy as np
import pytest
import torch

from . import _golden as G
from . import _sgcn_np as SN
from ._gpu_common import *  # noqa: F401,F403 -- fixtures (dev, ops) and helpers

pytestmark = pytest.mark.gpu
Z = G.load("g20_sgcn_net.npz")
PICKS = sorted({k.split(".")[0] for k in Z.files if k.startswith("pick")}, key=lambda t: int(t[4:]))
GEN_ARGS = dict(number_asymmetric_conv_layer=3, n_tcn=2, out_dims=12)


def state(prefix="net."):
    return {k[len(prefix):]: np.array(Z[k]) for k in Z.files
            if k.startswith(prefix) and not k[len(prefix):].startswith(("net_out", "logit_", "pick"))}


def net(dev, prefix="net.", **kw):
    from eigentrajectory_amd.sgcn import SGCN
    args = dict(number_asymmetric_conv_layer=7, embedding_dims=64, number_gcn_layers=1, dropout=0, obs_len=8, pred_len=6,
                n_tcn=5, in_dims=1, out_dims=20)
    args.update(kw)
    m = SGCN(**args)
    if prefix:
        m.load_state_dict({k: torch.from_numpy(v) for k, v in state(prefix).items()})
    return m.to(dev).eval()


def scale_err(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def run_graph(ops, m, dev, v, ids, idt):
    """v (T, N), the identities as numpy -> the device's (out, logit_s, logit_t) as numpy"""
    out, ls, lt = ops.sgcn_forward_graph(m, T(v[None, :, :, None], dev), [T(ids, dev), T(idt, dev)], want_logits=True)
    plain = ops.sgcn_forward_graph(m, T(v[None, :, :, None], dev), [T(ids, dev), T(idt, dev)])
    assert torch.equal(plain, out)  # asking for the logits changes nothing, and runs are bit-identical
    return N_(out), N_(ls), N_(lt)


def wrapper(dev, scene, predictor):
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    g2 = G.load("g2_fit_all_scenes.npz")
    hp = default_hyper_params(lr=1e-3, weight_decay=1e-4, static_dist=float(Z[f"{scene}.static_dist"]))
    model = EigenTrajectory(predictor, get_hook_func("sgcn"), hp)
    sd = model.state_dict()
    for k in sd:
        if k.startswith("ET_"):
            sd[k] = torch.from_numpy(g2[f"{scene}.{k}"])
    model.load_state_dict(sd)
    return model.to(dev).eval()


def split(scene, dev):
    obs, pred, sse = G.dataset(scene, "test")
    return T(obs, dev), T(pred, dev), np.asarray(sse)


def test_graph_form_on_the_recorded_scenes(dev, ops):
    m, sd = net(dev), state()
    direct = 0
    for t in PICKS:
        v, ids, idt = Z[f"{t}.v"][0, :, :, 0], Z[f"{t}.identity_s"], Z[f"{t}.identity_t"]
        out, ls, lt = run_graph(ops, m, dev, v, ids, idt)
        assert out.shape == Z[f"{t}.net_out"].shape and ls.shape == Z[f"{t}.logit_s"].shape
        SN.check_against(sd, v, ids, idt, out, ls, lt)
        if (np.array_equal(SN.decisions_fp32(ls), SN.decisions_fp32(Z[f"{t}.logit_s"]))
                and np.array_equal(SN.decisions_fp32(lt), SN.decisions_fp32(Z[f"{t}.logit_t"]))):
            direct += 1  # the same decisions as the reference on every entry: its output directly
            assert scale_err(out, Z[f"{t}.net_out"]) <= SN.TOL, t
        via_module = m(T(Z[f"{t}.v"], dev), [T(ids, dev), T(idt, dev)])  # forward is the graph form
        assert np.array_equal(N_(via_module), out)
    print(f"sgcn recorded scenes with the reference's decisions on every entry: {direct} of {len(PICKS)}")
    assert direct >= len(PICKS) - 2  # (two picks carry an undecided entry)


def test_generic_layer_counts(dev, ops):
    m, sd = net(dev, "gen.", **GEN_ARGS), state("gen.")
    for i in range(2):
        t = str(Z[f"gen.pick{i}"])
        v, ids, idt = Z[f"{t}.v"][0, :, :, 0], Z[f"{t}.identity_s"], Z[f"{t}.identity_t"]
        out, ls, lt = run_graph(ops, m, dev, v, ids, idt)
        SN.check_against(sd, v, ids, idt, out, ls, lt)
        if (np.array_equal(SN.decisions_fp32(ls), SN.decisions_fp32(Z[f"gen.logit_s{i}"]))
                and np.array_equal(SN.decisions_fp32(lt), SN.decisions_fp32(Z[f"gen.logit_t{i}"]))):
            assert scale_err(out, Z[f"gen.net_out{i}"]) <= SN.TOL


def test_identities_are_honoured(dev, ops):
    """the identities are read as given, with their broadcast strides: the bridge's all-ones temporal one, eye(T) per
    pedestrian, and a spatial one that changes with t"""
    m, sd = net(dev), state()
    t = next(t for t in PICKS if Z[f"{t}.v"].shape[2] == 8)
    v = Z[f"{t}.v"][0, :, :, 0]
    n, T_ = 8, 8
    ids, idt = SN.bridge_identities(T_, n)
    eye_t = np.ascontiguousarray(np.broadcast_to(np.eye(T_, dtype=np.float32), (n, T_, T_)))
    ids_t = np.ascontiguousarray(np.eye(n, dtype=np.float32)[None] * (1 + 0.25 * np.arange(T_, dtype=np.float32))[:, None, None])
    outs = []
    for a, b in ((ids, idt), (ids, eye_t), (ids_t, idt)):
        out, ls, lt = run_graph(ops, m, dev, v, a, b)
        SN.check_against(sd, v, a, b, out, ls, lt)
        outs.append(out)
    for i in range(3):
        for j in range(i):
            assert scale_err(outs[i], outs[j]) > 1e-3, (i, j)


@pytest.mark.parametrize("n", SN.RAGGED)
def test_ragged_sizes(dev, ops, n):
    m, sd = net(dev), state()
    v = SN.synthetic_v(n)
    ids, idt = SN.bridge_identities(8, n)
    out, ls, lt = run_graph(ops, m, dev, v, ids, idt)
    SN.check_against(sd, v, ids, idt, out, ls, lt)


def test_scenes_form(dev, ops):
    model = wrapper(dev, "eth", net(dev))
    m, sd = model.baseline_model, state()
    sizes = list(SN.SPLIT_SIZES)
    C_obs, nrm = SN.synthetic_split(sizes, SN.SPLIT_SEED)
    Cd, nd = T(C_obs, dev), T(nrm, dev)
    Cc, ls, lt = ops.sgcn_forward_scenes(m, Cd, nd, scene_sizes=sizes, want_logits=True)
    assert Cc.shape == (6, sum(sizes), 20) and Cc.is_contiguous()
    assert torch.equal(ops.sgcn_forward_scenes(m, Cd, nd, scene_sizes=sizes), Cc)
    Cc, ls, lt = N_(Cc), N_(ls), N_(lt)
    lo = sq = und = total = 0
    for n in sizes:
        v = SN.scene_input(C_obs, nrm, lo, lo + n)
        ids, idt = SN.bridge_identities(8, n)
        fig = SN.check_against(sd, v, ids, idt, Cc[:, lo:lo + n], ls[32 * sq:32 * (sq + n * n)].reshape(8, 4, n, n),
                               lt[256 * lo:256 * (lo + n)].reshape(n, 4, 8, 8))
        und, total = und + fig["undecided"], total + fig["entries"]
        # the graph form through the bridge: the same decisions wherever the logits agree on them
        o = nd[:2, lo:lo + n] - nd[:2, lo:lo + n].mean(dim=1, keepdim=True)
        net_in = model.hook_func.model_forward_pre_hook(Cd[:, lo:lo + n], o, None)
        ref, gs, gt = ops.sgcn_forward_graph(m, *net_in, want_logits=True)
        same = (np.array_equal(SN.decisions_fp32(N_(gs)), SN.decisions_fp32(ls[32 * sq:32 * (sq + n * n)].reshape(8, 4, n, n)))
                and np.array_equal(SN.decisions_fp32(N_(gt)), SN.decisions_fp32(lt[256 * lo:256 * (lo + n)].reshape(n, 4, 8, 8))))
        assert np.abs(N_(gs).ravel() - ls[32 * sq:32 * (sq + n * n)]).max() <= SN.DELTA
        if same:
            assert scale_err(Cc[:, lo:lo + n], N_(ref)) <= SN.TOL, (lo, n)
        assert torch.equal(model._predict(Cd[:, lo:lo + n], o, None), ref)
        lo, sq = lo + n, sq + n * n
    assert und <= SN.CAP_SPLIT * total
    # a scene's result does not depend on its neighbours: alone and in the middle of the split, bit for bit
    lo = sum(sizes[:3])
    alone = N_(ops.sgcn_forward_scenes(m, Cd[:, lo:lo + 64].contiguous(), nd[:, lo:lo + 64].contiguous(), scene_sizes=[64]))
    assert np.array_equal(alone, Cc[:, lo:lo + 64])
    one = N_(ops.sgcn_forward_scenes(m, Cd[:, lo:lo + 64].contiguous(), nd[:, lo:lo + 64].contiguous()))  # no scene list
    assert np.array_equal(one, alone)


@pytest.mark.parametrize("scene", G.SCENES)
def test_split_end_to_end(dev, scene):
    """evaluate_split with G2's descriptors and G20's weights against the reference's per-pedestrian ADE / FDE, on the
    scenes without an undecided entry in the reference's run; the split means over ALL scenes."""
    model = wrapper(dev, scene, net(dev))
    obs, pred, sse = split(scene, dev)
    res = model.evaluate_split(obs, pred, sse)
    decided_scene = Z[f"{scene}.min_abs_logit"] >= SN.DELTA
    assert decided_scene.mean() >= (0.65 if scene == "univ" else 0.90)
    rows = np.repeat(decided_scene, Z[f"{scene}.scene_size"])
    for key in ("ADE", "FDE"):
        ref = Z[f"{scene}.{key.lower()}"]
        got = N_(res[key]).astype(np.float64)
        err = np.abs(got - ref) / np.abs(ref).max()
        print(f"sgcn {scene} {key}: decided rows {int(rows.sum())} of {rows.size}, beyond TOL {int((err[rows] > SN.TOL).sum())}, "
              f"max {err[rows].max():.3e}; undecided rows beyond TOL {int((err[~rows] > SN.TOL).sum())}, "
              f"max {err[~rows].max() if (~rows).any() else 0:.3e}; mean diff {abs(got.mean() - ref.mean(dtype=np.float64)):.3e}")
        assert err[rows].max() <= SN.TOL, (key, float(err[rows].max()))  # (no pinned deviations: DESIGN §4)
        assert abs(float(got.mean()) - float(ref.mean(dtype=np.float64))) <= 3e-4
    if scene == "eth":  # ETTrainer.test's scene-by-scene path through the hooks gives the same means
        from eigentrajectory_amd.data import TrajectoryData
        from eigentrajectory_amd.trainer import ETTrainer
        data = TrajectoryData.from_arrays(N_(obs), N_(pred), sse)
        tr = ETTrainer(model, model.hyper_params, data, data, data, mode="sequenced", device=dev)
        means = tr.test()
        assert abs(means["ADE"] - float(N_(res["ADE"]).mean(dtype=np.float64))) <= 1e-5
        assert abs(means["FDE"] - float(N_(res["FDE"]).mean(dtype=np.float64))) <= 1e-5


def test_hook_path_captured_and_replayed(dev):
    model = wrapper(dev, "eth", net(dev))
    obs, pred, sse = split("eth", dev)
    s, e = (int(v) for v in sse[np.argmax(sse[:, 1] - sse[:, 0])])
    o = obs[s:e].contiguous()
    eager = model.forward(o)["recon_traj"].clone()
    rep = model.forward_replayed(o)["recon_traj"].clone()
    assert torch.equal(rep, eager)
    new = {k: torch.from_numpy(v) for k, v in state("net.").items()}
    gen = torch.Generator().manual_seed(5)
    new = {k: v + 0.05 * torch.randn(v.shape, generator=gen) for k, v in new.items()}
    model.baseline_model.load_state_dict(new)  # in place: the captured graph sees the new weights
    eager2 = model.forward(o)["recon_traj"].clone()
    rep2 = model.forward_replayed(o)["recon_traj"].clone()
    assert not torch.equal(eager2, eager)
    assert torch.equal(rep2, eager2)


def test_errors_and_empty_inputs(dev, ops):
    from eigentrajectory_amd._lib import SGCN_MAX_N, ETLibraryError
    m = net(dev)
    ids, idt = SN.bridge_identities(8, 3)
    v = T(SN.synthetic_v(3)[None, :, :, None], dev)
    ident = [T(ids, dev), T(idt, dev)]
    good = m(v, ident)
    assert good.shape == (6, 3, 20) and torch.isfinite(good).all()
    # N = 0: empty in, empty out
    out = m(torch.zeros((1, 8, 0, 1), device=dev), [torch.zeros((1, 0, 0), device=dev), torch.zeros((0, 1, 1), device=dev)])
    assert out.shape == (6, 0, 20)
    out = ops.sgcn_forward_scenes(m, torch.zeros((6, 0), device=dev), torch.zeros((4, 0), device=dev), scene_sizes=[])
    assert out.shape == (6, 0, 20)
    C_obs, nrm = SN.synthetic_split([7], 2)
    a = N_(ops.sgcn_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=[0, 3, 0, 4, 0]))
    b = N_(ops.sgcn_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=[3, 4]))
    assert np.array_equal(a, b) and np.isfinite(a).all()
    # inputs the kernels read in place: contiguous, on the model's device
    wide = torch.zeros((1, 8, 3, 2), device=dev)[..., :1]
    assert not wide.is_contiguous()
    with pytest.raises(ValueError, match="contiguous"):
        m(wide, ident)
    with pytest.raises(ValueError, match="contiguous float32 tensor on"):
        m(v.cpu(), [t.cpu() for t in ident])
    with pytest.raises(ValueError, match="are not"):
        m(v, [ident[0], torch.ones((3, 2, 2), device=dev)])
    big = SGCN_MAX_N + 1
    with pytest.raises(ValueError, match="exceeds"):
        m(torch.zeros((1, 8, big, 1), device=dev), [torch.eye(big, device=dev)[None], torch.ones((big, 1, 1), device=dev)])
    with pytest.raises(ValueError, match="exceeds"):
        ops.sgcn_forward_scenes(m, torch.zeros((6, big), device=dev), torch.zeros((4, big), device=dev))
    with pytest.raises(ETLibraryError, match="no CPU path"):
        net("cpu")(v.cpu(), [t.cpu() for t in ident])
    # outside the native family: constructs, the forward answers ET_ERR_UNSUPPORTED
    for kw in (dict(num_heads=2), dict(obs_len=9), dict(out_dims=65), dict(number_asymmetric_conv_layer=9)):
        bad = net(dev, prefix=None, **kw)
        vv = torch.zeros((1, bad.obs_len, 3, 1), device=dev)
        with pytest.raises(ETLibraryError, match="status 3"):
            bad(vv, ident)
    with pytest.raises(RuntimeError, match="training"):
        net(dev).train()(v, ident)
    with pytest.raises(RuntimeError, match="dropout"):
        net(dev, prefix=None, dropout=0.1)(v, ident)
    assert torch.equal(m(v, ident), good)  # nothing faulted: the device still answers, bit for bit
