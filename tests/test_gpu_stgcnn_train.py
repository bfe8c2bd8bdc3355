"""Native ET-STGCNN training on the GPU (csrc/et_stgcnn_train.hip; eigentrajectory_amd/stgcnn.py): every kept value of both
passes, the output, every gradient and the BatchNorm buffers against the float64 restatement's derived bounds
(tests/_stgcnn_train_np.py: step by step on the device's own kept inputs of each step), the training forward against the
stock-torch twin (tests/_stgcnn_twin.py), the scenes form, determinism, zero and one-hot upstream gradients, a NaN scene,
the autograd contract and a wrapped model under ETTrainer.  No tolerance is fixed in advance: every comparison with the
restatement is |device - value| <= bound.

Measured on the MI355X ("STGCNN training"): every comparison within its bound; largest error / bound of the
gradients per group gcn 0.23, tcn 0.30, residual 0.28, prelu 0.076, tpcnns 0.34, tpcnn_ouput 0.33, prelus 0.13; of the output
0.17; of the buffers 0.51; of a kept forward value 1.000 (one rounding against a half-ulp bound), of a kept backward value
0.999.  Fixture G31, the device against the reference's float64 gradients within the whole-chain bound: largest error / bound
0.32 (tp3_n1; 0.055 over the ET-shape cases, the recorded real scene included), against its fp32 gradients 0.14 of (bound +
that run's error); |device - reference| / largest entry at most 1.1e-2 (tp3_n2), 4.9e-4 for the ET shape."""
import ctypes as C

import numpy as np
import pytest
import torch

from . import _golden as G
from . import _stgcnn_np as SN
from . import _stgcnn_train_cases as CS
from . import _stgcnn_train_np as TN
from . import _stgcnn_twin as TW
from ._gpu_common import *  # noqa: F401,F403 -- fixtures (dev, ops) and helpers

pytestmark = pytest.mark.gpu
BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def fresh(dev, name):
    """a module of its own: every training forward moves the buffers"""
    return CS.module(name, dev).train()


def views_np(views):
    return {k: [N_(x) for x in val] if isinstance(val, list) else N_(val) for k, val in views.items()}


def native(ops, dev, m, v, a, d_out, want_views=True):
    """training forward + backward, graph form -> (out (S,k,n), {name: gradient}, kept values, buffers after) as numpy, and
    the flat gradient buffer"""
    n = v.shape[1]
    ws = ops.stgcnn_train_workspace(m, n)
    out = ops.stgcnn_train_forward_graph(m, T(v[None, None], dev), T(a, dev), ws)
    flat = ops.stgcnn_backward_graph(m, ws, T(d_out, dev))
    grads = {k: N_(g) for k, g in ops.stgcnn_grad_views(m, flat).items()}
    kept = views_np(ops.stgcnn_train_views(m, ws, n)) if want_views else None
    return N_(out)[0], grads, kept, CS.state(m), flat


def check(tag, name, sd, v, a, d_out, out, grads, kept, after):
    """every kept value, the output, every gradient and the buffers within the restatement's bound"""
    n = v.shape[1]
    R = TN.run(sd, v, a, d_out, momentum=CS.MOMENTUM, eps=CS.EPS, device=TN.device_dict(kept))
    worst = {g: 0.0 for g in TN.GROUPS}
    zero = TN.exact_zero_names(sd)
    for k, ref in R["grads"].items():
        if k in zero:
            assert not grads[k].any(), (tag, k)   # an exact zero
            continue
        worst[TN.group_of(k)] = max(worst[TN.group_of(k)], TN.compare(grads[k], ref))
    out_ratio = TN.compare(out, R["out"])
    buf_ratio = 0.0
    for k, ref in R["buffers"].items():
        if k.endswith("num_batches_tracked"):
            assert int(after[k]) == ref, (tag, k)
        else:
            buf_ratio = max(buf_ratio, TN.compare(after[k], ref))
    assert np.array_equal(kept["d_fin"].reshape(-1), np.asarray(d_out).reshape(-1)), tag
    fwd = {k: r for k, r in R["kept_ratio"].items() if not k.startswith(("d_", "stat_bwd"))}
    back = {k: r for k, r in R["kept_ratio"].items() if k.startswith(("d_", "stat_bwd"))}
    print(f"{tag}: kept forward error / bound {max(fwd.values()):.3f} ({max(fwd, key=fwd.get)}), backward "
          f"{max(back.values()):.3f} ({max(back, key=back.get)}), out {out_ratio:.3f}, buffers {buf_ratio:.3f}, gradients "
          + ", ".join(f"{g} {w:.2e}" for g, w in worst.items()) + f"; decisions {R['decisions']['prelu']}")
    assert R["decisions"]["prelu"]["flips_outside_band"] == 0, (tag, R["decisions"])
    assert not TN.vacuous(sd, R["grads"], n), (tag, TN.vacuous(sd, R["grads"], n))
    assert all(r <= 1.0 for r in R["kept_ratio"].values()), (tag, R["kept_ratio"])
    assert out_ratio <= 1.0 and buf_ratio <= 1.0, (tag, out_ratio, buf_ratio)
    assert all(w <= 1.0 for w in worst.values()), (tag, worst)
    return R


def run_case(ops, dev, name, n, tag, twin=False):
    m = fresh(dev, name)
    sd = CS.state(m)
    (v, a), d_out = CS.scene(name, n), CS.d_out(name, n)
    out, grads, kept, after, flat = native(ops, dev, m, v, a, d_out)
    check(f"{tag} {name} n={n}", name, sd, v, a, d_out, out, grads, kept, after)
    m2 = fresh(dev, name)
    out2, _, _, after2, flat2 = native(ops, dev, m2, v, a, d_out, want_views=False)
    assert torch.equal(flat, flat2) and np.array_equal(out, out2)          # a second run is bit-equal
    assert all(np.array_equal(after[k], after2[k]) for k in after)
    if twin:   # the training forward against the twin's fp32 output and buffers: both inside the whole-chain bound
        R = TN.run(sd, v, a, d_out, momentum=CS.MOMENTUM, eps=CS.EPS, propagate=True)
        tw = TW.clone(CS.module(name), torch.float32)
        tw_out = TW.forward(tw, v[None, None], a).detach().numpy()[0]
        assert TN.compare(out, R["out"]) <= 1.0 and TN.compare(tw_out, R["out"]) <= 1.0, (name, n)
        for k, b in TW.buffers(tw).items():
            if k.endswith("num_batches_tracked"):
                assert int(b) == int(after[k]) == R["buffers"][k]
            else:
                assert TN.compare(b, R["buffers"][k]) <= 1.0 and TN.compare(after[k], R["buffers"][k]) <= 1.0, (name, n, k)
    return grads


@pytest.mark.parametrize("name", list(CS.CONFIGS))
def test_exact_cases(dev, ops, name):
    """scenes of 1, 2, 3, 5 pedestrians, every configuration: everything within bound, the two biases in front of a
    BatchNorm and the unused tail exactly zero, a second run bit-equal, the forward and the buffers against the twin"""
    for n in CS.EXACT_N:
        grads = run_case(ops, dev, name, n, "exact", twin=True)
        assert grads["tpcnn_ouput.weight"].any() and grads["st_gcns.0.tcn.2.weight"].any()


@pytest.mark.parametrize("n", CS.RAGGED_N + (CS.BEYOND_N,))
def test_ragged_and_beyond(dev, ops, n):
    """63, 64, 65 and 257: the wavefront and workgroup edges; 512: beyond -- checked WITH the kept-value views, like the
    others (more than the out-and-gradients-only comparison asked for at that size; it still runs in about a second)"""
    run_case(ops, dev, "et", n, "ragged")


def _scenes_run(ops, dev, m, C_obs, nrm, sizes, d_all):
    out, ws = ops.stgcnn_train_forward_scenes(m, T(C_obs, dev), T(nrm, dev), sizes)
    flat = ops.stgcnn_backward_scenes(m, ws, T(d_all, dev), sizes)
    return N_(out), flat, ws


def _graph_d_out(d_scene, S, k):
    """(k, n, S) of the scenes form -> (1, S, k, n) of the graph form"""
    return np.ascontiguousarray(np.transpose(d_scene, (2, 0, 1)))[None]


def test_one_scene_scenes_form_is_the_graph_form(dev, ops):
    """a one-scene scenes call (with and without offsets) against the graph call on the scene's own input and the Laplacian
    in the kernel's float32 order: output, gradients and buffers bit for bit"""
    name = "et"
    _, S, k = CS.CONFIGS[name]
    for n in (5, 65):
        C_obs, nrm = CS.split([n], name, seed=5)
        d_all = np.random.default_rng(n).normal(0, 1, (k, n, S)).astype(np.float32)
        u = SN.scene_input(C_obs, nrm, 0, n)
        _, lap = CS.kernel_laplacian(u)
        mg = fresh(dev, name)
        out_g, _, kept, after_g, flat_g = native(ops, dev, mg, u, lap, _graph_d_out(d_all, S, k))
        for sizes in (None, [n]):
            ms = fresh(dev, name)
            out, flat, ws = _scenes_run(ops, dev, ms, C_obs, nrm, sizes, d_all)
            mine = views_np(ops.stgcnn_train_views(ms, ws, n))
            assert np.array_equal(mine["u"], u) and np.array_equal(mine["P"], kept["P"]), (n, sizes)
            assert np.array_equal(SN.c_pred_refine(out_g), out), (n, sizes)
            assert torch.equal(flat, flat_g), (n, sizes)
            assert all(np.array_equal(after_g[key], val) for key, val in CS.state(ms).items()), (n, sizes)


@pytest.mark.parametrize("which", sorted(CS.LAYOUTS))
def test_scenes_form_layouts(dev, ops, which):
    """a batch's gradients are the ascending fixed-order fp32 sum of the scenes' own device gradients (the reduction adds the
    same partials in the same order: bit for bit, which is inside any bound of that sum), its buffers those of consecutive
    single-scene calls, each scene's output and kept values what the scene gives alone; an empty scene contributes nothing
    and is no batch"""
    name = "et"
    _, S, k = CS.CONFIGS[name]
    sizes = CS.LAYOUTS[which]
    N = int(sum(sizes))
    C_obs, nrm = CS.split(sizes, name)
    d_all = np.random.default_rng(len(sizes)).normal(0, 1, (k, N, S)).astype(np.float32)
    m = fresh(dev, name)
    start = CS.state(m)
    out, flat, ws = _scenes_run(ops, dev, m, C_obs, nrm, list(sizes), d_all)
    assert torch.equal(flat, ops.stgcnn_backward_scenes(m, ws, T(d_all, dev), list(sizes)))
    alone = fresh(dev, name)   # the same weights and buffers: consecutive calls, scene after scene
    total, lo = None, 0
    for s, n in enumerate(sizes):
        if n == 0:
            continue
        cols = slice(lo, lo + n)
        o1, f1, w1 = _scenes_run(ops, dev, alone, C_obs[:, cols], nrm[:, cols], [n], d_all[:, cols])
        assert np.array_equal(o1, out[:, cols]), (which, s)
        mine = views_np(ops.stgcnn_train_views(m, ws, N, len(sizes), lo=lo, scene=s, scene_n=n))
        single = views_np(ops.stgcnn_train_views(alone, w1, n))
        for key, val in single.items():
            pairs = zip(val, mine[key]) if isinstance(val, list) else [(val, mine[key])]
            assert all(np.array_equal(p, q) for p, q in pairs), (which, s, key)
        total = N_(f1) if total is None else total + N_(f1)   # ascending, in fp32
        lo += n
    assert np.array_equal(N_(flat), total), which
    after, want = CS.state(m), CS.state(alone)
    assert all(np.array_equal(after[key], want[key]) for key in after), which
    live = sum(1 for n in sizes if n)
    assert all(int(after[key]) == int(start[key]) + live for key in after if key.endswith("num_batches_tracked"))


G31 = G.load("g31_stgcnn_train.npz")
G31_CASES = sorted({k.split(".")[0] for k in G31.files})
G31_WORST = {}


@pytest.mark.parametrize("case", G31_CASES)
def test_fixture_g31(dev, ops, case):
    """the reference's social_stgcnn in training mode (CPU): the device's gradients against its float64 gradients within the
    restatement's whole-chain bound, its buffers, and its fp32 output and gradients within the bound plus that run's own
    error.  The fixture tool could not keep every PReLU input outside the PROPAGATED band (its docstring); what matters for
    the gradient being ONE gradient is asserted here directly: the device's kept PReLU words have the float64 run's signs."""
    from .test_stgcnn_train_cpu import g31_gradients
    name = str(G31[f"{case}.config"])
    v, a, d_out = G31[f"{case}.v"], G31[f"{case}.a"], G31[f"{case}.d_out"]
    m = fresh(dev, name)
    sd = CS.state(m)
    out, grads, kept, after, _ = native(ops, dev, m, v, a, d_out)
    check(f"g31 {case}", name, sd, v, a, d_out, out, grads, kept, after)
    exact = TN.run(sd, v, a, d_out, momentum=CS.MOMENTUM, eps=CS.EPS)   # float64, its own decisions
    for key in ("a1", "s"):
        assert np.array_equal(kept[key] > 0, exact["kept"][key].val > 0), (case, key)
    for j, z in enumerate(exact["kept"]["tp_pre"]):
        assert np.array_equal(kept["tp_pre"][j] > 0, z.val > 0), (case, "tp_pre", j)
    R = TN.run(sd, v, a, d_out, momentum=CS.MOMENTUM, eps=CS.EPS, propagate=True)   # the distance to the exact gradient
    want, theirs = g31_gradients(sd, G31[f"{case}.grad64"]), g31_gradients(sd, G31[f"{case}.grad32"])
    zero = TN.exact_zero_names(sd)
    worst = worst32 = plain = 0.0
    for key, ref in R["grads"].items():
        if key in zero:
            continue   # the reference's is rounding noise or absent, the device's an exact zero (asserted in check)
        worst = max(worst, TN.compare(grads[key], TN.V(want[key], ref.err)))
        worst32 = max(worst32, TN.compare(grads[key], TN.V(theirs[key], ref.err + np.abs(theirs[key] - want[key]))))
        if want[key].size > 1 and np.abs(want[key]).max() > 0:
            plain = max(plain, float(np.abs(grads[key] - want[key]).max() / np.abs(want[key]).max()))
    out_ratio = TN.compare(out, R["out"])
    out32_ratio = TN.compare(G31[f"{case}.out32"], R["out"])
    buf = 0.0
    for key, ref in R["buffers"].items():
        if key.endswith("num_batches_tracked"):
            assert int(after[key]) == int(G31[f"{case}.{key}"])
        else:
            buf = max(buf, TN.compare(after[key], TN.V(G31[f"{case}.{key}"], ref.err)))
    G31_WORST[case] = worst
    print(f"g31 {case}: device against the reference's float64 gradients, error / whole-chain bound {worst:.3e} (largest over "
          f"the cases so far {max(G31_WORST.values()):.3e}); against its fp32 gradients {worst32:.3e} of (bound + that run's "
          f"error); |device - reference| / largest entry at most {plain:.2e}; output {out_ratio:.3e} (the reference's fp32 "
          f"output {out32_ratio:.3e}); buffers {buf:.3e}")
    assert worst <= 1.0 and worst32 <= 1.0 and out_ratio <= 1.0 and out32_ratio <= 1.0 and buf <= 1.0


def test_a_scene_beyond_the_scene_limit_is_not_computed(dev, ops):
    """[3, ET_SCENE_MAX_N + 1, 2]: the middle scene's output rows are NaN, it is no batch and contributes no gradient (its
    rows of d_out, NaN here, are not read); its neighbours are bit for bit what they give alone"""
    from eigentrajectory_amd import _lib as L
    name = "et"
    _, S, k = CS.CONFIGS[name]
    big = L.SCENE_MAX_N + 1
    sizes = [3, big, 2]
    N = sum(sizes)
    rng = np.random.default_rng(11)
    C_obs = rng.normal(0, 1, (k, N)).astype(np.float32)
    nrm = rng.normal(0, 5, (4, N)).astype(np.float32)
    d_all = rng.normal(0, 1, (k, N, S)).astype(np.float32)
    d_all[:, 3:3 + big] = np.nan
    m = fresh(dev, name)
    start = CS.state(m)
    out, flat, ws = _scenes_run(ops, dev, m, C_obs, nrm, sizes, d_all)
    assert np.isnan(out[:, 3:3 + big]).all() and np.isfinite(out[:, :3]).all() and np.isfinite(out[:, -2:]).all()
    alone = fresh(dev, name)
    total = None
    for cols in (slice(0, 3), slice(N - 2, N)):
        n = cols.stop - cols.start
        o1, f1, _ = _scenes_run(ops, dev, alone, C_obs[:, cols], nrm[:, cols], [n], d_all[:, cols])
        assert np.array_equal(o1, out[:, cols])
        total = N_(f1) if total is None else total + N_(f1)
    assert np.array_equal(N_(flat), total) and np.isfinite(total).all()
    after, want = CS.state(m), CS.state(alone)
    assert all(np.array_equal(after[key], want[key]) for key in after)
    assert all(int(after[key]) == int(start[key]) + 2 for key in after if key.endswith("num_batches_tracked"))


def test_zero_and_one_hot_d_out(dev, ops):
    name, n = "et", 5
    (v, a) = CS.scene(name, n)
    m = fresh(dev, name)
    sd = CS.state(m)
    _, grads, _, _, _ = native(ops, dev, m, v, a, np.zeros_like(CS.d_out(name, n)), want_views=False)
    assert all(not g.any() for g in grads.values())   # exact zeros
    d_out = np.zeros_like(CS.d_out(name, n))
    d_out[0, 7, 2, 3] = 1.0
    m = fresh(dev, name)
    out, grads, kept, after, _ = native(ops, dev, m, v, a, d_out)
    check("one-hot d_out", name, sd, v, a, d_out, out, grads, kept, after)
    assert grads["st_gcns.0.gcn.conv.weight"].any() and grads["tpcnns.0.weight"].any()


def test_a_nan_stays_in_its_scene(dev, ops):
    """a NaN in the one-pedestrian scene of [3, 1, 5]: only that scene's rows of the output are NaN; the NaN patterns of the
    gradients and of the buffers are the twin's (scene by scene, summed), except at the device's exact zeros"""
    name = "et"
    _, S, k = CS.CONFIGS[name]
    sizes = [3, 1, 5]
    C_obs, nrm = CS.split(sizes, name)
    C_obs = C_obs.copy()
    C_obs[2, 3] = np.nan
    d_all = np.random.default_rng(3).normal(0, 1, (k, 9, S)).astype(np.float32)
    m = fresh(dev, name)
    sd = CS.state(m)
    out, flat, _ = _scenes_run(ops, dev, m, C_obs, nrm, sizes, d_all)
    nan_rows = np.isnan(out).any(axis=(0, 2))
    assert np.array_equal(nan_rows, np.arange(9) == 3) and np.isnan(out[:, 3]).all()
    tw = TW.clone(CS.module(name), torch.float32)
    total, lo = None, 0
    for n in sizes:
        u = SN.scene_input(C_obs, nrm, lo, lo + n)
        with np.errstate(invalid="ignore"):
            adj = SN.adjacency(u).astype(np.float32)
        _, g = TW.grads(tw, u[None, None], adj, _graph_d_out(d_all[:, lo:lo + n], S, k))
        total = g if total is None else {key: total[key] + g[key] for key in g}
        lo += n
    grads = {key: N_(g) for key, g in ops.stgcnn_grad_views(m, flat).items()}
    zero = TN.exact_zero_names(sd)
    for key, g in grads.items():
        if key in zero:
            assert not g.any(), key
        else:
            assert np.array_equal(np.isnan(g), np.isnan(total[key].numpy())), key
    after = CS.state(m)
    for key, b in TW.buffers(tw).items():
        if key.endswith("num_batches_tracked"):
            assert int(after[key]) == int(b) == int(sd[key]) + 3
        else:
            assert np.array_equal(np.isnan(after[key]), np.isnan(b)), key


def test_autograd_contract(dev, ops):
    import eigentrajectory_amd as ET
    name, n = "et", 5
    m = ET.enable_native_training(CS.module(name, dev).train())
    (v, a), d_out = CS.scene(name, n), CS.d_out(name, n)
    tv, ta, td = T(v[None, None], dev), T(a, dev), T(d_out, dev)
    out = m(tv, ta)
    assert out.requires_grad and tuple(out.shape) == tuple(d_out.shape)
    out.backward(td)
    _, grads, _, after, _ = native(ops, dev, fresh(dev, name), v, a, d_out, want_views=False)
    unused = m.unused_parameter_names()
    assert unused == {"tpcnns.4.weight", "tpcnns.4.bias", "prelus.4.weight"}
    for key, p in m.named_parameters():
        if key in unused:
            assert p.grad is None and not grads[key].any(), key   # as in the reference: the optimiser skips them
        else:
            assert np.array_equal(N_(p.grad), grads[key]), key
    assert all(np.array_equal(after[key], val) for key, val in CS.state(m).items())   # the buffers moved as the ops path's
    with pytest.raises(RuntimeError, match="no input gradient"):
        m(tv.clone().requires_grad_(True), ta)
    out3 = m(tv, ta)
    with torch.no_grad():
        m.tpcnn_ouput.bias.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out3.backward(td)
    out4 = m(tv, ta)
    m.tpcnn_ouput.bias = torch.nn.Parameter(m.tpcnn_ouput.bias.detach().clone())   # another tensor under the same name
    with pytest.raises(RuntimeError, match="a parameter tensor was replaced between forward and backward"):
        out4.backward(td)
    m.eval()
    before = CS.state(m)
    assert m(tv, ta).requires_grad is False   # eval mode: the inference path, whatever the flag
    assert all(np.array_equal(before[key], val) for key, val in CS.state(m).items())   # ... and the buffers stay


def _wrapped(dev, native_flag, twin=False):
    import eigentrajectory_amd as ET
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.data import TrajectoryData
    from eigentrajectory_amd.trainer import ETTrainer
    from eigentrajectory_amd.utils import default_hyper_params
    fit_obs, fit_pred = synth(2048, seed=3)   # enough static and moving trajectories for the anchors
    obs, pred = fit_obs[:96], fit_pred[:96]
    hp = default_hyper_params(lr=1e-3, weight_decay=1e-4, static_dist=0.3, batch_size=8, clip_grad=10, lr_schd=False)
    model = ET.EigenTrajectory(TW.Twin(CS.module("et")) if twin else CS.module("et"), get_hook_func("stgcnn"), hp).to(dev)
    model.calculate_parameters(T(fit_obs, dev), T(fit_pred, dev))
    if native_flag:
        assert ET.enable_native_training(model) is model and model.baseline_model.native_training is True
    data = TrajectoryData.from_arrays(obs, pred, [(i, i + 3) for i in range(0, 96, 3)])
    return ETTrainer(model, hp, data, data, data, mode="sequenced", device=dev), data


def _six_steps(tr, data, first=None):
    tr.model.train()
    losses = []
    for step in range(6):
        tr.optimizer.zero_grad(set_to_none=True)
        losses.append(tr._train_batch(data, list(range(8))))
        if step == 0 and first:
            first(tr)
        tr.optimizer.step()
    return losses


def test_trainer_end_to_end(dev, ops):
    """6 sequenced steps of 8 scenes on the 96-row toy set (the SGCN test's), lr 1e-3, natively and with the SAME network in
    stock torch operators under autograd (tests/_stgcnn_twin.py) under the same ETTrainer.  The twin is the reference
    figure: its loss must drop by a clear margin (5 % over the six steps) for the learning rate and step count to stand, the
    native first loss (same weights, only fp32 rounding between the two forwards: 1e-4 is some hundred roundings) must equal
    the twin's, and the native sequence must drop at least half as far as the twin's.  Measured on the MI355X: twin 4.276520,
    4.086279, 3.920296, 3.774261, 3.644242, 3.531498 (a drop of 17 %); native the same six figures to 1e-7."""
    twin_tr, twin_data = _wrapped(dev, False, twin=True)
    twin_losses = _six_steps(twin_tr, twin_data)
    print("twin losses", twin_losses)
    assert np.isfinite(twin_losses).all() and twin_losses[-1] < 0.95 * twin_losses[0]
    tr, data = _wrapped(dev, True)
    start = CS.state(tr.predictor)

    def first(tr):
        params = dict(tr.predictor.named_parameters())
        unused = tr.predictor.unused_parameter_names()
        for key, p in params.items():
            if key in unused:
                assert p.grad is None, key
            else:
                assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), key
        assert sum(bool(p.grad.any()) for key, p in params.items() if key not in unused) >= len(params) - len(unused) - 2

    losses = _six_steps(tr, data, first)
    print("trainer losses", losses)
    after = CS.state(tr.predictor)
    for key in after:
        if key.endswith("num_batches_tracked"):
            assert int(after[key]) == int(start[key]) + 6 * 8, key   # one forward per scene
        elif key.endswith(("running_mean", "running_var")):
            assert np.abs(after[key] - start[key]).max() > 0 and np.isfinite(after[key]).all(), key
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert abs(losses[0] - twin_losses[0]) <= 1e-4 * abs(twin_losses[0])
    assert losses[0] - losses[-1] >= 0.5 * (twin_losses[0] - twin_losses[-1])
    plain, data = _wrapped(dev, False)
    plain.model.train()
    with pytest.raises(RuntimeError, match="training-mode forward and backward are not implemented"):
        plain._train_batch(data, [0])


def test_the_device_answers_after_the_refusals(dev, ops):
    """the host-side refusals of the new entries launch nothing: the eval forward is bit for bit what it was, and so are the
    buffers"""
    from eigentrajectory_amd import _lib as L
    name, n = "et", 5
    m = CS.module(name, dev).eval()
    (v, a) = CS.scene(name, n)
    tv, ta = T(v[None, None], dev), T(a, dev)
    before, state = ops.stgcnn_forward_graph(m, tv, ta).clone(), CS.state(m)
    params, _ = m.et_params()
    train = m.et_train_state()
    lib = L.lib()
    ws = ops.stgcnn_train_workspace(m, n)
    g = torch.zeros(int(lib.et_stgcnn_grad_floats(C.byref(params))), device=dev)
    d = T(CS.d_out(name, n), dev)
    out = torch.zeros((1, 20, 6, n), device=dev)
    assert lib.et_stgcnn_backward_graph(C.byref(params), n, L.ptr(d), L.ptr(g), g.numel(), L.ptr(ws), 16, None) == 4
    assert lib.et_stgcnn_backward_graph(C.byref(params), n, None, L.ptr(g), g.numel(), L.ptr(ws), ws.numel(), None) == 1
    assert lib.et_stgcnn_backward_graph(C.byref(params), n, L.ptr(d), L.ptr(g), 3, L.ptr(ws), ws.numel(), None) == 1
    assert lib.et_stgcnn_train_forward_graph(C.byref(params), C.byref(train), L.ptr(tv), L.ptr(ta), n, L.ptr(out), L.ptr(ws),
                                             16, None) == 4
    assert lib.et_stgcnn_train_forward_graph(C.byref(params), C.byref(train), L.ptr(tv), L.ptr(ta), n, None, L.ptr(ws),
                                             ws.numel(), None) == 1
    assert lib.et_stgcnn_train_forward_graph(C.byref(params), None, L.ptr(tv), L.ptr(ta), n, L.ptr(out), L.ptr(ws),
                                             ws.numel(), None) == 1
    bad = m.et_params()[0]
    bad.n_stgcnn = 2
    assert lib.et_stgcnn_train_forward_graph(C.byref(bad), C.byref(train), L.ptr(tv), L.ptr(ta), n, L.ptr(out), L.ptr(ws),
                                             ws.numel(), None) == 3
    assert lib.et_stgcnn_backward_graph(C.byref(bad), n, L.ptr(d), L.ptr(g), g.numel(), L.ptr(ws), ws.numel(), None) == 3
    torch.cuda.synchronize()
    assert torch.equal(ops.stgcnn_forward_graph(m, tv, ta), before) and not out.any() and not g.any()
    assert all(np.array_equal(state[key], val) for key, val in CS.state(m).items())
