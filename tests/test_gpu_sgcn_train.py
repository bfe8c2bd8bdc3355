"""Native ET-SGCN training on the GPU (csrc/et_sgcn_train.inl; eigentrajectory_amd/sgcn.py): the training forward against
the eval forward, every kept value and every gradient against the float64 restatement's derived bounds
(tests/_sgcn_train_np.py: both passes step by step on the device's own kept inputs of each step), the
scenes form, determinism, zero and sparse upstream gradients, the reference's float64 gradients (fixture G29) and a wrapped
model under ETTrainer.  No tolerance is fixed in advance: every comparison with the restatement is |device - value| <= bound.

Measured on the MI355X ("SGCN training"): every comparison within its bound; largest error / bound of the
gradients 0.24 (output), of a kept forward value 1.000 (one rounding against a half-ulp bound), of a kept backward value 0.98,
against G29's float64 gradients 0.14; the bound itself at most 0.12 of a multi-element tensor's largest entry."""
import ctypes as C

import numpy as np
import pytest
import torch

from eigentrajectory_amd import _lib as L_

from . import _golden as G
from . import _sgcn_np as SN
from . import _sgcn_train_cases as CS
from . import _sgcn_train_np as TN
from ._gpu_common import *  # noqa: F401,F403 -- fixtures (dev, ops) and helpers

pytestmark = pytest.mark.gpu
_MODULES = {}


def net(dev, name):
    if name not in _MODULES:
        _MODULES[name] = CS.module(name, dev).eval()
    return _MODULES[name]


def identities(name, n, dev):
    ids, idt = SN.bridge_identities(SN.CONFIGS[name]["k"] + 2, n)
    return (ids, idt), (T(ids, dev), T(idt, dev))


def views_np(views):
    return {k: [N_(x) for x in val] if isinstance(val, list) else N_(val) for k, val in views.items()}


def native(ops, dev, name, v, d_out, want_views=True):
    """training forward + backward, graph form -> (out, {name: gradient}, kept values) as numpy, and the flat buffer"""
    m = net(dev, name)
    n = v.shape[1]
    _, ident = identities(name, n, dev)
    tv = T(v[None, :, :, None], dev)
    ws = ops.sgcn_train_workspace(m, n)
    out = ops.sgcn_train_forward_graph(m, tv, ident, ws)
    flat = ops.sgcn_backward_graph(m, ident, ws, T(d_out, dev))
    grads = {k: N_(g) for k, g in ops.sgcn_grad_views(m, flat).items()}
    return N_(out), grads, views_np(ops.sgcn_train_views(m, ws, n)) if want_views else None, flat


def check(tag, name, v, d_out, out, grads, kept, exact=False):
    """every kept value, the output and every gradient within the restatement's bound; the decisions' bookkeeping"""
    ids, idt = SN.bridge_identities(v.shape[0], v.shape[1])
    R = TN.run(SN.random_state(name), v, ids, idt, d_out, device=kept)
    fig = R["decisions"]
    worst = {g: 0.0 for g in TN.GROUPS}
    for k, ref in R["grads"].items():
        if "key.bias" in k:
            assert not grads[k].any(), (tag, k)   # an exact zero
            continue
        worst[TN.group_of(k)] = max(worst[TN.group_of(k)], TN.compare(grads[k], ref))
    out_ratio = TN.compare(out, R["out"])
    back = {k: r for k, r in R["kept_ratio"].items() if k.startswith(("d_", "g_", "dir_", "dd_"))}
    loosest = max(float(g.err.max() / np.abs(g.val).max()) for g in R["grads"].values() if g.val.size > 1 and np.abs(g.val).max() > 1e-12)
    print(f"{tag}: kept error / bound {max(R['kept_ratio'].values()):.3f} ({max(R['kept_ratio'], key=R['kept_ratio'].get)}), of the "
          f"backward's {max(back.values()):.3f} ({max(back, key=back.get)}), bound / largest entry at most {loosest:.1e}, out "
          f"{out_ratio:.3f}, gradients " + ", ".join(f"{g} {w:.2e}" for g, w in worst.items()) + f"; decisions {fig}")
    for kind in ("mask", "prelu"):
        assert fig[kind]["flips_outside_band"] == 0, (tag, fig)
        assert fig[kind]["undecided"] <= SN.CAP_SCENE * fig[kind]["entries"], (tag, fig)
        if exact:
            assert fig[kind]["undecided"] == 0, (tag, fig)
    assert not TN.vacuous(R["grads"], v.shape[1]), (tag, TN.vacuous(R["grads"], v.shape[1]))   # zeros or a flipped sign would exceed every bound
    assert all(r <= 1.0 for r in R["kept_ratio"].values()), (tag, R["kept_ratio"])
    assert out_ratio <= 1.0, (tag, out_ratio)
    assert all(w <= 1.0 for w in worst.values()), (tag, worst)
    return R


@pytest.mark.parametrize("name", CS.EXACT_CONFIGS)
def test_exact_cases(dev, ops, name):
    """scenes of 1, 2, 3, 5 with the bridge's identities: everything within bound, with an EMPTY band"""
    m = net(dev, name)
    for n in CS.EXACT_N:
        v, d_out = CS.scene(name, n), CS.d_out(name, n)
        out, grads, kept, flat = native(ops, dev, name, v, d_out)
        _, ident = identities(name, n, dev)
        assert np.array_equal(out, N_(ops.sgcn_forward_graph(m, T(v[None, :, :, None], dev), ident)))  # bit-equal to eval
        check(f"exact {name} n={n}", name, v, d_out, out, grads, kept, exact=True)
        assert torch.equal(flat, native(ops, dev, name, v, d_out, want_views=False)[3])  # determinism


@pytest.mark.parametrize("name,n", CS.RAGGED)
def test_ragged_and_deep(dev, ops, name, n):
    v, d_out = CS.scene(name, n), CS.d_out(name, n)
    out, grads, kept, flat = native(ops, dev, name, v, d_out)
    _, ident = identities(name, n, dev)
    assert np.array_equal(out, N_(ops.sgcn_forward_graph(net(dev, name), T(v[None, :, :, None], dev), ident)))
    check(f"ragged {name} n={n}", name, v, d_out, out, grads, kept)
    assert torch.equal(flat, native(ops, dev, name, v, d_out, want_views=False)[3])


@pytest.mark.parametrize("which", sorted(CS.LAYOUTS))
def test_scenes_form(dev, ops, which):
    """a batch's gradients = the ascending fixed-order sum of the single-scene device gradients, within the fp32 bound of
    that sum: the batch adds the same per-workgroup partials in one chain over all scenes' chunks instead of scene by scene,
    so per element the two differ by at most gamma(chunks + scenes) x the sum of the partials' magnitudes, which the
    restatement bounds by ``tm`` (the sum of the terms' magnitudes) plus its own bound; the attention tensors follow from
    d alpha / d beta through the (linear) prep backward.  A scene's kept values do not depend on its neighbours, bit for bit."""
    name, sizes, C_obs, nrm = CS.layout(which)
    m = net(dev, name)
    sd = SN.random_state(name)
    N = int(sum(sizes))
    d_all = CS.d_out(name, N, seed=7)
    out, ws = ops.sgcn_train_forward_scenes(m, T(C_obs, dev), T(nrm, dev), list(sizes))
    assert np.array_equal(N_(out), N_(ops.sgcn_forward_scenes(m, T(C_obs, dev), T(nrm, dev), list(sizes))))
    flat = ops.sgcn_backward_scenes(m, ws, T(d_all, dev), list(sizes))
    assert torch.equal(flat, ops.sgcn_backward_scenes(m, ws, T(d_all, dev), list(sizes)))
    batch = {k: N_(g).astype(np.float64) for k, g in ops.sgcn_grad_views(m, flat).items()}
    total = {k: np.zeros(np.asarray(w).shape, np.float32) for k, w in sd.items()}
    bound = {k: np.zeros(np.asarray(w).shape) for k, w in sd.items()}
    sum_n2, sq, n_chunks = sum(s * s for s in sizes), 0, 0
    dab_tm = [[np.zeros(4), np.zeros(4)], [np.zeros(4), np.zeros(4)]]
    pr = None
    for s, lo, n, _ in SN.scenes_of(sizes, C_obs, nrm):
        d_out = np.ascontiguousarray(d_all[:, lo:lo + n])
        mine = views_np(ops.sgcn_train_views(m, ws, N, sum_n2, len(sizes), lo=lo, sq=sq, scene_n=n))
        v = np.ascontiguousarray(mine["v"])   # the scene's input as the batch formed it (its mean in the kernel's order)
        _, grads, kept, _ = native(ops, dev, name, v, d_out)
        for k, val in kept.items():   # bit for bit what the scene gives alone
            pairs = zip(val, mine[k]) if isinstance(val, list) else [(val, mine[k])]
            assert all(np.array_equal(a, b) for a, b in pairs), (which, s, k)
        sq += n * n
        ids, idt = SN.bridge_identities(v.shape[0], n)
        R = TN.run(sd, v, ids, idt, d_out, device=kept)
        pr = R["prep"]
        n_chunks += -(-n * n * v.shape[0] // L_.SGCN_BWD_ITEMS) + -(-n // L_.SGCN_BWD_CHUNK) + 2
        for k in total:
            total[k] = total[k] + grads[k]          # ascending, in fp32
            tm = R["grads"][k].tm
            bound[k] += R["grads"][k].err + (np.abs(R["grads"][k].val) if tm is None else np.asarray(tm).reshape(bound[k].shape))
        for a in range(2):
            for q in range(2):
                dab_tm[a][q] += R["dab"][a][q].tm + R["dab"][a][q].err
    g = TN.gamma(n_chunks + len(sizes) + 2)
    for a, att in enumerate(("spatial_attention.", "temporal_attention.")):   # the attention tensors: through the prep backward
        lin = TN.prep_bwd(pr[a], TN.V(np.zeros(4), g * dab_tm[a][0]), TN.V(np.zeros(4), g * dab_tm[a][1]), SN.SWA + att)
        for k, val in lin.items():
            bound[k] = val.err.reshape(bound[k].shape) + 2 * len(sizes) * TN.U * np.abs(total[k])
    worst = 0.0
    for k in total:
        if "key.bias" in k:
            assert not batch[k].any()
            continue
        b = bound[k] if "attention" in k else g * bound[k]
        err = np.abs(batch[k] - total[k].astype(np.float64))
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = float(np.where(err == 0, 0.0, err / b).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (which, k, ratio)
    print(f"scenes form {which}: batch against the fixed-order sum of {len(sizes)} scenes, error / bound {worst:.3f}")


def test_one_scene_scenes_form_is_the_graph_form(dev, ops):
    name, n = "et", 17
    m = net(dev, name)
    C_obs, nrm = SN.synthetic_split([n], 5, SN.CONFIGS[name]["k"])
    d_out = CS.d_out(name, n)
    _, ws = ops.sgcn_train_forward_scenes(m, T(C_obs, dev), T(nrm, dev), [n])
    v = np.ascontiguousarray(N_(ops.sgcn_train_views(m, ws, n)["v"]))   # the input as the scenes form builds it
    out_g, _, kept, flat_g = native(ops, dev, name, v, d_out)
    for sizes in (None, [n]):
        out, ws = ops.sgcn_train_forward_scenes(m, T(C_obs, dev), T(nrm, dev), sizes)
        assert np.array_equal(N_(out), out_g)
        assert torch.equal(ops.sgcn_backward_scenes(m, ws, T(d_out, dev), sizes), flat_g)


@pytest.mark.parametrize("n", CS.BEYOND)
def test_sizes_beyond_the_restatement(dev, ops, n):
    """n = 257, 512 with k1: the 64-bit offsets and the workspace arithmetic.  No float64 comparison (tests/_sgcn_np.py: at
    these sizes ZeroSoftmax cancels in fp32 itself)."""
    name = "k1"
    m = net(dev, name)
    C_obs, nrm = SN.synthetic_split([n], SN.SEEDS[name, "big" if n == 257 else "limit"], SN.CONFIGS[name]["k"])
    v, d_out = SN.scene_input(C_obs, nrm, 0, n), CS.d_out(name, n)
    out, grads, _, flat = native(ops, dev, name, v, d_out, want_views=False)
    _, ident = identities(name, n, dev)
    assert np.array_equal(out, N_(ops.sgcn_forward_graph(m, T(v[None, :, :, None], dev), ident)))
    assert all(np.isfinite(g).all() for g in grads.values()) and any(g.any() for g in grads.values())
    assert torch.equal(flat, native(ops, dev, name, v, d_out, want_views=False)[3])


def test_zero_and_sparse_d_out(dev, ops):
    name, n = "et", 17
    v = CS.scene(name, n)
    _, grads, _, _ = native(ops, dev, name, v, np.zeros_like(CS.d_out(name, n)), want_views=False)
    assert all(not g.any() for g in grads.values())   # exact zeros
    d_out = np.zeros_like(CS.d_out(name, n))
    d_out[:, 11] = CS.d_out(name, n)[:, 11]           # one pedestrian: its tail, everybody's adjacency rows
    out, grads, kept, _ = native(ops, dev, name, v, d_out)
    check("sparse d_out", name, v, d_out, out, grads, kept)
    assert grads["output.weight"].any() and grads[SN.SWA + "spatial_attention.query.weight"].any()


G29 = G.load("g29_sgcn_train.npz")
G29_CASES = sorted({k.split(".")[0] for k in G29.files if "." in k})


@pytest.mark.parametrize("case", G29_CASES)
def test_fixture_g29(dev, ops, case):
    """the reference's TrajectoryModel in training mode (CPU): its fp32 output within TOL of the largest entry (tests/_sgcn_np.py:
    two fp32 implementations), its logits and mask decisions, and its float64 gradients within the restatement's whole-chain
    bound of the device's (the step-by-step check of the same case is ``check``: this one is about the reference)"""
    name = str(G29[f"{case}.config"])
    v, d_out = G29[f"{case}.v"], G29[f"{case}.d_out"]
    out, grads, kept, _ = native(ops, dev, name, v, d_out)
    ref_out = G29[f"{case}.out32"]
    assert np.abs(out - ref_out).max() <= SN.TOL * np.abs(ref_out).max()
    for mine, theirs in ((kept["stack_s"][-1], G29[f"{case}.logit_s32"]), (kept["stack_t"][-1], G29[f"{case}.logit_t32"])):
        assert np.abs(mine - theirs).max() <= SN.DELTA                       # the two fp32 runs' logits ...
        assert np.array_equal(SN.decisions_fp32(mine), SN.decisions_fp32(theirs))   # ... and mask decisions (none in the band)
    R = check(f"g29 {case}", name, v, d_out, out, grads, kept)
    worst = 0.0
    wanted = CS.g29_gradients(G29, case, SN.random_state(name))
    ids, idt = SN.bridge_identities(v.shape[0], v.shape[1])
    R = TN.run(SN.random_state(name), v, ids, idt, d_out, propagate=True)   # the distance to the exact gradient: whole-chain bounds
    for k, ref in R["grads"].items():
        want = wanted[k]
        if "key.bias" in k:
            continue   # the reference's is rounding noise (tests/test_sgcn_train_cpu.py), the device's an exact zero
        worst = max(worst, TN.compare(grads[k], TN.V(want, ref.err)))
    print(f"g29 {case}: device against the reference's float64 gradients, error / bound {worst:.3e}")
    assert worst <= 1.0
    if f"{case}.grad32" in G29.files:   # the reference's fp32 run: within the device's bound plus that run's own error
        theirs, worst32 = CS.g29_gradients(G29, case, SN.random_state(name), "grad32"), 0.0
        for k, ref in R["grads"].items():
            if "key.bias" not in k:
                worst32 = max(worst32, TN.compare(grads[k], TN.V(theirs[k], ref.err + np.abs(theirs[k] - wanted[k]))))
        print(f"g29 {case}: device against the reference's fp32 gradients, error / (bound + that run's error) {worst32:.3e}")
        assert worst32 <= 1.0


def _wrapped(dev, native_flag):
    import eigentrajectory_amd as ET
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.data import TrajectoryData
    from eigentrajectory_amd.trainer import ETTrainer
    from eigentrajectory_amd.utils import default_hyper_params
    fit_obs, fit_pred = synth(2048, seed=3)   # enough static and moving trajectories for the anchors
    obs, pred = fit_obs[:96], fit_pred[:96]
    hp = default_hyper_params(lr=1e-3, weight_decay=1e-4, static_dist=0.3, batch_size=8, clip_grad=10, lr_schd=False)
    model = ET.EigenTrajectory(CS.module("et"), get_hook_func("sgcn"), hp).to(dev)
    model.calculate_parameters(T(fit_obs, dev), T(fit_pred, dev))
    if native_flag:
        assert ET.enable_native_training(model) is model and model.baseline_model.native_training is True
    data = TrajectoryData.from_arrays(obs, pred, [(i, i + 3) for i in range(0, 96, 3)])
    return ETTrainer(model, hp, data, data, data, mode="sequenced", device=dev), data


def test_trainer_end_to_end(dev, ops):
    tr, data = _wrapped(dev, True)
    tr.model.train()
    losses = []
    for step in range(6):
        tr.optimizer.zero_grad(set_to_none=True)
        losses.append(tr._train_batch(data, list(range(8))))
        if step == 0:
            params = dict(tr.predictor.named_parameters())
            assert len(params) == 97 and all(p.grad is not None and p.grad.shape == p.shape for p in params.values())
            assert all(bool(torch.isfinite(p.grad).all()) for p in params.values())
            assert sum(bool(p.grad.any()) for p in params.values()) >= 95   # the two key.bias are exact zeros
        tr.optimizer.step()
    print("trainer losses", losses)
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    plain, data = _wrapped(dev, False)
    plain.model.train()
    with pytest.raises(RuntimeError, match="training-mode forward is not implemented"):
        plain._train_batch(data, [0])


def test_autograd_contract(dev, ops):
    import eigentrajectory_amd as ET
    name, n = "et", 5
    m = ET.enable_native_training(CS.module(name, dev).train())
    _, ident = identities(name, n, dev)
    v, d_out = T(CS.scene(name, n)[None, :, :, None], dev), T(CS.d_out(name, n), dev)
    out = m(v, list(ident))
    assert out.requires_grad
    out.backward(d_out)
    _, grads, _, _ = native(ops, dev, name, CS.scene(name, n), CS.d_out(name, n), want_views=False)
    assert all(np.array_equal(N_(p.grad), grads[k]) for k, p in m.named_parameters())
    with pytest.raises(RuntimeError, match="no input gradient"):
        m(v.clone().requires_grad_(True), list(ident))
    out3 = m(v, list(ident))
    with torch.no_grad():
        m.output.bias.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out3.backward(d_out)
    out4 = m(v, list(ident))
    m.output.bias = torch.nn.Parameter(m.output.bias.detach().clone())   # another tensor under the same name
    with pytest.raises(RuntimeError, match="a parameter tensor was replaced between forward and backward"):
        out4.backward(d_out)
    m.eval()
    assert m(v, list(ident)).requires_grad is False   # eval mode: the inference path, whatever the flag


def test_the_device_answers_after_the_refusals(dev, ops):
    """the host-side refusals of the new entries launch nothing: the eval forward is bit for bit what it was"""
    from eigentrajectory_amd import _lib as L
    name, n = "et", 5
    m = net(dev, name)
    _, ident = identities(name, n, dev)
    v = T(CS.scene(name, n)[None, :, :, None], dev)
    before = ops.sgcn_forward_graph(m, v, ident).clone()
    params, _ = m.et_params()
    lib = L.lib()
    ws = ops.sgcn_train_workspace(m, n)
    g = torch.zeros(int(lib.et_sgcn_grad_floats(C.byref(params))), device=dev)
    d = T(CS.d_out(name, n), dev)
    args = (L.ptr(ident[0]), 1, L.ptr(ident[1]), 1, n, L.ptr(d), L.ptr(g), g.numel())
    assert lib.et_sgcn_backward_graph(C.byref(params), *args, L.ptr(ws), 16, None) == 4          # ET_ERR_WORKSPACE
    assert lib.et_sgcn_backward_graph(C.byref(params), *args[:6], None, g.numel(), L.ptr(ws), ws.numel(), None) == 1
    assert lib.et_sgcn_backward_graph(C.byref(params), *args[:7], 3, L.ptr(ws), ws.numel(), None) == 1
    bad = m.et_params()[0]
    bad.dropout = 0.5
    assert lib.et_sgcn_backward_graph(C.byref(bad), *args, L.ptr(ws), ws.numel(), None) == 3      # ET_ERR_UNSUPPORTED
    assert lib.et_sgcn_train_forward_graph(C.byref(params), L.ptr(v), L.ptr(ident[0]), 1, L.ptr(ident[1]), 1, n, None, None,
                                           None, L.ptr(ws), ws.numel(), None) == 1
    torch.cuda.synchronize()
    assert torch.equal(ops.sgcn_forward_graph(m, v, ident), before)
