"""Native ET-DMRGCN training on the GPU (csrc/et_dmrgcn_train.hip; eigentrajectory_amd/dmrgcn.py): every kept value of both
passes, the output and every gradient against the float64 restatement's derived bounds (tests/_dmrgcn_train_np.py: step by
step on the device's own kept inputs of each step), under a NULL, an all-ones, a seeded 0.8, an all-zeros and a strictly
upper-triangular keep mask; bit-equality with the eval kernel when nothing is dropped; the scenes form, determinism, the
scene cap, zero and one-hot upstream gradients, a NaN scene, fixture G32, the autograd contract and a wrapped model under
ETTrainer.  No tolerance is fixed in advance: every comparison with the restatement is |device - value| <= bound.

Measured on the MI355X ("DMRGCN training"): every comparison within its bound; largest error / bound of a
gradient 0.61 (tpcnns.3.gtacn.0.0.weight, et n = 2), of a kept backward value 0.66 (d q), of a kept forward value 1.000 (one
rounding against a half-ulp bound).  Fixture G32, the device against the reference's float64 gradients within the
whole-chain bound: largest error / bound 0.17 (tp1_n1; 0.15 over the ET-shape cases, the recorded real scene included);
|device - reference| / largest entry at most 6.3e-7.  ETTrainer: native within 1.2e-6 of the twin's fp32 loss sequence, the
twin's fp32 and float64 runs 3.2e-6 apart."""
import ctypes as C

import numpy as np
import pytest
import torch

from . import _dmrgcn_np as DN
from . import _dmrgcn_train_cases as CS
from . import _dmrgcn_train_np as TN
from . import _dmrgcn_twin as TW
from ._gpu_common import *  # noqa: F401,F403 -- fixtures (dev, ops) and helpers
from .test_dmrgcn_train_cpu import G32, G32_CASES, g32_case, g32_gradients

pytestmark = pytest.mark.gpu
_MODULES = {}


def module(dev, name):
    """the configuration's module on the device (no buffers: a training forward changes nothing in it) and its state"""
    if name not in _MODULES:
        _MODULES[name] = (CS.module(name, dev).train(), CS.random_state(name))
    return _MODULES[name]


def views_np(views):
    return {q: [N_(x) for x in val] if isinstance(val, list) else N_(val) for q, val in views.items()}


def native(ops, dev, m, v, a, d_out, keep, want_views=True):
    """training forward + backward, graph form -> (out (S,k,n), {name: gradient}, kept values) as numpy, and the flat
    gradient buffer"""
    n = v.shape[1]
    ws = ops.dmrgcn_train_workspace(m, n)
    out = ops.dmrgcn_train_forward_graph(m, T(v[None, None], dev), T(a[None], dev), ws, keep=None if keep is None else T(keep, dev))
    flat = ops.dmrgcn_backward_graph(m, ws, T(d_out, dev))
    grads = {q: N_(g) for q, g in ops.dmrgcn_grad_views(m, flat).items()}
    kept = views_np(ops.dmrgcn_train_views(m, ws, n)) if want_views else None
    return N_(out)[0], grads, kept, flat


def check(tag, sd, v, a, d_out, keep, kind, out, grads, kept, decided=True):
    """every kept value, the output and every gradient within the restatement's bound; every device PReLU word with the
    restatement's sign (``decided``: the case's seed leaves no input inside its band, so there is no exception)"""
    n = v.shape[1]
    R = TN.run(sd, v, a, d_out[0], keep=keep, device=TN.device_dict(kept))
    zero = TN.analytic_zero(sd, n, kind)
    worst = {}
    for q, ref in R["grads"].items():
        worst[q] = TN.compare(grads[q], ref)   # an analytically zero tensor: held to its bound around zero
        if q in zero and (n == 1 or kind == "zeros"):
            assert not grads[q].any(), (tag, q)   # L = 0: P is an exact zero, and so is the sum
    out_ratio = TN.compare(out, R["out"])
    assert np.array_equal(kept["u"], v), tag
    fwd = {q: r for q, r in R["kept_ratio"].items() if not q.startswith("d_")}
    back = {q: r for q, r in R["kept_ratio"].items() if q.startswith("d_")}
    top = max(worst, key=worst.get)
    print(f"{tag}: kept forward error / bound {max(fwd.values()):.3f} ({max(fwd, key=fwd.get)}), backward "
          f"{max(back.values()):.3f} ({max(back, key=back.get)}), out {out_ratio:.3f}, gradients {worst[top]:.3f} ({top}); "
          f"decisions {R['decisions']['prelu']}")
    assert R["decisions"]["prelu"]["flips_outside_band"] == 0, (tag, R["decisions"])
    if decided:
        assert R["decisions"]["prelu"]["undecided"] == 0, (tag, R["decisions"])
    assert not TN.vacuous(sd, R["grads"], zero), (tag, TN.vacuous(sd, R["grads"], zero))
    assert all(r <= 1.0 for r in R["kept_ratio"].values()), (tag, R["kept_ratio"])
    assert out_ratio <= 1.0, (tag, out_ratio)
    assert all(w <= 1.0 for w in worst.values()), (tag, {q: w for q, w in worst.items() if w > 1.0})
    return R


def run_case(ops, dev, name, n, kind, tag, decided=True):
    m, sd = module(dev, name)
    (v, a), d_out = CS.scene(name, n), CS.d_out(name, n)
    keep = CS.keep_mask(kind, v.shape[0], n)
    out, grads, kept, flat = native(ops, dev, m, v, a, d_out, keep)
    check(f"{tag} {name} n={n} {kind}", sd, v, a, d_out, keep, kind, out, grads, kept, decided)
    out2, _, _, flat2 = native(ops, dev, m, v, a, d_out, keep, want_views=False)
    assert torch.equal(flat, flat2) and np.array_equal(out, out2)          # a second run is bit-equal
    return out, grads


def eval_out(ops, dev, m, v, a):
    m.eval()
    try:
        return N_(ops.dmrgcn_forward_graph(m, T(v[None, None], dev), T(a[None], dev)))[0]
    finally:
        m.train()


@pytest.mark.parametrize("name", list(CS.CONFIGS))
def test_exact_cases(dev, ops, name):
    """scenes of 1, 2, 3, 5 pedestrians, every configuration, every mask: everything within bound, a second run bit-equal;
    with a NULL and with an all-ones mask the training forward's output is the eval kernel's bit for bit; the upper
    triangular mask and its transpose give different outputs"""
    m, _ = module(dev, name)
    for n in CS.EXACT_N:
        outs = {}
        for kind in CS.MASKS:
            outs[kind], grads = run_case(ops, dev, name, n, kind, "exact")
            assert grads["tpcnns.0.tpcn.0.0.weight"].any() and grads["st_dmrgcns.0.tcn.1.bias"].any()
            assert grads["st_dmrgcns.0.tcn.1.weight"].any() == (n > 1 and kind != "zeros")   # L = 0: the tcn's input is 0
        v, a = CS.scene(name, n)
        ref = eval_out(ops, dev, m, v, a)
        assert np.array_equal(outs["null"], ref) and np.array_equal(outs["ones"], ref), (name, n)
        if n > 2:
            assert not np.array_equal(outs["draw"], ref) and not np.array_equal(outs["zeros"], ref), (name, n)
            lower = np.ascontiguousarray(np.swapaxes(CS.keep_mask("triu", v.shape[0], n), -1, -2))
            out_t, _, _, _ = native(ops, dev, m, v, a, CS.d_out(name, n), lower, want_views=False)
            assert not np.array_equal(out_t, outs["triu"]), (name, n)     # [w, v] is not [v, w]


@pytest.mark.parametrize("n", (CS.train_arena_limit("et"), CS.train_arena_limit("et") + 1) + CS.RAGGED_N)
def test_arena_edge_and_ragged(dev, ops, n):
    """the largest scene whose training arena fits LDS and the first that runs from the workspace; 64, 65 and 257: the
    wavefront and workgroup edges.  A NULL mask (bit-equal to the eval kernel) and the seeded draw"""
    m, _ = module(dev, "et")
    decided = n <= CS.train_arena_limit("et") + 1   # larger scenes have 10^5 PReLU inputs: some lie inside their band
    out, _ = run_case(ops, dev, "et", n, "null", "ragged", decided)
    v, a = CS.scene("et", n)
    assert np.array_equal(out, eval_out(ops, dev, m, v, a)), n
    run_case(ops, dev, "et", n, "draw", "ragged", decided)


def _scenes_run(ops, dev, m, C_obs, nrm, sizes, d_all, keep):
    out, ws = ops.dmrgcn_train_forward_scenes(m, T(C_obs, dev), T(nrm, dev), sizes, keep=None if keep is None else T(keep, dev))
    flat = ops.dmrgcn_backward_scenes(m, ws, T(d_all, dev), sizes)
    return N_(out), flat, ws


def _graph_d_out(d_scene):
    """(k, n, S) of the scenes form -> (1, S, k, n) of the graph form"""
    return np.ascontiguousarray(np.transpose(d_scene, (2, 0, 1)))[None]


def _packed_keep(sizes, K, seed=9):
    """every scene's (2, 5, K, n, n) draw, one after the other -> (the packed mask, the list of the scenes' own)"""
    own = [CS.keep_mask("draw", K, n, seed + s) if n and n <= 512 else np.zeros((0,), np.uint8) for s, n in enumerate(sizes)]
    return np.concatenate([q.reshape(-1) for q in own]), own


def test_one_scene_scenes_form_is_the_graph_form(dev, ops):
    """a one-scene scenes call (with and without offsets) against the graph call on the scene's own input (the kept u: the
    scene mean is summed in the projection's order) and the bridge's adjacency of it: output, contraction rows and gradients
    bit for bit, below and above the arena's limit"""
    name = "et"
    _, S, k = CS.CONFIGS[name]
    m, _ = module(dev, name)
    for n in (5, 65):
        C_obs, nrm = CS.split([n], name, seed=5)
        d_all = np.random.default_rng(n).normal(0, 1, (k, n, S)).astype(np.float32)
        keep = CS.keep_mask("draw", k + 2, n)
        runs = []
        for sizes in (None, [n]):
            out, flat, ws = _scenes_run(ops, dev, m, C_obs, nrm, sizes, d_all, keep.reshape(-1))
            runs.append((out, flat, views_np(ops.dmrgcn_train_views(m, ws, n))))
        u = runs[0][2]["u"]
        assert np.array_equal(u[:k], C_obs) and np.abs(u - DN.scene_input(C_obs, nrm, 0, n)).max() <= 1e-5
        out_g, _, kept, flat_g = native(ops, dev, m, u, DN.adjacency(u), _graph_d_out(d_all), keep)
        for out, flat, mine in runs:
            assert np.array_equal(mine["u"], u) and np.array_equal(mine["P"], kept["P"]), n
            assert np.array_equal(DN.c_pred_refine(out_g), out), n
            assert torch.equal(flat, flat_g), n


@pytest.mark.parametrize("which", sorted(CS.LAYOUTS))
def test_scenes_form_layouts(dev, ops, which):
    """a batch's gradients are the ascending fixed-order fp32 sum of the scenes' own device gradients (bit for bit), each
    scene's output and kept values what the scene gives alone under its own block of the packed mask; an empty scene
    contributes nothing; a NULL mask is the all-ones mask"""
    name = "et"
    _, S, k = CS.CONFIGS[name]
    sizes = CS.LAYOUTS[which]
    N = int(sum(sizes))
    m, _ = module(dev, name)
    C_obs, nrm = CS.split(sizes, name)
    d_all = np.random.default_rng(len(sizes)).normal(0, 1, (k, N, S)).astype(np.float32)
    packed, own = _packed_keep(sizes, k + 2)
    out, flat, ws = _scenes_run(ops, dev, m, C_obs, nrm, list(sizes), d_all, packed)
    assert torch.equal(flat, ops.dmrgcn_backward_scenes(m, ws, T(d_all, dev), list(sizes)))
    total, lo = None, 0
    for s, n in enumerate(sizes):
        if n == 0:
            continue
        cols = slice(lo, lo + n)
        o1, f1, w1 = _scenes_run(ops, dev, m, C_obs[:, cols], nrm[:, cols], [n], d_all[:, cols], own[s].reshape(-1))
        assert np.array_equal(o1, out[:, cols]), (which, s)
        mine = views_np(ops.dmrgcn_train_views(m, ws, N, len(sizes), lo=lo, scene=s, scene_n=n))
        single = views_np(ops.dmrgcn_train_views(m, w1, n))
        for key, val in single.items():
            pairs = zip(val, mine[key]) if isinstance(val, list) else [(val, mine[key])]
            assert all(np.array_equal(p, q) for p, q in pairs), (which, s, key)
        total = N_(f1) if total is None else total + N_(f1)   # ascending, in fp32
        lo += n
    assert np.array_equal(N_(flat), total), which
    out_null, flat_null, _ = _scenes_run(ops, dev, m, C_obs, nrm, list(sizes), d_all, None)
    out_ones, flat_ones, _ = _scenes_run(ops, dev, m, C_obs, nrm, list(sizes), d_all, np.ones_like(packed))
    assert np.array_equal(out_null, out_ones) and torch.equal(flat_null, flat_ones)
    m.eval()
    assert np.array_equal(out_null, N_(ops.dmrgcn_forward_scenes(m, T(C_obs, dev), T(nrm, dev), list(sizes))))
    m.train()


def test_a_scene_above_the_cap_is_not_computed(dev, ops):
    """[3, 513, 2]: the middle scene's output rows are NaN and it contributes no gradient (its rows of d_out, NaN here, are
    not read; it takes no room in the packed mask); its neighbours are bit for bit what they give alone"""
    name = "et"
    _, S, k = CS.CONFIGS[name]
    big = CS.BEYOND_N
    sizes = [3, big, 2]
    N = sum(sizes)
    m, _ = module(dev, name)
    rng = np.random.default_rng(11)
    C_obs = rng.normal(0, 1, (k, N)).astype(np.float32)
    nrm = rng.normal(0, 5, (4, N)).astype(np.float32)
    d_all = rng.normal(0, 1, (k, N, S)).astype(np.float32)
    d_all[:, 3:3 + big] = np.nan
    packed, own = _packed_keep(sizes, k + 2)
    assert packed.size == 10 * (k + 2) * (9 + 4)
    out, flat, _ = _scenes_run(ops, dev, m, C_obs, nrm, sizes, d_all, packed)
    assert np.isnan(out[:, 3:3 + big]).all() and np.isfinite(out[:, :3]).all() and np.isfinite(out[:, -2:]).all()
    total = None
    for s, cols in ((0, slice(0, 3)), (2, slice(N - 2, N))):
        n = cols.stop - cols.start
        o1, f1, _ = _scenes_run(ops, dev, m, C_obs[:, cols], nrm[:, cols], [n], d_all[:, cols], own[s].reshape(-1))
        assert np.array_equal(o1, out[:, cols])
        total = N_(f1) if total is None else total + N_(f1)
    assert np.array_equal(N_(flat), total) and np.isfinite(total).all()
    with pytest.raises(ValueError, match="exceeds the 512"):
        ops.dmrgcn_train_forward_scenes(m, T(C_obs, dev), T(nrm, dev), None)
    only = [big]
    out1, flat1, _ = _scenes_run(ops, dev, m, C_obs[:, 3:3 + big], nrm[:, 3:3 + big], only, d_all[:, 3:3 + big], None)
    assert np.isnan(out1).all() and not N_(flat1).any()   # no live scene: exact zeros


def test_zero_and_one_hot_d_out(dev, ops):
    name, n = "et", 5
    m, sd = module(dev, name)
    (v, a) = CS.scene(name, n)
    keep = CS.keep_mask("draw", v.shape[0], n)
    _, grads, _, _ = native(ops, dev, m, v, a, np.zeros_like(CS.d_out(name, n)), keep, want_views=False)
    assert all(not g.any() for g in grads.values())   # exact zeros
    d_out = np.zeros_like(CS.d_out(name, n))
    d_out[0, 7, 2, 3] = 1.0
    out, grads, kept, _ = native(ops, dev, m, v, a, d_out, keep)
    R = TN.run(sd, v, a, d_out[0], keep=keep, device=TN.device_dict(kept))
    assert all(r <= 1.0 for r in R["kept_ratio"].values()) and TN.compare(out, R["out"]) <= 1.0
    assert all(TN.compare(grads[q], ref) <= 1.0 for q, ref in R["grads"].items())
    assert R["decisions"]["prelu"]["flips_outside_band"] == 0
    assert grads["st_dmrgcns.0.gcns.0.conv.weight"].any() and grads["tpcnns.0.residual.0.weight"].any()


def test_a_nan_stays_in_its_scene(dev, ops):
    """a NaN in the one-pedestrian scene of [3, 1, 5]: only that scene's rows of the output are NaN, and the other scenes'
    outputs are what they are without it; the gradient sum over the scenes carries the NaN scene's partial"""
    name = "et"
    _, S, k = CS.CONFIGS[name]
    sizes = [3, 1, 5]
    m, _ = module(dev, name)
    C_obs, nrm = CS.split(sizes, name)
    clean, _, _ = _scenes_run(ops, dev, m, C_obs, nrm, sizes, np.zeros((k, 9, S), np.float32), None)
    C_obs = C_obs.copy()
    C_obs[2, 3] = np.nan
    d_all = np.random.default_rng(3).normal(0, 1, (k, 9, S)).astype(np.float32)
    packed, _ = _packed_keep(sizes, k + 2)
    for keep in (None, packed):
        out, flat, _ = _scenes_run(ops, dev, m, C_obs, nrm, sizes, d_all, keep)
        nan_rows = np.isnan(out).any(axis=(0, 2))
        assert np.array_equal(nan_rows, np.arange(9) == 3) and np.isnan(out[:, 3]).all()
        if keep is None:
            assert np.array_equal(out[:, nan_rows == 0], clean[:, nan_rows == 0])
        assert np.isnan(N_(flat)).any()
    # a larger scene: a dropped or out-of-bin entry still multiplies its column by 0, so the NaN reaches its whole time row
    v, a = CS.scene(name, 5)
    v = v.copy()
    v[3, 2] = np.nan
    with np.errstate(invalid="ignore"):
        adj = DN.adjacency(v)
    out, _, kept, _ = native(ops, dev, m, v, adj, CS.d_out(name, 5), CS.keep_mask("zeros", v.shape[0], 5))
    assert np.isnan(kept["P"][:, :, 0, 3]).all() and np.isfinite(kept["P"][:, :, 1]).all() and np.isnan(out).any()


G32_WORST = {}


@pytest.mark.parametrize("case", G32_CASES)
def test_fixture_g32(dev, ops, case):
    """the reference's social_dmrgcn in training mode (CPU) under the masks it drew: the device's kept values and gradients
    within the step bounds, its PReLU words with the float64 run's signs, and its gradients against the reference's float64
    gradients within the restatement's whole-chain bound; the plain distance is printed next to it"""
    name, sd, v, a, keep, d_out = g32_case(case)
    m, _ = module(dev, name)
    out, grads, kept, _ = native(ops, dev, m, v, a, d_out, keep)
    check(f"g32 {case}", sd, v, a, d_out, keep, "draw", out, grads, kept)
    R = TN.run(sd, v, a, d_out[0], keep=keep, propagate=True)   # the distance to the exact gradient
    want = g32_gradients(sd, G32[f"{case}.grad64"])
    worst = plain = 0.0
    for q, ref in R["grads"].items():
        worst = max(worst, TN.compare(grads[q], TN.V(want[q], ref.err)))
        if want[q].size > 1 and np.abs(want[q]).max() > ref.err.max():   # (not a tensor that is rounding residue on both sides)
            plain = max(plain, float(np.abs(grads[q] - want[q]).max() / np.abs(want[q]).max()))
    out_ratio = TN.compare(out, TN.V(G32[f"{case}.out64"], R["out"].err))
    out32_ratio = TN.compare(G32[f"{case}.out32"], TN.V(G32[f"{case}.out64"], R["out"].err))
    G32_WORST[case] = worst
    print(f"g32 {case}: device against the reference's float64 gradients, error / whole-chain bound {worst:.3e} (largest over "
          f"the cases so far {max(G32_WORST.values()):.3e}); |device - reference| / largest entry at most {plain:.2e}; output "
          f"{out_ratio:.3e} (the reference's fp32 output {out32_ratio:.3e})")
    assert worst <= 1.0 and out_ratio <= 1.0 and out32_ratio <= 1.0


def test_autograd_contract(dev, ops):
    import eigentrajectory_amd as ET
    name, n = "et", 5
    m = ET.enable_native_training(CS.module(name, dev).train())
    (v, a), d_out = CS.scene(name, n), CS.d_out(name, n)
    keep = CS.keep_mask("draw", v.shape[0], n)
    tv, ta, td, tk = T(v[None, None], dev), T(a[None], dev), T(d_out, dev), T(keep, dev)
    out, a_back = m(tv, ta, keep=tk)
    assert out.requires_grad and tuple(out.shape) == tuple(d_out.shape) and torch.equal(a_back, ta)
    out.backward(td)
    _, grads, _, _ = native(ops, dev, module(dev, name)[0], v, a, d_out, keep, want_views=False)
    first = {q: p.grad.clone() for q, p in m.named_parameters()}
    assert all(np.array_equal(N_(first[q]), grads[q]) for q in grads) and len(first) == len(grads)
    m(tv, ta, keep=tk)[0].backward(td)   # .grad accumulates
    assert all(torch.equal(p.grad, first[q] + first[q]) for q, p in m.named_parameters())
    torch.manual_seed(17)   # without keep the forward draws: the device generator's next two rand((1, 5, K, n, n))
    drawn = m(tv, ta)[0]
    torch.manual_seed(17)
    mask = m.draw_keep(n, dev)
    assert tuple(mask.shape) == (2, 5, v.shape[0], n, n) and mask.dtype == torch.uint8 and 0.6 < float(mask.float().mean()) < 0.95
    assert torch.equal(drawn, m(tv, ta, keep=mask)[0]) and not torch.equal(drawn, m(tv, ta, keep=torch.ones_like(mask))[0])
    out2 = m(tv, ta, keep=tk)[0]
    (g,) = torch.autograd.grad(out2, [m.tpcnns[0].tpcn[0][0].weight], td, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()                           # the backward is a kernel: a double backward is refused
    with pytest.raises(RuntimeError, match="no input gradient"):
        m(tv.clone().requires_grad_(True), ta)
    out3 = m(tv, ta, keep=tk)[0]
    with torch.no_grad():
        m.tpcnns[3].gtacn[0][0].bias.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out3.backward(td)                            # a version-counter change between forward and backward
    out4 = m(tv, ta, keep=tk)[0]
    blk = m.tpcnns[3].gtacn[0][0]
    blk.bias = torch.nn.Parameter(blk.bias.detach().clone())   # another tensor under the same name
    with pytest.raises(RuntimeError, match="a parameter tensor was replaced between forward and backward"):
        out4.backward(td)
    m.eval()
    ev = m(tv, ta)[0]
    assert ev.requires_grad is False and torch.equal(ev, ops.dmrgcn_forward_graph(m, tv, ta))   # eval: the inference path
    plain = CS.module(name, dev).train()
    with pytest.raises(RuntimeError, match="training-mode forward and backward are not implemented"):
        plain(tv, ta)


LR = 1e-3


def _wrapped(dev, kind, lr=LR):
    """kind: "native", "twin32" or "twin64" (the twin's parameters and arithmetic in float64 inside the fp32 wrapper)"""
    import eigentrajectory_amd as ET
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.data import TrajectoryData
    from eigentrajectory_amd.trainer import ETTrainer
    from eigentrajectory_amd.utils import default_hyper_params
    fit_obs, fit_pred = synth(2048, seed=3)   # enough static and moving trajectories for the anchors
    obs, pred = fit_obs[:96], fit_pred[:96]
    hp = default_hyper_params(lr=lr, weight_decay=1e-4, static_dist=0.3, batch_size=8, clip_grad=10, lr_schd=False)
    base = CS.module("et")
    net = {"native": lambda: base, "twin32": lambda: TW.Twin(base),
           "twin64": lambda: TW.Twin(base.double(), out_dtype=torch.float32)}[kind]()
    model = ET.EigenTrajectory(net, get_hook_func("dmrgcn"), hp).to(dev)
    model.calculate_parameters(T(fit_obs, dev), T(fit_pred, dev))
    if kind == "native":
        assert ET.enable_native_training(model) is model and model.baseline_model.native_training is True
    data = TrajectoryData.from_arrays(obs, pred, [(i, i + 3) for i in range(0, 96, 3)])
    return ETTrainer(model, hp, data, data, data, mode="sequenced", device=dev), data


def _six_steps(tr, data, seed=None):
    tr.model.train()
    if seed is not None:
        torch.manual_seed(seed)
    losses = []
    for _ in range(6):
        tr.optimizer.zero_grad(set_to_none=True)
        losses.append(tr._train_batch(data, list(range(8))))
        tr.optimizer.step()
    return losses


def test_trainer_end_to_end(dev, ops):
    """6 sequenced steps of 8 scenes on the 96-row toy set under one device seed, natively and with the SAME network in stock
    torch operators under autograd (tests/_dmrgcn_twin.py) under the same ETTrainer: both draw their masks from the device
    generator in the same order.  The twin is the reference figure: its loss must fall by at least 10 % over the six steps,
    and the native sequence must agree with it within ten times the distance between the twin's fp32 run and its float64 run
    (float64 parameters and arithmetic inside the same fp32 wrapper) of the same steps on the same recorded masks -- the
    factor of ten covers the different summation orders of two fp32 implementations."""
    tw32, data = _wrapped(dev, "twin32")
    l32 = _six_steps(tw32, data, seed=23)
    masks = list(tw32.predictor.log)
    assert len(masks) == 6 * 8 and all(tuple(q.shape) == (2, 5, 8, 3, 3) for q in masks)
    tw64, data64 = _wrapped(dev, "twin64")
    tw64.predictor.replay = iter(masks)
    l64 = _six_steps(tw64, data64)
    tr, datan = _wrapped(dev, "native")
    seen = []
    draw = tr.predictor.draw_keep
    tr.predictor.draw_keep = lambda *a, **kw: seen.append(draw(*a, **kw)) or seen[-1]
    ln = _six_steps(tr, datan, seed=23)
    assert len(seen) == len(masks) and all(torch.equal(p, q) for p, q in zip(seen, masks))   # one seed, the same draws
    dist = max(abs(p - q) for p, q in zip(l32, l64))
    gap = max(abs(p - q) for p, q in zip(ln, l32))
    print(f"twin fp32 losses {l32}\ntwin float64 losses {l64}\nnative losses {ln}\n"
          f"distance fp32 - float64 {dist:.3e}, native - twin fp32 {gap:.3e}, margin {10 * dist / max(gap, 1e-300):.2f}")
    assert np.isfinite(l32).all() and np.isfinite(l64).all() and np.isfinite(ln).all()
    assert l32[-1] <= 0.9 * l32[0], l32
    assert gap <= 10 * dist, (gap, dist)
    params = dict(tr.predictor.named_parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params.values())


def test_the_device_answers_after_the_refusals(dev, ops):
    """the host-side refusals of the new entries launch nothing: the eval forward is bit for bit what it was"""
    from eigentrajectory_amd import _lib as L
    name, n = "et", 5
    m = CS.module(name, dev).eval()
    (v, a) = CS.scene(name, n)
    tv, ta = T(v[None, None], dev), T(a[None], dev)
    before = ops.dmrgcn_forward_graph(m, tv, ta).clone()
    params, _ = m.et_params()
    lib = L.lib()
    ws = ops.dmrgcn_train_workspace(m, n)
    g = torch.zeros(int(lib.et_dmrgcn_grad_floats(C.byref(params))), device=dev)
    d = T(CS.d_out(name, n), dev)
    out = torch.zeros((1, 20, 6, n), device=dev)
    assert lib.et_dmrgcn_backward_graph(C.byref(params), n, L.ptr(d), L.ptr(g), g.numel(), L.ptr(ws), 16, None) == 4
    assert lib.et_dmrgcn_backward_graph(C.byref(params), n, None, L.ptr(g), g.numel(), L.ptr(ws), ws.numel(), None) == 1
    assert lib.et_dmrgcn_backward_graph(C.byref(params), n, L.ptr(d), L.ptr(g), 3, L.ptr(ws), ws.numel(), None) == 1
    assert lib.et_dmrgcn_train_forward_graph(C.byref(params), L.ptr(tv), L.ptr(ta), n, None, L.ptr(out), L.ptr(ws), 16, None) == 4
    assert lib.et_dmrgcn_train_forward_graph(C.byref(params), L.ptr(tv), L.ptr(ta), n, None, None, L.ptr(ws), ws.numel(),
                                             None) == 1
    assert lib.et_dmrgcn_train_forward_graph(C.byref(params), L.ptr(tv), L.ptr(ta), 513, None, L.ptr(out), L.ptr(ws),
                                             ws.numel(), None) == 1
    bad = m.et_params()[0]
    bad.n_stgcn = 2
    assert lib.et_dmrgcn_train_forward_graph(C.byref(bad), L.ptr(tv), L.ptr(ta), n, None, L.ptr(out), L.ptr(ws), ws.numel(),
                                             None) == 3
    assert lib.et_dmrgcn_backward_graph(C.byref(bad), n, L.ptr(d), L.ptr(g), g.numel(), L.ptr(ws), ws.numel(), None) == 3
    torch.cuda.synchronize()
    assert torch.equal(ops.dmrgcn_forward_graph(m, tv, ta), before) and not out.any() and not g.any()
