"""Native ET-Graph-TERN training on the GPU (csrc/et_graphtern_train.hip; eigentrajectory_amd/graphtern.py): every kept value
of both passes, the output and every gradient against the float64 restatement's derived bounds
(tests/_graphtern_train_np.py: step by step on the device's own kept inputs of each step), under a NULL, an all-ones, a seeded
0.8, an all-zeros and a strictly upper-triangular keep mask; bit-equality with the eval kernel when nothing is dropped; the
scenes form, determinism, the scene cap with guard bands, fixture G35, the autograd contract and a wrapped model under
ETTrainer.  No tolerance is fixed in advance: every comparison with the restatement is |device - value| <= bound.

Measured on the MI355X ("Graph-TERN training"), largest error / bound.  Kept forward values: d 0.459,
P 0.451, yp 0.414, x0 0.085, c0 0.174, y 0.997, c1 0.044, o 1.000 (one rounding against a half-ulp bound).  Kept backward
values: d_o 0.585, d_y 0.167, d_x0 0.305, d_yt 0.079.  Gradients by parameter group: gcn.conv 0.276 / 0.274 (weight / bias),
tcn 0.301 / 0.227, residual 0.212 / 0.227, tpcns 0.241 / 0.164, cpcns 0.371 / 0.325, restconv 0.140 / 0.103, rescconv
0.458 / 0.137.  Fixture G35, the device against the reference's float64 output and gradients within the whole-chain bound:
largest error / bound 0.137 (k1_n5); |device - reference| / largest entry at most 6.9e-7.  ETTrainer, two runs: native
7.45e-7 and 3.87e-7 from the twin's fp32 loss sequence, the twin's fp32 and float64 runs 6.56e-7 and 8.35e-7 apart:
test_trainer_end_to_end's bound was missed in the first run and held in the second (its docstring)."""
import ctypes as C

import numpy as np
import pytest
import torch

from . import _graphtern_np as GN
from . import _graphtern_train_cases as CS
from . import _graphtern_train_np as TN
from . import _graphtern_twin as TW
from ._gpu_common import *  # noqa: F401,F403 -- fixtures (dev, ops) and helpers
from .test_gpu_sgcn_shapes import guarded, guards_intact
from .test_graphtern_train_cpu import G35, G35_CASES, g35_case, g35_gradients

pytestmark = pytest.mark.gpu
_MODULES = {}
WORST = {"forward": {}, "backward": {}, "gradients": {}}


def module(dev, name):
    """the configuration's module on the device (no buffers: a training forward changes nothing in it) and its state"""
    if name not in _MODULES:
        _MODULES[name] = (CS.module(name, dev).train(), CS.random_state(name))
    return _MODULES[name]


def views_np(views):
    return {q: [N_(x) for x in val] if isinstance(val, list) else N_(val) for q, val in views.items()}


def native(ops, dev, m, u, d_out, keep, want_views=True):
    """training forward + backward, graph form -> (out (k,n,S), {name: gradient}, kept values) as numpy, and the flat
    gradient buffer"""
    n = u.shape[1]
    ws = ops.graphtern_train_workspace(m, n)
    out = ops.graphtern_train_forward_graph(m, T(GN.s_obs_of(u), dev), ws, keep=None if keep is None else T(keep, dev))
    flat = ops.graphtern_backward_graph(m, ws, T(d_out, dev))
    grads = {q: N_(g) for q, g in ops.graphtern_grad_views(m, flat).items()}
    kept = views_np(ops.graphtern_train_views(m, ws, n)) if want_views else None
    return N_(out)[0], grads, kept, flat


def group_of(q):
    return ".".join(p for p in q.split(".") if not p.isdigit())


def check(tag, sd, u, d_out, keep, out, grads, kept, decided=True):
    """every kept value, the output and every gradient within the restatement's bound; every device PReLU word with the
    restatement's sign (``decided``: the case's seed leaves no input inside its band, so there is no exception)"""
    R = TN.run(sd, u, None, d_out[0], keep=keep, device=TN.device_dict(kept))
    worst = {q: TN.compare(grads[q], ref) for q, ref in R["grads"].items()}
    assert not grads[TN.UNUSED].any(), tag
    out_ratio = TN.compare(out, R["out"])
    assert np.array_equal(kept["u"], u), tag
    fwd = {q: r for q, r in R["kept_ratio"].items() if not q.startswith("d_")}
    back = {q: r for q, r in R["kept_ratio"].items() if q.startswith("d_")}
    for q, r in fwd.items():
        WORST["forward"][q] = max(WORST["forward"].get(q, 0.0), r)
    for q, r in back.items():
        WORST["backward"][q] = max(WORST["backward"].get(q, 0.0), r)
    for q, r in worst.items():
        WORST["gradients"][group_of(q)] = max(WORST["gradients"].get(group_of(q), 0.0), r)
    top = max(worst, key=worst.get)
    print(f"{tag}: kept forward error / bound {max(fwd.values()):.3f} ({max(fwd, key=fwd.get)}), backward "
          f"{max(back.values()):.3f} ({max(back, key=back.get)}), out {out_ratio:.3f}, gradients {worst[top]:.3f} ({top}); "
          f"decisions {R['decisions']['prelu']}")
    print("  so far:", {g: {q: round(r, 3) for q, r in w.items()} for g, w in WORST.items()})
    assert R["decisions"]["prelu"]["flips_outside_band"] == 0, (tag, R["decisions"])
    if decided:
        assert R["decisions"]["prelu"]["undecided"] == 0, (tag, R["decisions"])
    assert not TN.vacuous(sd, R["grads"]), (tag, TN.vacuous(sd, R["grads"]))
    assert all(r <= 1.0 for r in R["kept_ratio"].values()), (tag, R["kept_ratio"])
    assert out_ratio <= 1.0, (tag, out_ratio)
    assert all(w <= 1.0 for w in worst.values()), (tag, {q: w for q, w in worst.items() if w > 1.0})
    return R


def run_case(ops, dev, name, n, kind, tag):
    m, sd = module(dev, name)
    u, d_out = CS.scene(name, n, kind), CS.d_out(name, n)
    keep = CS.keep_mask(kind, u.shape[0], n)
    out, grads, kept, flat = native(ops, dev, m, u, d_out, keep)
    check(f"{tag} {name} n={n} {kind}", sd, u, d_out, keep, out, grads, kept)
    out2, _, _, flat2 = native(ops, dev, m, u, d_out, keep, want_views=False)
    assert torch.equal(flat, flat2) and np.array_equal(out, out2)          # a second run is bit-equal
    return out, grads


def eval_out(ops, dev, m, u):
    m.eval()
    try:
        return N_(ops.graphtern_forward_graph(m, T(GN.s_obs_of(u), dev)))[0]
    finally:
        m.train()


@pytest.mark.parametrize("name", list(CS.CONFIGS))
def test_exact_cases(dev, ops, name):
    """scenes of 1, 2, 3, 5 pedestrians, every configuration, every mask: everything within bound, a second run bit-equal;
    with a NULL and with an all-ones mask the training forward's output is the eval kernel's bit for bit; the all-zeros mask
    (L = I) and the draw differ from it; the upper triangular mask and its transpose give different outputs"""
    m, _ = module(dev, name)
    for n in CS.EXACT_N:
        outs = {}
        for kind in CS.MASKS:
            outs[kind], grads = run_case(ops, dev, name, n, kind, "exact")
            # (a PReLU slope's gradient is an exact zero where no input of it is negative: k1 at n = 1 has 16 of them)
            assert all(g.any() for q, g in grads.items() if g.size > 1), (name, n, kind)
        u = CS.scene(name, n)
        ref = eval_out(ops, dev, m, u)
        assert np.array_equal(outs["null"], ref) and np.array_equal(outs["ones"], ref), (name, n)
        if n == 1:   # A = 0: nothing to drop
            assert all(np.array_equal(outs[q], ref) for q in CS.MASKS), name
        if n > 2:
            assert not np.array_equal(outs["draw"], ref) and not np.array_equal(outs["zeros"], ref), (name, n)
            assert not np.array_equal(outs["triu"], ref) and not np.array_equal(outs["triu"], outs["zeros"]), (name, n)
            lower = np.ascontiguousarray(np.swapaxes(CS.keep_mask("triu", u.shape[0], n), -1, -2))
            out_t, _, _, _ = native(ops, dev, m, u, CS.d_out(name, n), lower, want_views=False)
            assert not np.array_equal(out_t, outs["triu"]), (name, n)     # [w, v] is not [v, w]


@pytest.mark.parametrize("n", (CS.train_arena_limit("et"), CS.train_arena_limit("et") + 1) + CS.RAGGED_N)
def test_arena_edge_and_ragged(dev, ops, n):
    """the largest scene whose training arena fits LDS and the first that runs from the workspace; 64, 65 and 257: the
    wavefront and workgroup edges.  A NULL mask (bit-equal to the eval kernel) and the seeded draw"""
    m, _ = module(dev, "et")
    out, _ = run_case(ops, dev, "et", n, "null", "ragged")
    assert np.array_equal(out, eval_out(ops, dev, m, CS.scene("et", n, "null"))), n
    run_case(ops, dev, "et", n, "draw", "ragged")


def _scenes_run(ops, dev, m, C_obs, nrm, sizes, d_all, keep):
    out, ws = ops.graphtern_train_forward_scenes(m, T(C_obs, dev), T(nrm, dev), sizes, keep=None if keep is None else T(keep, dev))
    flat = ops.graphtern_backward_scenes(m, ws, T(d_all, dev), sizes)
    return N_(out), flat, ws


def _packed_keep(sizes, T_, seed=9):
    """every scene's (4, T, n, n) draw, one after the other -> (the packed mask, the list of the scenes' own)"""
    own = [CS.keep_mask("draw", T_, n, seed + s) if n and n <= 512 else np.zeros((0,), np.uint8) for s, n in enumerate(sizes)]
    return np.concatenate([q.reshape(-1) for q in own]), own


def test_one_scene_scenes_form_is_the_graph_form(dev, ops):
    """a one-scene scenes call (with and without offsets) against the graph call on the scene's own input (the kept u: the
    scene mean is summed in the projection's order): output, contracted rows and gradients bit for bit, below and above the
    arena's limit"""
    name = "et"
    k, S, _ = CS.CONFIGS[name]
    m, _ = module(dev, name)
    for n in (5, 65):
        C_obs, nrm = CS.split([n], name, seed=5)
        d_all = np.random.default_rng(n).normal(0, 1, (k, n, S)).astype(np.float32)
        keep = CS.keep_mask("draw", k + 2, n)
        runs = []
        for sizes in (None, [n]):
            out, flat, ws = _scenes_run(ops, dev, m, C_obs, nrm, sizes, d_all, keep.reshape(-1))
            runs.append((out, flat, views_np(ops.graphtern_train_views(m, ws, n))))
        u = runs[0][2]["u"]
        assert np.array_equal(u[:k], C_obs) and np.abs(u - GN.scene_input(C_obs, nrm, 0, n)).max() <= 1e-5
        out_g, _, kept, flat_g = native(ops, dev, m, u, d_all[None], keep)
        for out, flat, mine in runs:
            assert np.array_equal(mine["u"], u) and np.array_equal(mine["P"], kept["P"]) and np.array_equal(mine["d"], kept["d"]), n
            assert np.array_equal(out_g, out), n
            assert torch.equal(flat, flat_g), n


@pytest.mark.parametrize("which", sorted(CS.LAYOUTS))
def test_scenes_form_layouts(dev, ops, which):
    """a batch's gradients are the ascending fixed-order fp32 sum of the scenes' own device gradients (bit for bit), each
    scene's output and kept values what the scene gives alone under its own block of the packed mask (it does not depend on
    its neighbours); an empty scene contributes nothing; a NULL mask is the all-ones mask and the eval entry's output"""
    name = "et"
    k, S, _ = CS.CONFIGS[name]
    sizes = CS.LAYOUTS[which]
    N = int(sum(sizes))
    m, _ = module(dev, name)
    C_obs, nrm = CS.split(sizes, name)
    d_all = np.random.default_rng(len(sizes)).normal(0, 1, (k, N, S)).astype(np.float32)
    packed, own = _packed_keep(sizes, k + 2)
    out, flat, ws = _scenes_run(ops, dev, m, C_obs, nrm, list(sizes), d_all, packed)
    assert torch.equal(flat, ops.graphtern_backward_scenes(m, ws, T(d_all, dev), list(sizes)))
    total, lo = None, 0
    for s, n in enumerate(sizes):
        if n == 0:
            continue
        cols = slice(lo, lo + n)
        o1, f1, w1 = _scenes_run(ops, dev, m, C_obs[:, cols], nrm[:, cols], [n], d_all[:, cols], own[s].reshape(-1))
        assert np.array_equal(o1, out[:, cols]), (which, s)
        mine = views_np(ops.graphtern_train_views(m, ws, N, len(sizes), lo=lo, scene=s, scene_n=n))
        single = views_np(ops.graphtern_train_views(m, w1, n))
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
    assert np.array_equal(out_null, N_(ops.graphtern_forward_scenes(m, T(C_obs, dev), T(nrm, dev), list(sizes))))
    m.train()


def test_a_scene_above_the_cap_is_not_computed(dev, ops):
    """[3, 513, 2]: the middle scene's output rows are NaN and it contributes exactly nothing (its rows of d_out, NaN here,
    are not read; it takes no room in the packed mask); its neighbours are bit for bit what they give alone; the graph form
    raises; the guard bands around the workspace and the gradient buffer stay intact"""
    from eigentrajectory_amd import _lib as L
    name = "et"
    k, S, _ = CS.CONFIGS[name]
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
    assert packed.size == 4 * (k + 2) * (9 + 4)
    params, _ = m.et_params()
    lib = L.lib()
    nbytes = int(lib.et_graphtern_train_workspace_bytes(C.byref(params), N, len(sizes)))
    G_ = int(lib.et_graphtern_grad_floats(C.byref(params)))
    ws_whole, ws = guarded(nbytes, 0x5A, dev)
    g_whole, g_bytes = guarded(4 * G_, 0x5A, dev)
    out, _ = ops.graphtern_train_forward_scenes(m, T(C_obs, dev), T(nrm, dev), sizes, keep=T(packed, dev), workspace=ws)
    out = N_(out)
    off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev)
    td = T(d_all, dev)
    rc = lib.et_graphtern_backward_scenes(C.byref(params), N, L.ptr(off), len(sizes), L.ptr(td), L.ptr(g_bytes), G_, L.ptr(ws),
                                          nbytes, L.stream(dev))
    torch.cuda.synchronize()
    assert rc == 0 and guards_intact(ws_whole, nbytes, 0x5A) and guards_intact(g_whole, 4 * G_, 0x5A)
    flat = N_(g_bytes.view(torch.float32))
    assert np.isnan(out[:, 3:3 + big]).all() and np.isfinite(out[:, :3]).all() and np.isfinite(out[:, -2:]).all()
    total = None
    for s, cols in ((0, slice(0, 3)), (2, slice(N - 2, N))):
        n = cols.stop - cols.start
        o1, f1, _ = _scenes_run(ops, dev, m, C_obs[:, cols], nrm[:, cols], [n], d_all[:, cols], own[s].reshape(-1))
        assert np.array_equal(o1, out[:, cols])
        total = N_(f1) if total is None else total + N_(f1)
    assert np.array_equal(flat, total) and np.isfinite(total).all()
    with pytest.raises(ValueError, match="exceeds the 512"):
        ops.graphtern_train_forward_scenes(m, T(C_obs, dev), T(nrm, dev), None)
    only = [big]
    out1, flat1, _ = _scenes_run(ops, dev, m, C_obs[:, 3:3 + big], nrm[:, 3:3 + big], only, d_all[:, 3:3 + big], None)
    assert np.isnan(out1).all() and not N_(flat1).any()   # no live scene: exact zeros
    u = GN.scene_input(C_obs, nrm, 3, 3 + big)
    with pytest.raises(ValueError, match="exceeds the 512"):
        ops.graphtern_train_forward_graph(m, T(GN.s_obs_of(u), dev), ws)
    s_obs, o513 = T(GN.s_obs_of(u), dev), torch.zeros((1, k, big, S), device=dev)
    assert lib.et_graphtern_train_forward_graph(C.byref(params), L.ptr(s_obs), big, None, L.ptr(o513), L.ptr(ws), nbytes,
                                                L.stream(dev)) == 1
    torch.cuda.synchronize()
    assert not o513.any()


def test_zero_and_one_hot_d_out(dev, ops):
    name, n = "et", 5
    m, sd = module(dev, name)
    u = CS.scene(name, n)
    keep = CS.keep_mask("draw", u.shape[0], n)
    _, grads, _, _ = native(ops, dev, m, u, np.zeros_like(CS.d_out(name, n)), keep, want_views=False)
    assert all(not g.any() for g in grads.values())   # exact zeros
    d_out = np.zeros_like(CS.d_out(name, n))
    d_out[0, 2, 3, 7] = 1.0
    out, grads, kept, _ = native(ops, dev, m, u, d_out, keep)
    R = TN.run(sd, u, None, d_out[0], keep=keep, device=TN.device_dict(kept))
    assert all(r <= 1.0 for r in R["kept_ratio"].values()) and TN.compare(out, R["out"]) <= 1.0
    assert all(TN.compare(grads[q], ref) <= 1.0 for q, ref in R["grads"].items())
    assert R["decisions"]["prelu"]["flips_outside_band"] == 0
    assert grads["tp_mrgcns.0.gcn.conv.weight"].any() and grads["tpcnns.0.restconv.0.weight"].any()


G35_WORST = {}


@pytest.mark.parametrize("case", G35_CASES)
def test_fixture_g35(dev, ops, case):
    """the reference's graph_tern_light in training mode (CPU) under the mask it drew: the device's kept values and gradients
    within the step bounds, its PReLU words with the float64 run's signs, and its output and gradients against the
    reference's float64 ones within the restatement's whole-chain bound; the plain distance is printed next to it"""
    name, sd, u, keep, d_out = g35_case(case)
    m, _ = module(dev, name)
    out, grads, kept, _ = native(ops, dev, m, u, d_out, keep)
    check(f"g35 {case}", sd, u, d_out, keep, out, grads, kept)
    R = TN.run(sd, u, None, d_out[0], keep=keep, propagate=True)   # the distance to the exact gradient
    want = g35_gradients(sd, G35[f"{case}.grad64"])
    worst = plain = 0.0
    for q, ref in R["grads"].items():
        worst = max(worst, TN.compare(grads[q], TN.V(want[q], ref.err)))
        if want[q].size > 1 and np.abs(want[q]).max() > ref.err.max():
            plain = max(plain, float(np.abs(grads[q] - want[q]).max() / np.abs(want[q]).max()))
    out_ratio = TN.compare(out, TN.V(G35[f"{case}.out64"], R["out"].err))
    out32_ratio = TN.compare(G35[f"{case}.out32"], TN.V(G35[f"{case}.out64"], R["out"].err))
    G35_WORST[case] = worst
    print(f"g35 {case}: device against the reference's float64 gradients, error / whole-chain bound {worst:.3e} (largest over "
          f"the cases so far {max(G35_WORST.values()):.3e}); |device - reference| / largest entry at most {plain:.2e}; output "
          f"{out_ratio:.3e} (the reference's fp32 output {out32_ratio:.3e})")
    assert worst <= 1.0 and out_ratio <= 1.0 and out32_ratio <= 1.0


def test_autograd_contract(dev, ops):
    import eigentrajectory_amd as ET
    name, n = "et", 5
    m = ET.enable_native_training(CS.module(name, dev).train())
    u, d_out = CS.scene(name, n), CS.d_out(name, n)
    keep = CS.keep_mask("draw", u.shape[0], n)
    ts, td, tk = T(GN.s_obs_of(u), dev), T(d_out, dev), T(keep, dev)
    out = m(ts, keep=tk)
    assert out.requires_grad and tuple(out.shape) == tuple(d_out.shape)
    out.backward(td)
    _, grads, _, _ = native(ops, dev, module(dev, name)[0], u, d_out, keep, want_views=False)
    assert m.tp_mrgcns[0].prelu.weight.grad is None            # never applied: as torch leaves it
    first = {q: p.grad.clone() for q, p in m.named_parameters() if q != TN.UNUSED}
    assert all(np.array_equal(N_(first[q]), grads[q]) for q in first) and len(first) == len(grads) - 1
    assert all(bool(g.any()) for g in first.values())          # .grad is filled on every other parameter
    m(ts, keep=tk).backward(td)   # .grad accumulates
    assert all(torch.equal(p.grad, first[q] + first[q]) for q, p in m.named_parameters() if q != TN.UNUSED)
    torch.manual_seed(17)   # without keep the forward draws: the device generator's next rand((1, 4, T, n, n))
    drawn = m(ts)
    torch.manual_seed(17)
    mask = m.draw_keep(n, dev)
    assert tuple(mask.shape) == (4, u.shape[0], n, n) and mask.dtype == torch.uint8 and 0.6 < float(mask.float().mean()) < 0.95
    assert torch.equal(drawn, m(ts, keep=mask)) and not torch.equal(drawn, m(ts, keep=torch.ones_like(mask)))
    params = [p for q, p in m.named_parameters() if q != TN.UNUSED]
    for square in (False, True):   # the check of tests/test_gpu_native_train_once.py for this family
        o = m(ts, keep=tk)
        loss = (o * o).sum() if square else o.sum()
        gs = torch.autograd.grad(loss, list(m.native_parameters()), create_graph=True, allow_unused=True)
        used = [g for g in gs if g is not None]
        assert len(used) == len(params) and all(bool(torch.isfinite(g).all()) for g in used)
        with pytest.raises(RuntimeError, match="once_differentiable" if square else None):
            sum(g.sum() for g in used).backward()      # the backward is a kernel: differentiable once
    with pytest.raises(RuntimeError, match="no input gradient"):
        m(ts.clone().requires_grad_(True))
    out3 = m(ts, keep=tk)
    with torch.no_grad():
        m.tpcnns[3].cpcns[0][0].bias.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out3.backward(td)                            # a version-counter change between forward and backward
    out4 = m(ts, keep=tk)
    blk = m.tpcnns[3].cpcns[0][0]
    blk.bias = torch.nn.Parameter(blk.bias.detach().clone())   # another tensor under the same name
    with pytest.raises(RuntimeError, match="a parameter tensor was replaced between forward and backward"):
        out4.backward(td)
    m.eval()
    ev = m(ts)
    assert ev.requires_grad is False and torch.equal(ev, ops.graphtern_forward_graph(m, ts))   # eval: the inference path
    plain = CS.module(name, dev).train()
    with pytest.raises(RuntimeError, match="training"):
        plain(ts)


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
    model = ET.EigenTrajectory(net, get_hook_func("graphtern"), hp).to(dev)
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
    torch operators under autograd (tests/_graphtern_twin.py) under the same ETTrainer, the twin fed the masks the native
    run drew (recorded by wrapping ``draw_keep``).  The native loss sequence may not be farther from the twin's fp32
    sequence than the twin's own fp32 run is from its float64 run (float64 parameters and arithmetic inside the same fp32
    wrapper) on the same steps and masks: that distance is measured here, not fixed.

    Measured on the MI355X, two runs.  The native sequence is the same bits in both; the twin's sequences are not (stock
    torch's backward does not repeat from run to run), so the yardstick itself moves.  Run A: native - twin fp32 7.45e-7,
    twin fp32 - twin float64 6.56e-7: the bound is MISSED by 14 %.  Run B: 3.87e-7 against 8.35e-7: held.  The losses are
    fp32 numbers between 3.8 and 5.3 (ulp 4.8e-7), so every one of these distances is one to two ulp of the loss; the first
    step's losses, which no update precedes, agree to 6e-8, and the sequences then drift by single roundings that six
    AdamW steps pass on.  The assertion stays as the yardstick was set."""
    tr, datan = _wrapped(dev, "native")
    seen = []
    draw = tr.predictor.draw_keep
    tr.predictor.draw_keep = lambda *a, **kw: seen.append(draw(*a, **kw)) or seen[-1]
    ln = _six_steps(tr, datan, seed=23)
    assert len(seen) == 6 * 8 and all(tuple(q.shape) == (4, 8, 3, 3) and q.dtype == torch.uint8 for q in seen)
    tw32, data = _wrapped(dev, "twin32")
    tw32.predictor.replay = iter(seen)
    l32 = _six_steps(tw32, data)
    tw64, data64 = _wrapped(dev, "twin64")
    tw64.predictor.replay = iter(seen)
    l64 = _six_steps(tw64, data64)
    dist = max(abs(p - q) for p, q in zip(l32, l64))
    gap = max(abs(p - q) for p, q in zip(ln, l32))
    print(f"twin fp32 losses {l32}\ntwin float64 losses {l64}\nnative losses {ln}\n"
          f"distance fp32 - float64 {dist:.3e}, native - twin fp32 {gap:.3e}")
    assert np.isfinite(l32).all() and np.isfinite(l64).all() and np.isfinite(ln).all()
    assert gap <= dist, (gap, dist)
    params = dict(tr.predictor.named_parameters())
    assert all((p.grad is None) == (q == TN.UNUSED) for q, p in params.items())
    assert all(bool(torch.isfinite(p.grad).all()) for p in params.values() if p.grad is not None)


def test_the_device_answers_after_the_refusals(dev, ops):
    """the host-side refusals of the new entries launch nothing: the eval forward is bit for bit what it was"""
    from eigentrajectory_amd import _lib as L
    name, n = "et", 5
    m = CS.module(name, dev).eval()
    ts = T(GN.s_obs_of(CS.scene(name, n)), dev)
    before = ops.graphtern_forward_graph(m, ts).clone()
    params, _ = m.et_params()
    lib = L.lib()
    ws = ops.graphtern_train_workspace(m, n)
    g = torch.zeros(int(lib.et_graphtern_grad_floats(C.byref(params))), device=dev)
    d = T(CS.d_out(name, n), dev)
    out = torch.zeros((1, 6, n, 20), device=dev)
    assert lib.et_graphtern_backward_graph(C.byref(params), n, L.ptr(d), L.ptr(g), g.numel(), L.ptr(ws), 16, None) == 4
    assert lib.et_graphtern_backward_graph(C.byref(params), n, None, L.ptr(g), g.numel(), L.ptr(ws), ws.numel(), None) == 1
    assert lib.et_graphtern_backward_graph(C.byref(params), n, L.ptr(d), L.ptr(g), 3, L.ptr(ws), ws.numel(), None) == 1
    assert lib.et_graphtern_train_forward_graph(C.byref(params), L.ptr(ts), n, None, L.ptr(out), L.ptr(ws), 16, None) == 4
    assert lib.et_graphtern_train_forward_graph(C.byref(params), L.ptr(ts), n, None, None, L.ptr(ws), ws.numel(), None) == 1
    assert lib.et_graphtern_train_forward_graph(C.byref(params), L.ptr(ts), 513, None, L.ptr(out), L.ptr(ws), ws.numel(),
                                                None) == 1
    bad = m.et_params()[0]
    bad.n_epgcn = 2
    assert lib.et_graphtern_train_forward_graph(C.byref(bad), L.ptr(ts), n, None, L.ptr(out), L.ptr(ws), ws.numel(), None) == 3
    assert lib.et_graphtern_backward_graph(C.byref(bad), n, L.ptr(d), L.ptr(g), g.numel(), L.ptr(ws), ws.numel(), None) == 3
    torch.cuda.synchronize()
    assert torch.equal(ops.graphtern_forward_graph(m, ts), before) and not out.any() and not g.any()
