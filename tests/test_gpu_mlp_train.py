"""Native ET-LBEBM training on the GPU (csrc/et_mlp_train.hip, eigentrajectory_amd/lbebm.py): the training forward against the
eval-mode ``predict`` (bit for bit) and the float64 restatement (tests/_mlp_train_np.py); the backward pass against the
restatement run with the masks the native forward produced; uninitialised buffers, determinism, row independence, exact
zeros, the autograd contract under the wrapper and one ETTrainer step against the restatement and a torch-autograd twin.

Every tolerance is the restatement's elementwise bound (derived in its docstring), except the cross-check against torch's
own backward of the same chains (the twin), a loose 1e-4 of the tensor's largest entry.  The largest error / bound ratios
measured on an MI355X (the tests print them, ``pytest -s``) are in DESIGN.md section 4, "LBEBM training"."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from . import _golden as G
from . import _mlp_train_np as TN
from . import _pecnet_np as PN
from ._gpu_common import N_, T, dev, ops, synth  # noqa: F401 -- dev and ops are fixtures

pytestmark = pytest.mark.gpu
Z = G.load("g24_pecnet.npz")
GEN_N = [1, 2, 3, 5, 15, 16, 17, 33]  # the tile edge of 16 rows and the k step of 4 of the reduction over the rows
CASES = [("lbebm", 37)] + [("lbebm_gen", n) for n in GEN_N] + [("width1", 17), ("wide", 17)]
ZERO_UNITS = (("encoder_past", 0, 3), ("predictor", 1, 2))  # of lbebm_gen: weight row and bias set to zero
_SD, _NET, _REF = {}, {}, {}


def build(cfg):
    from eigentrajectory_amd import LBEBM
    args = dict(non_local_theta_size=[4], non_local_phi_size=[4], non_local_g_size=[4], non_local_dim=3, nonlocal_pools=0,
                sub_goal_indexes=[11], ny=1)
    if cfg == "width1":  # widths of 1 in every position: input 2 -> 1 -> 3 -> 1 | 2 -> 2 -> 1 -> 1 | 2 -> 1 -> 1 -> 2 -> 2
        return LBEBM([1, 3], [2, 1], [4], [4], [1, 1, 2], 1, 2, 1.3, 1, 1, args)
    if cfg == "wide":  # a 1024-wide layer as output and as input (the LDS image's edge), 4 hidden layers in the predictor
        return LBEBM([40, 1024], [1024, 9], [4], [4], [1024, 20, 7, 33], 6, 2, 1.3, 3, 5, args)
    if cfg == "gen_deleted":  # lbebm_gen without the two units of ZERO_UNITS
        return LBEBM([23, 12], [24, 12], [24, 12], [24, 12], [24, 11], 5, 3, 1.3, 2, 6,
                     args=dict(args, non_local_theta_size=[24, 12], non_local_phi_size=[24, 12], non_local_g_size=[24, 12],
                               non_local_dim=7, nonlocal_pools=2))
    return PN.native_module(cfg)


def sd_of(cfg):
    """the configuration's weights (numpy float32), generated once"""
    if cfg not in _SD:
        if cfg in ("lbebm", "lbebm_gen"):
            _SD[cfg] = PN.weights(Z, cfg)
        elif cfg == "gen_zero":
            sd = {k: v.copy() for k, v in sd_of("lbebm_gen").items()}
            for chain, layer, unit in ZERO_UNITS:
                sd[f"{chain}.layers.{layer}.weight"][unit] = 0.0
                sd[f"{chain}.layers.{layer}.bias"][unit] = 0.0
            _SD[cfg] = sd
        elif cfg == "gen_deleted":
            sd = {k: v.copy() for k, v in sd_of("gen_zero").items()}
            for chain, layer, unit in ZERO_UNITS:
                for kind in ("weight", "bias"):
                    sd[f"{chain}.layers.{layer}.{kind}"] = np.delete(sd[f"{chain}.layers.{layer}.{kind}"], unit, axis=0)
                sd[f"{chain}.layers.{layer + 1}.weight"] = np.delete(sd[f"{chain}.layers.{layer + 1}.weight"], unit, axis=1)
            _SD[cfg] = sd
        else:
            st = build(cfg).state_dict()
            _SD[cfg] = PN.make_weights(list(st), [tuple(v.shape) for v in st.values()], 20 + len(cfg), 1.0)
    return _SD[cfg]


def net(dev, cfg):
    """the native module with the configuration's weights, built once (tests that change it make their own: fresh)"""
    if cfg not in _NET:
        _NET[cfg] = fresh(dev, cfg)
    return _NET[cfg]


def fresh(dev, cfg):
    m = build("lbebm_gen" if cfg == "gen_zero" else cfg)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd_of(cfg).items()}, strict=True)
    return m.to(dev).eval()


def data(cfg, n, seed=0):
    """past (n, kp), dest (n, kd), g_out (n, out_width), float32; the first rows of a longer draw are the shorter draw"""
    sd = sd_of(cfg)
    kp, kd = sd["encoder_past.layers.0.weight"].shape[1], sd["encoder_dest.layers.0.weight"].shape[1]
    ow = sd[f"predictor.layers.{TN.n_layers(sd, 'predictor') - 1}.weight"].shape[0]
    rng = np.random.default_rng(1000 + seed)
    x = rng.standard_normal((64, kp + kd + ow)).astype(np.float32)[:n]
    assert n <= 64
    return np.ascontiguousarray(x[:, :kp]), np.ascontiguousarray(x[:, kp:kp + kd]), np.ascontiguousarray(x[:, kp + kd:])


def reference(cfg, n):
    """the float64 forward of the case, computed once and left alone"""
    if (cfg, n) not in _REF:
        past, dest, _ = data(cfg, n)
        _REF[cfg, n] = TN.forward(sd_of(cfg), past, dest)
    return _REF[cfg, n]


def layout(sd, n):
    """offsets (in floats) of `saved` / the workspace as include/eigentraj.h documents them -> feat offsets, {chain: [(offset,
    width) of a_1 .. a_{L-1}]}, total"""
    at = 0

    def take(w):
        nonlocal at
        here = at
        at += (n * w + 3) & ~3
        return here
    fdim = sd[f"encoder_past.layers.{TN.n_layers(sd, 'encoder_past') - 1}.weight"].shape[0]
    feat = [(take(fdim), fdim), (take(fdim), fdim)]
    hidden = {c: [(take(w), w) for w in (sd[f"{c}.layers.{i}.weight"].shape[0] for i in range(TN.n_layers(sd, c) - 1))]
              for c in TN.CHAINS}
    return feat, hidden, at


def blocks(flat, sd, n):
    """-> ([encoder outputs], {chain: [hidden blocks]}) as (n, width) numpy views of a flat saved / workspace tensor"""
    flat = N_(flat)
    feat, hidden, total = layout(sd, n)
    assert flat.size >= total
    cut = lambda o, w: flat[o:o + n * w].reshape(n, w)
    return [cut(o, w) for o, w in feat], {c: [cut(o, w) for o, w in hidden[c]] for c in hidden}


def as_views(dev, past, dest, transposed):
    """the inputs on the device: row-major, or as the bridge hands them over (the .T of a (k, N) array)"""
    if transposed:
        return T(past.T, dev).T, T(dest.T, dev).T
    return T(past, dev), T(dest, dev)


def raw(dev, m, sd, past, dest, g_out, fill, want_inputs=True):
    """both C entries through _lib.call with every buffer they write prefilled with ``fill`` -> dict of device tensors"""
    from eigentrajectory_amd import _lib as L
    params, _ = m.et_params()
    n = past.shape[0]
    nbytes = L.lib().et_lbebm_train_workspace_bytes(C.byref(params), n)
    assert nbytes == 4 * layout(sd, n)[2]
    new = lambda *shape: torch.full(shape, fill, device=dev, dtype=torch.float32)
    r = dict(out=new(n, params.out_width), saved=new(nbytes // 4), ws=new(nbytes // 4))
    st = (past.stride(0), past.stride(1), L.ptr(dest), dest.stride(0), dest.stride(1), n)
    L.call("et_lbebm_train_fwd", C.byref(params), L.ptr(past), *st, L.ptr(r["out"]), L.ptr(r["saved"]), None, 0, L.stream(dev))
    grads = L.LBEBMGrads()
    for name, p in zip(m.chain_parameter_names(), m.chain_parameters()):
        r[name] = new(*p.shape)
        chain, _, i, kind = name.split(".")
        getattr(getattr(grads, chain), "dw" if kind == "weight" else "db")[int(i)] = r[name].data_ptr()
    if want_inputs:
        r["past"], r["dest"] = new(*past.shape), new(*dest.shape)
    L.call("et_lbebm_train_bwd", C.byref(params), L.ptr(past), *st, L.ptr(r["saved"]), L.ptr(g_out), C.byref(grads),
           L.ptr(r.get("past")), L.ptr(r.get("dest")), L.ptr(r["ws"]), nbytes, L.stream(dev))
    return r


RATIO = {}


def within(kind, got, ref, err, what):
    """|got - ref| <= err elementwise (exact where the bound is 0); keeps the largest error / bound ratio per tensor kind
    (the parametrised tests clear the record first and print their own)"""
    d = np.abs(np.asarray(got, np.float64) - ref)
    assert np.isfinite(d).all(), what
    assert (d[err == 0] == 0).all(), what
    ratio = float((d[err > 0] / err[err > 0]).max()) if (err > 0).any() else 0.0
    RATIO[kind] = max(RATIO.get(kind, 0.0), ratio)
    assert ratio <= 1.0, (what, ratio)
    return ratio


def kind_of(name):
    return "dW" if name.endswith("weight") else "db" if name.endswith("bias") else "input gradient"


@pytest.mark.parametrize("cfg,n", CASES)
def test_forward_is_predict_bit_for_bit_and_keeps_the_activations(dev, ops, cfg, n):
    m, sd, f = net(dev, cfg), sd_of(cfg), reference(cfg, n)
    past, dest, _ = data(cfg, n)
    RATIO.clear()
    for transposed in (False, True):
        p, d = as_views(dev, past, dest, transposed)
        out, saved = ops.lbebm_train_fwd(m, p, d)
        assert torch.equal(out, m.predict(T(past, dev), T(dest, dev)))
        within("activation", N_(out), f["out"], f["out_err"], "out")
        feat, hidden = blocks(saved, sd, n)
        for a, c in zip(feat, ("encoder_past", "encoder_dest")):
            within("activation", a, f["z"][c][-1], f["z_err"][c][-1], c)
        for c in TN.CHAINS:
            for i, a in enumerate(hidden[c]):
                within("activation", a, f["acts"][c][i + 1], f["acts_err"][c][i + 1], (c, i))
                z, ez = f["z"][c][i], f["z_err"][c][i]
                assert (a >= 0).all() and (z[a == 0] <= ez[a == 0]).all() and (z[a > 0] > -ez[a > 0]).all(), (c, i)
    print(f"{cfg} n={n}: activation error / bound {RATIO['activation']:.3f}")


@pytest.mark.parametrize("cfg,n", CASES)
def test_backward_is_within_the_bound_of_the_restatement(dev, ops, cfg, n):
    m, sd = net(dev, cfg), sd_of(cfg)
    past, dest, g_out = data(cfg, n)
    first = None
    RATIO.clear()
    for transposed in (False, True):
        p, d = as_views(dev, past, dest, transposed)
        out, saved = ops.lbebm_train_fwd(m, p, d)
        g = ops.lbebm_train_bwd(m, p, d, saved, T(g_out, dev), need_input_grads=True)
        assert g["past"].stride() == p.stride() and g["dest"].stride() == d.stride()
        assert list(g) == m.chain_parameter_names() + ["past", "dest"]
        if first is None:
            masks = TN.masks_of(blocks(saved, sd, n)[1])
            b = TN.backward(sd, masks, past, dest, g_out)
            first = g
        for name in g:
            assert g[name].shape == b["grads"][name].shape and torch.equal(g[name], first[name]), name
            within(kind_of(name), N_(g[name]), b["grads"][name], b["grads_err"][name], name)
    only = ops.lbebm_train_bwd(m, p, d, saved, T(g_out, dev))  # without the input gradients: layer 0 is not run backward
    assert list(only) == m.chain_parameter_names() and all(torch.equal(only[k], first[k]) for k in only)
    one = ops.lbebm_train_bwd(m, p, d, saved, T(g_out, dev), need_input_grads=(False, True))
    assert "past" not in one and torch.equal(one["dest"], first["dest"])
    r = raw(dev, m, sd, T(past, dev), T(dest, dev), T(g_out, dev), 0.0)
    gfeat, gz = blocks(r["ws"], sd, n)
    for c, gf in zip(("encoder_past", "encoder_dest"), gfeat):
        within("g_z", gf, b["gz"][c][-1], b["gz_err"][c][-1], c)
    for c in TN.CHAINS:
        for i, z in enumerate(gz[c]):
            within("g_z", z, b["gz"][c][i], b["gz_err"][c][i], (c, i))
    print(f"{cfg} n={n}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(RATIO.items())))


def test_nothing_uninitialised_is_read(dev):
    cfg, n = "lbebm_gen", 17
    m, sd = net(dev, cfg), sd_of(cfg)
    past, dest, g_out = (T(a, dev) for a in data(cfg, n))
    zero, nan = (raw(dev, m, sd, past, dest, g_out, fill) for fill in (0.0, float("nan")))
    for key in zero:
        if key in ("saved", "ws"):  # the floats between two blocks (up to a multiple of 4) belong to nobody
            fa, ha = blocks(zero[key], sd, n)
            fb, hb = blocks(nan[key], sd, n)
            pairs = list(zip(fa, fb)) + [(x, y) for c in ha for x, y in zip(ha[c], hb[c])]
        else:
            pairs = [(N_(zero[key]), N_(nan[key]))]
        for x, y in pairs:
            assert not np.isnan(y).any(), key
            assert np.array_equal(x.view(np.int32), y.view(np.int32)), key


def test_no_rows(dev, ops):
    """N = 0: the forward has nothing to do, the backward overwrites every dW and db with zeros (one launch)"""
    m = net(dev, "lbebm_gen")
    past, dest = torch.empty((0, 4), device=dev), torch.empty((0, 2), device=dev)
    out, saved = ops.lbebm_train_fwd(m, past, dest)
    assert out.shape == (0, 12) and saved.numel() == 0
    g = ops.lbebm_train_bwd(m, past, dest, saved, torch.empty((0, 12), device=dev), need_input_grads=True)
    assert g["past"].shape == (0, 4) and g["dest"].shape == (0, 2)
    for name, p in zip(m.chain_parameter_names(), m.chain_parameters()):
        assert g[name].shape == p.shape and not bool(g[name].any()), name


def test_determinism_and_row_independence(dev):
    cfg = "lbebm_gen"
    m, sd = net(dev, cfg), sd_of(cfg)
    past, dest, g_out = data(cfg, 33)
    r17, again = (raw(dev, m, sd, T(past[:17], dev), T(dest[:17], dev), T(g_out[:17], dev), 0.0) for _ in range(2))
    assert all(torch.equal(r17[k], again[k]) for k in r17)
    r33 = raw(dev, m, sd, T(past, dev), T(dest, dev), T(g_out, dev), 0.0)
    assert torch.equal(r33["past"][:17], r17["past"]) and torch.equal(r33["dest"][:17], r17["dest"])
    assert torch.equal(r33["out"][:17], r17["out"])
    for key in ("saved", "ws"):
        fa, ha = blocks(r17[key], sd, 17)
        fb, hb = blocks(r33[key], sd, 33)
        for x, y in list(zip(fa, fb)) + [(x, y) for c in ha for x, y in zip(ha[c], hb[c])]:
            assert np.array_equal(x, y[:17]), key
    assert not torch.equal(r33["predictor.layers.0.weight"], r17["predictor.layers.0.weight"])  # 16 more rows count
    g0 = g_out.copy()
    g0[17:] = 0.0
    rz = raw(dev, m, sd, T(past, dev), T(dest, dev), T(g0, dev), 0.0)
    for name in m.chain_parameter_names():  # rows without an output gradient add exact zeros to every sum over the rows
        assert torch.equal(rz[name], r17[name]), name


def test_exact_zeros_flow_through_a_dead_unit(dev):
    """a hidden unit whose weight row and bias are zero has z = 0 exactly: no gradient passes it (torch's convention), its
    dW row, its db and its column of the next layer's dW are exactly 0, and every other value is what the network without
    that unit gives, bit for bit (adding an exact zero changes no fmaf chain)"""
    n = 17
    a, b = fresh(dev, "gen_zero"), fresh(dev, "gen_deleted")
    past, dest, g_out = (T(x, dev) for x in data("lbebm_gen", n))
    ra, rb = raw(dev, a, sd_of("gen_zero"), past, dest, g_out, 0.0), raw(dev, b, sd_of("gen_deleted"), past, dest, g_out, 0.0)
    assert torch.equal(ra["out"], rb["out"]) and torch.equal(ra["past"], rb["past"]) and torch.equal(ra["dest"], rb["dest"])
    cut = {}
    for chain, layer, unit in ZERO_UNITS:
        w, bias, nxt = (f"{chain}.layers.{layer}.weight", f"{chain}.layers.{layer}.bias", f"{chain}.layers.{layer + 1}.weight")
        assert float(ra[w][unit].abs().max()) == 0.0 and float(ra[bias][unit]) == 0.0
        assert float(ra[nxt][:, unit].abs().max()) == 0.0
        cut.update({w: (unit, 0), bias: (unit, 0), nxt: (unit, 1)})
    for name in a.chain_parameter_names():
        got = N_(ra[name])
        if name in cut:
            got = np.delete(got, cut[name][0], axis=cut[name][1])
        assert np.array_equal(got, N_(rb[name])), name
    _, gz = blocks(ra["ws"], sd_of("gen_zero"), n)
    for chain, layer, unit in ZERO_UNITS:
        assert (gz[chain][layer][:, unit] == 0).all()


class Twin:
    """mixin: ``predict`` as the same chains in F.linear + relu under torch autograd"""

    def predict(self, past, dest):
        def chain(mlp, x):
            for i, lin in enumerate(mlp.layers):
                x = F.linear(x, lin.weight, lin.bias)
                if i + 1 < len(mlp.layers):
                    x = torch.relu(x)
            return x
        return chain(self.predictor, torch.cat([chain(self.encoder_past, past), chain(self.encoder_dest, dest)], dim=1))


def wrapper(dev, cfg, twin=False, **hp_kw):
    """EigenTrajectory(LBEBM, lbebm hooks) whose model_forward also records the bridge's inputs and the gradient that
    arrives at predict's output -> (model, record)"""
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    base = fresh(dev, cfg)
    if twin:
        base.__class__ = type("TwinLBEBM", (Twin, base.__class__), {})
    else:
        base.enable_native_training()
    hooks, rec = get_hook_func("lbebm"), {}
    call = hooks.model_forward

    def forward(net_in, baseline_model):
        out = call(net_in, baseline_model)
        rec["past"], rec["dest"] = net_in
        if out.requires_grad:
            out.register_hook(lambda g: rec.__setitem__("g_out", g.clone()))
        return out
    hooks.model_forward = forward
    return EigenTrajectory(base, hooks, default_hyper_params(static_dist=0.3, **hp_kw)).to(dev), rec


def test_autograd_contract_under_the_wrapper(dev, ops):
    cfg = "lbebm"
    model, rec = wrapper(dev, cfg)
    obs, pred = (T(a, dev) for a in synth(600, seed=3))
    model.calculate_parameters(obs, pred)
    m = model.baseline_model
    names = m.chain_parameter_names()
    so, sp = (T(a, dev) for a in synth(9, seed=4))
    model.train()
    so.requires_grad_(False)
    out = model(so, sp, addl_info={"num_samples": 20})
    loss = out["loss_eigentraj"] + out["loss_euclidean_ade"] + out["loss_euclidean_fde"]
    assert bool(torch.isfinite(loss))
    loss.backward(retain_graph=True)
    past, dest, g_out = rec["past"], rec["dest"], rec["g_out"]
    assert not past.is_contiguous() and past.shape == (9, 6) and g_out.shape == (9, 120)  # the bridge's .T view
    grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    assert sorted(grads) == sorted(names)  # the three chains and nothing else: predict does not touch the rest
    _, saved = ops.lbebm_train_fwd(m, past, dest)
    direct = ops.lbebm_train_bwd(m, past, dest, saved, g_out)
    assert all(torch.equal(grads[k], direct[k]) for k in names)
    # at these widths the running bound is far wider than the values (|W| of a 1024-wide layer amplifies it ~16x per layer),
    # so the ET configuration is also held against torch's own backward: the cross-check's 1e-4 of the largest entry
    tw = fresh(dev, cfg)
    tw.__class__ = type("TwinLBEBM", (Twin, tw.__class__), {})
    tw.predict(past, dest).backward(g_out)
    for k in names:
        ref = tw.get_parameter(k).grad
        assert float((grads[k] - ref).abs().max()) <= 1e-4 * float(ref.abs().max()), k
    loss.backward()  # no zero_grad in between: autograd accumulates
    assert all(torch.equal(m.get_parameter(k).grad, 2 * grads[k]) for k in names)
    # the gradient of an input that asks for one
    p2 = past.detach().clone().requires_grad_(True)
    out2 = m.predict(p2, dest)
    assert out2.requires_grad and torch.equal(out2.detach(), m.eval().predict(past, dest))
    m.train()
    out2.backward(g_out)
    sd = sd_of(cfg)
    b = TN.backward(sd, TN.masks_of(blocks(saved, sd, 9)[1]), N_(past), N_(dest), N_(g_out))
    print("input gradient error / bound", within("input gradient", N_(p2.grad), b["grads"]["past"], b["grads_err"]["past"], "past"))
    # an optimiser step between forward and backward is caught: the kernels read the weights in place
    out3 = m.predict(past, dest)
    with torch.no_grad():
        m.predictor.layers[0].bias.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out3.backward(g_out)
    with torch.no_grad():
        assert m.predict(past, dest).requires_grad is False
    model.eval()
    assert m.predict(past, dest).requires_grad is False  # eval mode: the inference path, whatever the flag


def scenes_data(sizes, seed):
    from eigentrajectory_amd.data import TrajectoryData
    obs, pred = synth(sum(sizes), seed=seed)
    ends = np.cumsum(sizes)
    return TrajectoryData.from_arrays(obs, pred, [(int(e - s), int(e)) for e, s in zip(ends, sizes)])


def trainer(dev, twin, like=None):
    """a collated ETTrainer on six synthetic scenes around lbebm_gen (k = 4, S = 3); ``like``: take the fitted descriptors
    and anchors (and the weights) from that trainer instead of fitting again"""
    from eigentrajectory_amd.trainer import ETTrainer
    model, rec = wrapper(dev, "lbebm_gen", twin, k=4, num_samples=3, batch_size=16, lr=1e-3, weight_decay=1e-4, clip_grad=10,
                         lr_schd=False)
    train = scenes_data([3, 20, 7, 12, 5, 9], seed=11)
    tr = ETTrainer(model, model.hyper_params, train, scenes_data([4, 6], seed=12), scenes_data([5, 3], seed=13),
                   mode="collated", device=dev)
    if like is None:
        tr.init_descriptor()
    else:
        model.load_state_dict(like.model.state_dict(), strict=True)
    return tr, rec


def test_one_trainer_step_and_one_epoch(dev, ops):
    tr, rec = trainer(dev, twin=False)
    tw, _ = trainer(dev, twin=True, like=tr)
    m, names, sd = tr.predictor, tr.predictor.chain_parameter_names(), sd_of("lbebm_gen")
    batch = [1, 3]  # two scenes, 32 pedestrians: two tiles
    tr.model.train()
    tw.model.train()
    loss = tr._train_batch(tr.train_data, batch)
    loss_tw = tw._train_batch(tw.train_data, batch)
    assert np.isfinite(loss) and abs(loss - loss_tw) <= 1e-4 * abs(loss_tw)
    past, dest, g_out = N_(rec["past"]), N_(rec["dest"]), N_(rec["g_out"])
    assert past.shape == (32, 4)
    _, saved = ops.lbebm_train_fwd(m, rec["past"], rec["dest"])
    b = TN.backward(sd, TN.masks_of(blocks(saved, sd, 32)[1]), past, dest, g_out)
    for name in names:
        got = N_(m.get_parameter(name).grad)
        within(kind_of(name), got, b["grads"][name], b["grads_err"][name], name)
        ref = N_(tw.predictor.get_parameter(name).grad)
        assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max(), name
    assert all(p.grad is None for k, p in m.named_parameters() if k not in names)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    assert np.isfinite(tr.train(0))
    after = m.state_dict()
    for k in before:
        assert torch.equal(before[k], after[k]) == (k not in names), k  # the three chains moved, nothing else did
    assert np.isfinite(tr.valid()) and not m.training
    res = tr.test()
    assert np.isfinite(res["ADE"]) and np.isfinite(res["FDE"])
