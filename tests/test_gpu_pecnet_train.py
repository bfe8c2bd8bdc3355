"""Native ET-PECNet training on the GPU (csrc/et_mlp_train.hip, eigentrajectory_amd/pecnet.py): the training forward against
the eval-mode ``predict`` (bit for bit) and the float64 restatement (tests/_pecnet_train_np.py); the backward pass against the
restatement run with the ReLU masks the native forward produced; uninitialised buffers, determinism, N = 0, an all-zero mask
row, the shared weights' sum over the rounds, the autograd contract under the wrapper and one ETTrainer step and a two-epoch
fit against a torch-autograd twin.

Three yardsticks.  (1) The restatement's RUNNING bound (derived in its docstring) holds for every kept value and every
gradient; behind the 16-fold scaled theta / phi layers of the fixture it is sharp before the first softmax only and grows
past the values after the second round, so it is joined by (2) the STAGE bound: every pooling round forward, and round 0
and the last round backward, restated from the inputs the kernels themselves kept (``pool_stage``: that step's own rounding, a few 1e-5 to
3e-2 of a tensor's scale), and (3) torch's own backward of the same network on the GPU (the twin), the project's 1e-4 of each
tensor's largest entry (one exception, derived at ``near_twin``: the last bias gradient of non_local_phi is exactly 0 in
exact arithmetic, for every mask, and is held to 1e-4 of the largest of the terms it sums).  The largest error / bound ratios measured on an MI355X (the tests print them, ``pytest -s``) are in
DESIGN.md section 4, "PECNet training"."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from . import _golden as G
from . import _mlp_train_np as TN
from . import _pecnet_np as PN
from . import _pecnet_train_np as PT
from ._gpu_common import N_, T, dev, ops, synth  # noqa: F401 -- dev and ops are fixtures

pytestmark = pytest.mark.gpu
Z = G.load("g24_pecnet.npz")
GEN_N = [1, 2, 3, 5, 15, 16, 17, 33, 64, 65]  # the 16-row tile, the k step of 4, the wavefront's 64 columns, 4 rows per block
SCENES = (1, 3, 16, 13)  # collated scenes of the block mask, N = 33
CASES = ([("pecnet_gen", n, "ones") for n in GEN_N] +
         [("pecnet_gen", 33, "blocks"), ("pecnet_gen", 33, "blocks_bool"), ("pecnet_gen", 17, "zero_row"),
          ("pecnet_gen", 17, "fractional"), ("pecnet_gen", 17, "none"), ("gen_pools0", 17, "ones"), ("gen_pools1", 17, "ones"),
          ("gen_pools3", 17, "ones"), ("pecnet", 37, "ones"), ("width1", 17, "ones")])
_SD, _NET = {}, {}


def build(cfg):
    from eigentrajectory_amd import PECNet
    if cfg.startswith("gen_pools"):  # pecnet_gen's shapes and weights, another number of rounds
        g = PN.GEN
        return PECNet(g, g, g, g, g, g, g, g, 5, 3, int(cfg[-1]), 7, 1.3, 2, 7, False)
    if cfg == "width1":  # widths of 1 in every position; F = 4, non_local_dim 1, two rounds
        return PECNet([1, 3], [2, 1], [4], [4], [1, 1, 2], [1], [2], [1, 1], 1, 2, 2, 1, 1.3, 1, 2, False)
    return PN.native_module(cfg)


def sd_of(cfg):
    if cfg not in _SD:
        if cfg in ("pecnet", "pecnet_gen"):
            _SD[cfg] = PN.weights(Z, cfg)
        elif cfg.startswith("gen_pools"):
            _SD[cfg] = sd_of("pecnet_gen")
        else:
            st = build(cfg).state_dict()
            _SD[cfg] = PN.make_weights(list(st), [tuple(v.shape) for v in st.values()], 20 + len(cfg), 1.0)
    return _SD[cfg]


def fresh(dev, cfg):
    m = build(cfg)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd_of(cfg).items()}, strict=True)
    return m.to(dev).eval()


def net(dev, cfg):
    if cfg not in _NET:
        _NET[cfg] = fresh(dev, cfg)
    return _NET[cfg]


def widths(sd, chain):
    return [sd[f"{chain}.layers.0.weight"].shape[1]] + [sd[f"{chain}.layers.{i}.weight"].shape[0]
                                                        for i in range(TN.n_layers(sd, chain))]


def data(cfg, n, seed=0):
    """past (n, kp), dest (n, 2), pos (n, 2), g_out (n, out_width), float32"""
    sd = sd_of(cfg)
    kp, ow = widths(sd, "encoder_past")[0], widths(sd, "predictor")[-1]
    x = np.random.default_rng(2000 + seed).standard_normal((65, kp + 4 + ow)).astype(np.float32)[:n]
    assert n <= 65
    return tuple(np.ascontiguousarray(a) for a in (x[:, :kp], x[:, kp:kp + 2], x[:, kp + 2:kp + 4], x[:, kp + 4:]))


def mask_of(kind, n):
    """-> (what predict is given, the float64 mask the restatement takes)"""
    if kind == "none":
        return None, np.ones((n, n))
    m = np.ones((n, n), np.float32)
    if kind.startswith("blocks"):
        assert n == sum(SCENES)
        m[:] = 0
        lo = 0
        for s in SCENES:
            m[lo:lo + s, lo:lo + s] = 1
            lo += s
    elif kind == "zero_row":
        m[n // 2] = 0
    elif kind == "fractional":
        m = (0.25 + 0.75 * np.random.default_rng(5).random((n, n))).astype(np.float32)
        m[n // 2, n // 3] = -0.5
    return (m.astype(bool) if kind.endswith("bool") else m), m.astype(np.float64)


def layout(sd, n, pools, workspace):
    """offsets (in floats) of `saved` / the workspace as csrc/et_mlp_train.hip documents them -> dict name -> (offset, rows,
    width); ``total``"""
    at, out = 0, {}

    def take(name, rows, w):
        nonlocal at
        out[name] = (at, rows, w)
        at += (rows * w + 3) & ~3
    fdim, Fw = widths(sd, "encoder_past")[-1], widths(sd, "predictor")[0]
    take("ftraj", n, fdim), take("dfeat", n, fdim)
    for c in TN.CHAINS:
        for i, w in enumerate(widths(sd, c)[1:-1]):
            take((c, i), n, w)
    if pools:
        D = widths(sd, "non_local_theta")[-1]
        if workspace:
            take("G", n, Fw)
            for c in PT.POOLED:
                take(("part", c), n, Fw)
        else:
            take("feat", (pools + 1) * n, Fw)
        for c, w in zip(PT.POOLED, (D, D, Fw)):
            take(("out", c), pools * n, w)
        for c in PT.POOLED:
            for i, w in enumerate(widths(sd, c)[1:-1]):
                take((c, i), pools * n, w)
        if workspace:
            take("p", n, n), take("df", n, n)
    out["total"] = at
    return out


def blocks(flat, sd, n, pools, workspace=False):
    """name -> (rows, width) numpy view of a flat saved / workspace tensor"""
    flat, lay = N_(flat), layout(sd, n, pools, workspace)
    assert flat.size >= lay["total"]
    return {k: flat[v[0]:v[0] + v[1] * v[2]].reshape(v[1], v[2]) for k, v in lay.items() if k != "total"}


def hidden_of(bl, sd, pools):
    """{chain: [a_1 .. a_{L-1}]} as the restatement's backward takes the masks"""
    chains = PT.CHAINS if pools else TN.CHAINS
    return {c: [bl[c, i] for i in range(TN.n_layers(sd, c) - 1)] for c in chains}


def as_views(dev, arrays, transposed):
    """the inputs on the device: row-major, or as the bridge hands them over (the .T of a (k, N) array)"""
    return tuple(T(a.T, dev).T if transposed else T(a, dev) for a in arrays)


def raw(dev, m, sd, past, dest, pos, mask, g_out, fill, want_inputs=True):
    """both C entries through _lib.call with every buffer they write prefilled with ``fill`` -> dict of device tensors"""
    from eigentrajectory_amd import _lib as L
    params, _ = m.et_params()
    n, pools = past.shape[0], m.nonlocal_pools
    sbytes = L.lib().et_pecnet_train_saved_bytes(C.byref(params), n)
    wbytes = L.lib().et_pecnet_train_workspace_bytes(C.byref(params), n)
    assert sbytes == 4 * layout(sd, n, pools, False)["total"] and wbytes == 4 * layout(sd, n, pools, True)["total"]
    new = lambda *shape: torch.full(shape, fill, device=dev, dtype=torch.float32)
    r = dict(out=new(n, params.out_width), saved=new(sbytes // 4), ws=new(wbytes // 4))
    st = []
    for t in (past, dest, pos):
        st += [L.ptr(t), t.stride(0), t.stride(1)]
    L.call("et_pecnet_train_fwd", C.byref(params), *st, L.ptr(mask), n, L.ptr(r["out"]), L.ptr(r["saved"]), None, 0,
           L.stream(dev))
    grads = L.PECNetGrads()
    for name, p in zip(m.chain_parameter_names(), m.chain_parameters()):
        chain, _, i, kind = name.split(".")
        if pools == 0 and chain in PT.POOLED:
            continue
        r[name] = new(*p.shape)
        getattr(getattr(grads, chain), "dw" if kind == "weight" else "db")[int(i)] = r[name].data_ptr()
    if want_inputs:
        r["past"], r["dest"], r["pos"] = new(*past.shape), new(*dest.shape), new(*pos.shape)
    L.call("et_pecnet_train_bwd", C.byref(params), *st, L.ptr(mask), n, L.ptr(r["saved"]), L.ptr(g_out), C.byref(grads),
           L.ptr(r.get("past")), L.ptr(r.get("dest")), L.ptr(r.get("pos")), L.ptr(r["ws"]), wbytes, L.stream(dev))
    return r


RATIO = {}


def within(kind, got, ref, err, what):
    """|got - ref| <= err elementwise (exact where the bound is 0); keeps the largest error / bound ratio per tensor kind"""
    d = np.abs(np.asarray(got, np.float64) - ref)
    assert np.isfinite(d).all(), what
    assert (d[err == 0] == 0).all(), what
    ratio = float((d[err > 0] / err[err > 0]).max()) if (err > 0).any() else 0.0
    RATIO[kind] = max(RATIO.get(kind, 0.0), ratio)
    assert ratio <= 1.0, (what, ratio)
    return ratio


def kind_of(name):
    return "dW" if name.endswith("weight") else "db" if name.endswith("bias") else "input gradient"


def ratios():
    return ", ".join(f"{k} {v:.3f}" for k, v in sorted(RATIO.items()))


def chain_t(mlp, x):
    for i, lin in enumerate(mlp.layers):
        x = F.linear(x, lin.weight, lin.bias)
        if i + 1 < len(mlp.layers):
            x = torch.relu(x)
    return x


class Twin:
    """mixin: ``predict`` as the reference's formula in stock torch ops under torch autograd"""

    def predict(self, past, dest, mask, pos):
        feat = torch.cat([chain_t(self.encoder_past, past), chain_t(self.encoder_dest, dest), pos], dim=1)
        self.phi_outs = []  # phi of every round; their .grad after the backward: the terms phi's last bias gradient sums
        for _ in range(self.nonlocal_pools):
            phi = chain_t(self.non_local_phi, feat)
            if phi.requires_grad:
                phi.retain_grad()
                self.phi_outs.append(phi)
            f = torch.matmul(chain_t(self.non_local_theta, feat), phi.transpose(1, 0))
            w = F.softmax(f, dim=-1)
            if mask is not None:
                w = w * mask
            w = F.normalize(w, p=1, dim=1)
            feat = torch.matmul(w, chain_t(self.non_local_g, feat)) + feat
        return chain_t(self.predictor, feat)


def twin_of(m):
    tw = type("TwinPECNet", (Twin, m.__class__), {})
    return tw


def twin_grads(dev, cfg, past, dest, mask, pos, g_out):
    """torch's own backward of the same network with the same weights -> gradients by name (+ past, dest, pos), and the
    largest entry of the gradient at phi's outputs (``phi_terms`` of :func:`near_twin`)"""
    tw = fresh(dev, cfg)
    tw.__class__ = twin_of(tw)
    p, d, q = (t.detach().clone().requires_grad_(True) for t in (past, dest, pos))
    tw.predict(p, d, None if mask is None else mask.float(), q).backward(g_out)
    g = {k: v.grad for k, v in tw.named_parameters() if v.grad is not None}
    g.update(past=p.grad, dest=d.grad, pos=q.grad)
    return g, phi_terms_of(tw)


def phi_terms_of(twin):
    return max((float(t.grad.abs().max()) for t in twin.phi_outs), default=0.0)


def near_twin(got, ref, phi_terms):
    """every tensor of ``ref`` (name -> tensor): ``got``'s is within 1e-4 of ITS OWN largest entry.  One exception, the last
    bias gradient of non_local_phi.  It is sum_j d phi_j = sum_i (sum_j d f_ij) theta_i over the rows of every round, and
    sum_j d f_ij = sum_j s_ij ds_ij - (sum_k ds_ik s_ik)(sum_j s_ij) = 0 because a softmax row sums to 1: whatever the mask,
    the tensor is exactly 0 in exact arithmetic and holds rounding only, in torch and in the kernels, so "its largest entry"
    is no scale.  It is held to 1e-4 of the largest entry of the terms it sums, the gradient at phi's outputs
    (``phi_terms``, from the twin)."""
    layers = [int(k.split(".")[2]) for k in ref if k.startswith("non_local_phi.")]
    cancels = f"non_local_phi.layers.{max(layers)}.bias" if layers else None
    for name, r in ref.items():
        scale = phi_terms if name == cancels else float(r.abs().max())
        assert float((got[name] - r).abs().max()) <= 1e-4 * scale, name


def check_forward(sd, f, saved_blocks, pools, mask64):
    for key, c in (("ftraj", "encoder_past"), ("dfeat", "encoder_dest")):
        within("activation", saved_blocks[key], f["z"][c][-1], f["z_err"][c][-1], c)
    for c in TN.CHAINS:
        for i in range(TN.n_layers(sd, c) - 1):
            within("activation", saved_blocks[c, i], f["acts"][c][i + 1], f["acts_err"][c][i + 1], (c, i))
    if not pools:
        return
    n = f["out"].shape[0]
    rows = lambda a, r: a[r * n:(r + 1) * n]
    for r in range(pools + 1):
        within("features", rows(saved_blocks["feat"], r), f["feat"][r], f["feat_err"][r], ("feat", r))
    for r in range(pools):
        for c in PT.POOLED:
            within("theta / phi / g", rows(saved_blocks["out", c], r), f["z"][c][r][-1], f["z_err"][c][r][-1], (c, r))
            for i in range(TN.n_layers(sd, c) - 1):
                within("activation", rows(saved_blocks[c, i], r), f["acts"][c][r][i + 1], f["acts_err"][c][r][i + 1], (c, r, i))
        # the round restated from what the kernels kept: its own rounding only
        th, ph, g = (rows(saved_blocks["out", c], r) for c in PT.POOLED)
        rd, _ = PT.pool_stage(th, ph, g, rows(saved_blocks["feat"], r), mask64)
        assert not rd["unsure"].any()
        within("stage: pooled features", rows(saved_blocks["feat"], r + 1), rd["out"], rd["eout"], ("stage", r))


@pytest.mark.parametrize("cfg,n,kind", CASES)
def test_forward_is_predict_bit_for_bit_and_keeps_what_the_backward_needs(dev, ops, cfg, n, kind):
    m, sd, pools = net(dev, cfg), sd_of(cfg), net(dev, cfg).nonlocal_pools
    past, dest, pos, _ = data(cfg, n)
    mask, mask64 = mask_of(kind, n)
    mask_t = None if mask is None else T(mask, dev)
    f = PT.forward(sd, past, dest, pos, mask64, pools)
    RATIO.clear()
    for transposed in (False, True):
        p, d, q = as_views(dev, (past, dest, pos), transposed)
        out, saved = ops.pecnet_train_fwd(m, p, d, mask_t, q)
        assert torch.equal(out, m.predict(T(past, dev), T(dest, dev), mask_t, T(pos, dev)))
        within("activation", N_(out), f["out"], f["out_err"], "out")
        check_forward(sd, f, blocks(saved, sd, n, pools), pools, mask64)
    print(f"RATIO forward {cfg} n={n} {kind}: error / bound " + ratios())


@pytest.mark.parametrize("cfg,n,kind", CASES)
def test_backward_is_within_the_bounds_and_near_torch(dev, ops, cfg, n, kind):
    m, sd, pools = net(dev, cfg), sd_of(cfg), net(dev, cfg).nonlocal_pools
    past, dest, pos, g_out = data(cfg, n)
    mask, mask64 = mask_of(kind, n)
    mask_t = None if mask is None else T(mask, dev)
    names = [k for k in m.chain_parameter_names() if pools or k.split(".")[0] not in PT.POOLED]
    first = None
    RATIO.clear()
    for transposed in (False, True):
        p, d, q = as_views(dev, (past, dest, pos), transposed)
        out, saved = ops.pecnet_train_fwd(m, p, d, mask_t, q)
        g = ops.pecnet_train_bwd(m, p, d, mask_t, q, saved, T(g_out, dev), need_input_grads=True)
        assert all(g[k].stride() == t.stride() for k, t in (("past", p), ("dest", d), ("pos", q)))
        assert list(g) == names + ["past", "dest", "pos"]
        if first is None:
            bl = blocks(saved, sd, n, pools)
            b = PT.backward(sd, TN.masks_of(hidden_of(bl, sd, pools)), past, dest, pos, mask64, pools, g_out)
            first = g
        for name in g:  # (the two layouts of the inputs: the same bits)
            assert g[name].shape == b["grads"][name].shape and torch.equal(g[name], first[name]), name
            within(kind_of(name), N_(g[name]), b["grads"][name], b["grads_err"][name], name)
    tw, phi_terms = twin_grads(dev, cfg, T(past, dev), T(dest, dev), mask_t, T(pos, dev), T(g_out, dev))
    assert sorted(tw) == sorted(first)
    near_twin(first, tw, phi_terms)
    only = ops.pecnet_train_bwd(m, p, d, mask_t, q, saved, T(g_out, dev))  # without the input gradients
    assert list(only) == names and all(torch.equal(only[k], first[k]) for k in only)
    one = ops.pecnet_train_bwd(m, p, d, mask_t, q, saved, T(g_out, dev), need_input_grads=(False, True, False))
    assert "past" not in one and "pos" not in one and torch.equal(one["dest"], first["dest"])
    # the workspace: g_z of every chain, and round 0's pooling backward restated from what the kernels kept
    r = raw(dev, m, sd, T(past, dev), T(dest, dev), T(pos, dev), None if mask is None else T(mask, dev).float(),
            T(g_out, dev), 0.0)
    assert all(torch.equal(r[k], first[k]) for k in first)
    ws = blocks(r["ws"], sd, n, pools, workspace=True)
    for key, c in (("ftraj", "encoder_past"), ("dfeat", "encoder_dest")):
        within("g_z", ws[key], b["gz"][c][-1], b["gz_err"][c][-1], c)
    for c in (PT.CHAINS if pools else TN.CHAINS):
        for i in range(TN.n_layers(sd, c) - 1):
            within("g_z", ws[c, i], b["gz"][c][i], b["gz_err"][c][i], (c, i))
    if pools:
        for c, key in zip(PT.POOLED, ("dtheta", "dphi", "dg")):
            within("g_z", ws["out", c], b["gz"][c][-1], b["gz_err"][c][-1], key)
        within("feature gradient", ws["G"], b["gfeat"][1], b["gfeat_err"][1], "G")  # at round 0's output
        th, ph, g0 = (bl["out", c][:n] for c in PT.POOLED)
        rd, pb = PT.pool_stage(th, ph, g0, bl["feat"][:n], mask64, ws["G"])
        assert not rd["unsure"].any()
        for key, got in (("p", ws["p"]), ("df", ws["df"]), ("dtheta", ws["out", "non_local_theta"][:n]),
                         ("dphi", ws["out", "non_local_phi"][:n]), ("dg", ws["out", "non_local_g"][:n])):
            ref, err = (rd if key == "p" else pb)[key], (rd if key == "p" else pb)["e" + key]
            within("stage: " + key, got, ref, err, ("stage", key))
    if pools > 1:
        # the LAST round's pooling backward, the first one run: its G is the predictor's input gradient, which the kernels do
        # not keep past the next round -- restated from the kept g_z(1) of the predictor (one product over its first layer's
        # outputs, with that product's own bound), then the stage as above; d theta, d phi, d g of every round are kept
        last = pools - 1
        gz1 = ws["predictor", 0].astype(np.float64)
        w0 = sd["predictor.layers.0.weight"].astype(np.float64)
        G_last, eG = TN._dot(gz1, np.zeros_like(gz1), w0, np.zeros_like(w0))
        rows = slice(last * n, (last + 1) * n)
        th, ph, g0 = (bl["out", c][rows] for c in PT.POOLED)
        rd, pb = PT.pool_stage(th, ph, g0, bl["feat"][rows], mask64, G_last, eG)
        assert not rd["unsure"].any()
        for key, c in (("dtheta", "non_local_theta"), ("dphi", "non_local_phi"), ("dg", "non_local_g")):
            within("stage, last round: " + key, ws["out", c][rows], pb[key], pb["e" + key], ("stage", last, key))
    print(f"RATIO backward {cfg} n={n} {kind}: error / bound " + ratios())


def test_nothing_uninitialised_is_read_and_two_runs_agree(dev):
    cfg, n = "pecnet_gen", 17
    m, sd = net(dev, cfg), sd_of(cfg)
    past, dest, pos, g_out = (T(a, dev) for a in data(cfg, n))
    mask = T(mask_of("fractional", n)[0], dev)
    zero, nan, again = (raw(dev, m, sd, past, dest, pos, mask, g_out, fill) for fill in (0.0, float("nan"), 0.0))
    for key in zero:
        if key in ("saved", "ws"):  # the floats between two blocks (up to a multiple of 4) belong to nobody
            a, b_, c = (blocks(r[key], sd, n, 2, key == "ws") for r in (zero, nan, again))
            triples = [(a[k], b_[k], c[k]) for k in a]
        else:
            triples = [(N_(zero[key]), N_(nan[key]), N_(again[key]))]
        for x, y, z in triples:
            assert not np.isnan(y).any(), key
            assert np.array_equal(x.view(np.int32), y.view(np.int32)) and np.array_equal(x.view(np.int32), z.view(np.int32)), key


def test_no_rows(dev, ops):
    """N = 0: the forward has nothing to do, the backward overwrites every dW and db with zeros (one launch)"""
    m = net(dev, "pecnet_gen")
    e = lambda w: torch.empty((0, w), device=dev)
    out, saved = ops.pecnet_train_fwd(m, e(4), e(2), torch.empty((0, 0), device=dev), e(2))
    assert out.shape == (0, 12) and saved.numel() == 0
    g = ops.pecnet_train_bwd(m, e(4), e(2), None, e(2), saved, e(12), need_input_grads=True)
    assert g["past"].shape == (0, 4) and g["dest"].shape == (0, 2) and g["pos"].shape == (0, 2)
    for name, p in zip(m.chain_parameter_names(), m.chain_parameters()):
        assert g[name].shape == p.shape and not bool(g[name].any()), name


def test_an_all_zero_mask_row_gives_exact_zeros(dev):
    cfg, n = "pecnet_gen", 17
    m, sd = net(dev, cfg), sd_of(cfg)
    past, dest, pos, g_out = (T(a, dev) for a in data(cfg, n))
    row = n // 2
    r = raw(dev, m, sd, past, dest, pos, T(mask_of("zero_row", n)[0], dev), g_out, float("nan"))
    for key, v in r.items():
        if key not in ("saved", "ws"):
            assert bool(torch.isfinite(v).all()), key
    ws, sv = blocks(r["ws"], sd, n, 2, True), blocks(r["saved"], sd, n, 2)
    assert all(np.isfinite(v).all() for v in ws.values()) and all(np.isfinite(v).all() for v in sv.values())
    assert (ws["p"][row] == 0).all() and (ws["df"][row] == 0).all()  # round 0's
    assert (ws["out", "non_local_theta"].reshape(2, n, -1)[:, row] == 0).all()  # d theta of the row, both rounds
    feat = sv["feat"].reshape(3, n, -1)
    assert np.array_equal(feat[0, row], feat[1, row]) and np.array_equal(feat[1, row], feat[2, row])  # p = 0: feat passes
    # the row adds exactly nothing to d phi and d g: the same bits as with its output gradient's pooled part removed, i.e.
    # as a run whose G row is anything -- here: d g is p^T G, and column sums over the other rows only
    others = np.delete(np.arange(n), row)
    dg = (ws["p"][others].astype(np.float64).T @ ws["G"][others].astype(np.float64))
    assert np.abs(ws["out", "non_local_g"][:n] - dg).max() <= 1e-5 * np.abs(dg).max()
    assert (ws["p"] != 0).any() and (ws["df"] != 0).any()


def test_shared_weights_are_summed_over_the_rounds(dev, ops):
    """a dW of theta / phi / g is the sum of the restatement's per-round terms (within the bound of the one product over the
    stacked rows; the twin's 1e-4 as the sharp figure), and differs from what one round alone gives"""
    cfg, n = "pecnet_gen", 17
    m, sd = net(dev, cfg), sd_of(cfg)
    past, dest, pos, g_out = data(cfg, n)
    args = (T(past, dev), T(dest, dev), None, T(pos, dev))
    out, saved = ops.pecnet_train_fwd(m, *args)
    g = ops.pecnet_train_bwd(m, *args, saved, T(g_out, dev))
    b = PT.backward(sd, TN.masks_of(hidden_of(blocks(saved, sd, n, 2), sd, 2)), past, dest, pos, None, 2, g_out)
    one = net(dev, "gen_pools1")
    out1, saved1 = ops.pecnet_train_fwd(one, *args)
    g1 = ops.pecnet_train_bwd(one, *args, saved1, T(g_out, dev))
    RATIO.clear()
    for name, terms in b["round_terms"].items():
        assert len(terms) == 2
        total = terms[0] + terms[1]
        within(kind_of(name), N_(g[name]), total, b["grads_err"][name] + 1e-12 * np.abs(total).max(), name)
        if name.endswith("weight"):
            scale = np.abs(total).max()
            assert np.abs(N_(g[name]) - total).max() <= 1e-4 * scale, name
            for other in (*terms, N_(g1[name])):  # neither round alone, nor the one-round network: outside the 1e-4
                assert np.abs(N_(g[name]) - other).max() > 1e-3 * scale, name
    print("RATIO shared weights: error / bound " + ratios())


def wrapper(dev, cfg, twin=False, **hp_kw):
    """EigenTrajectory(PECNet, pecnet hooks) whose model_forward also records the bridge's inputs and the gradient that
    arrives at predict's output -> (model, record)"""
    import eigentrajectory_amd as ET
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    base = fresh(dev, cfg)
    if twin:
        base.__class__ = twin_of(base)
    hooks, rec = get_hook_func("pecnet"), {}
    call = hooks.model_forward

    def forward(net_in, baseline_model):
        out = call(net_in, baseline_model)
        rec["past"], rec["dest"], rec["mask"], rec["pos"] = net_in
        if out.requires_grad:
            out.register_hook(lambda g: rec.__setitem__("g_out", g.clone()))
        return out
    hooks.model_forward = forward
    model = ET.EigenTrajectory(base, hooks, default_hyper_params(static_dist=0.3, **hp_kw)).to(dev)
    if not twin:
        assert ET.enable_native_training(model) is model
    return model, rec


def test_autograd_contract_under_the_wrapper(dev, ops):
    cfg = "pecnet"
    model, rec = wrapper(dev, cfg)
    obs, pred = (T(a, dev) for a in synth(600, seed=3))
    model.calculate_parameters(obs, pred)
    m = model.baseline_model
    names = m.chain_parameter_names()
    so, sp = (T(a, dev) for a in synth(9, seed=4))
    addl = {"num_samples": 20, "scene_mask": torch.ones((9, 9), dtype=torch.bool, device=dev)}
    model.train()
    out = model(so, sp, addl_info=addl)
    loss = out["loss_eigentraj"] + out["loss_euclidean_ade"] + out["loss_euclidean_fde"]
    assert bool(torch.isfinite(loss))
    loss.backward(retain_graph=True)
    past, dest, mask, pos, g_out = rec["past"], rec["dest"], rec["mask"], rec["pos"], rec["g_out"]
    assert not past.is_contiguous() and past.shape == (9, 6) and g_out.shape == (9, 120)  # the bridge's views
    assert dest.data_ptr() == pos.data_ptr() and dest.stride() == pos.stride()  # one tensor handed over twice
    grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    assert sorted(grads) == sorted(names)  # the six chains; none of encoder_latent / decoder: predict does not touch them
    assert not any(k.startswith(("encoder_latent", "decoder")) for k in grads) and len(names) < len(list(m.parameters()))
    _, saved = ops.pecnet_train_fwd(m, past, dest, mask, pos)
    direct = ops.pecnet_train_bwd(m, past, dest, mask, pos, saved, g_out, need_input_grads=True)
    assert all(torch.equal(grads[k], direct[k]) for k in names)
    loss.backward()  # no zero_grad in between: autograd accumulates
    assert all(torch.equal(m.get_parameter(k).grad, 2 * grads[k]) for k in names)
    # one tensor as generated_dest AND initial_pos: autograd sums the two gradients itself
    x = dest.detach().clone().requires_grad_(True)
    p2 = past.detach().clone().requires_grad_(True)
    out2 = m.predict(p2, x, mask, x)
    assert out2.requires_grad and torch.equal(out2.detach(), m.eval().predict(past, dest, mask, pos))
    m.train()
    out2.backward(g_out)
    assert torch.equal(x.grad, direct["dest"] + direct["pos"]) and torch.equal(p2.grad, direct["past"])
    # the ET widths: the running bound is far wider than the values, so this configuration is held against torch's own backward
    near_twin(direct, *twin_grads(dev, cfg, past, dest, mask, pos, g_out))
    # an optimiser step between forward and backward is caught: the kernels read the weights in place
    out3 = m.predict(past, dest, mask, pos)
    with torch.no_grad():
        m.non_local_g.layers[0].bias.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out3.backward(g_out)
    with torch.no_grad():
        assert m.predict(past, dest, mask, pos).requires_grad is False
    model.eval()
    assert m.predict(past, dest, mask, pos).requires_grad is False  # eval mode: the inference path, whatever the flag
    # accumulation over two scenes
    model.train()
    m.zero_grad()
    for seed, cnt in ((5, 4), (6, 7)):
        a, b_ = (T(v, dev) for v in synth(cnt, seed=seed))
        o = model(a, b_, addl_info={"num_samples": 20, "scene_mask": torch.ones((cnt, cnt), dtype=torch.bool, device=dev)})
        (o["loss_eigentraj"] + o["loss_euclidean_ade"]).backward()
        if cnt == 4:
            first = {k: m.get_parameter(k).grad.clone() for k in names}
    assert all(bool(torch.isfinite(m.get_parameter(k).grad).all()) for k in names)
    assert any(not torch.equal(m.get_parameter(k).grad, first[k]) for k in names)


def scenes_data(sizes, seed):
    from eigentrajectory_amd.data import TrajectoryData
    obs, pred = synth(sum(sizes), seed=seed)
    ends = np.cumsum(sizes)
    return TrajectoryData.from_arrays(obs, pred, [(int(e - s), int(e)) for e, s in zip(ends, sizes)])


def trainer(dev, twin, like=None):
    """a collated ETTrainer on six synthetic scenes around pecnet_gen (k = 4, S = 3)"""
    from eigentrajectory_amd.trainer import ETTrainer
    model, rec = wrapper(dev, "pecnet_gen", twin, k=4, num_samples=3, batch_size=16, lr=1e-3, weight_decay=1e-4, clip_grad=10,
                         lr_schd=False)
    train = scenes_data([3, 20, 7, 12, 5, 9], seed=11)
    tr = ETTrainer(model, model.hyper_params, train, scenes_data([4, 6], seed=12), scenes_data([5, 3], seed=13),
                   mode="collated", device=dev)
    if like is None:
        tr.init_descriptor()
    else:
        model.load_state_dict(like.model.state_dict(), strict=True)
    return tr, rec


def test_one_trainer_step_and_a_two_epoch_fit(dev, ops):
    tr, rec = trainer(dev, twin=False)
    tw, _ = trainer(dev, twin=True, like=tr)
    m, names = tr.predictor, tr.predictor.chain_parameter_names()
    batch = [1, 3]  # two scenes, 32 pedestrians: two tiles, a block mask
    tr.model.train()
    tw.model.train()
    loss = tr._train_batch(tr.train_data, batch)
    loss_tw = tw._train_batch(tw.train_data, batch)
    assert np.isfinite(loss) and abs(loss - loss_tw) <= 1e-4 * abs(loss_tw)
    assert rec["past"].shape == (32, 4) and rec["mask"].dtype == torch.bool and not bool(rec["mask"][0, 31])
    near_twin({k: m.get_parameter(k).grad for k in names}, {k: tw.predictor.get_parameter(k).grad for k in names},
              phi_terms_of(tw.predictor))
    assert all(p.grad is None for k, p in m.named_parameters() if k not in names)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    for t in (tr, tw):
        if t.hp.clip_grad is not None:
            torch.nn.utils.clip_grad_norm_(t.predictor.parameters(), t.hp.clip_grad)
        t.optimizer.step()
    for k in before:  # the updated weights agree with the twin's; the six chains moved, nothing else did
        a, b_ = m.state_dict()[k], tw.predictor.state_dict()[k]
        assert float((a - b_).abs().max()) <= 1e-4 * max(float(b_.abs().max()), 1e-30), k
        assert torch.equal(before[k], a) == (k not in names), k
    tr.fit(2)
    assert len(tr.log["train_loss"]) == 2 and np.isfinite(tr.log["train_loss"]).all()
    assert tr.log["train_loss"][1] < tr.log["train_loss"][0]
    assert np.isfinite(tr.log["val_loss"]).all() and not m.training
    res = tr.test()
    assert np.isfinite(res["ADE"]) and np.isfinite(res["FDE"])
