"""CPU checks of native ET-PECNet training (eigentrajectory_amd/pecnet.py, csrc/et_mlp_train.hip): the float64 restatement
(tests/_pecnet_train_np.py) against torch's CPU autograd of the reference's formula, its error bound against a numpy float32
evaluation, the opt-in function's contract, and the four C entry points' declarations and argument checks (none of which
launches anything)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from . import _abi_header as H
from . import _golden as G
from . import _mlp_train_np as TN
from . import _pecnet_np as PN
from . import _pecnet_train_np as PT

Z = G.load("g24_pecnet.npz")
CFG = "pecnet_gen"  # encoders 4 / 2 -> 24 -> 12 -> 5, theta / phi 12 -> 24 -> 12 -> 7, g 12 -> 24 -> 12 -> 12, predictor -> 12
POOLS = 2
MASKS = ("ones", "blocks", "zero_row", "fractional")


def weights():
    return PN.weights(Z, CFG)


def inputs(n, seed=0):
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal((n, w)).astype(np.float32) for w in (4, 2, 2, 12))  # past, dest, pos, g_out


def mask_of(kind, n):
    """all ones | two scenes' blocks | ones with row n // 2 all zero | fractions in [0.25, 1] with one entry of -0.5"""
    if kind == "ones":
        return np.ones((n, n), np.float32)
    if kind == "blocks":
        m = np.zeros((n, n), np.float32)
        cut = (n + 1) // 2
        m[:cut, :cut] = 1
        m[cut:, cut:] = 1
        return m
    if kind == "zero_row":
        m = np.ones((n, n), np.float32)
        m[n // 2] = 0
        return m
    m = (0.25 + 0.75 * np.random.default_rng(5).random((n, n))).astype(np.float32)
    m[n // 2, n // 3] = -0.5
    return m


def torch_chain(sd, chain, x, keep=None):
    n = TN.n_layers(sd, chain)
    for i in range(n):
        x = F.linear(x, sd[f"{chain}.layers.{i}.weight"], sd[f"{chain}.layers.{i}.bias"])
        if i + 1 < n:
            x = torch.relu(x)
            if keep is not None:
                keep.append(x)
    return x


def torch_reference(sd_np, past, dest, pos, mask, pools, g_out):
    """float64 torch autograd of baseline/pecnet/model.py's predict -> out, the features entering every round and the
    predictor, theta of every round with its gradient, gradients by name (+ past, dest, pos)"""
    sd = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in sd_np.items()
          if k.split(".")[0] in PT.CHAINS}
    past, dest, pos = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (past, dest, pos))
    mask = torch.tensor(mask, dtype=torch.float64)
    feat = torch.cat([torch_chain(sd, "encoder_past", past), torch_chain(sd, "encoder_dest", dest), pos], dim=1)
    feats, thetas = [feat], []
    for _ in range(pools):
        theta = torch_chain(sd, "non_local_theta", feat)
        theta.retain_grad()
        thetas.append(theta)
        f = torch.matmul(theta, torch_chain(sd, "non_local_phi", feat).transpose(1, 0))
        w = F.softmax(f, dim=-1) * mask
        w = F.normalize(w, p=1, dim=1)
        feat = torch.matmul(w, torch_chain(sd, "non_local_g", feat)) + feat
        feats.append(feat)
    out = torch_chain(sd, "predictor", feat)
    out.backward(torch.tensor(g_out, dtype=torch.float64))
    grads = {k: v.grad.numpy() for k, v in sd.items() if v.grad is not None}
    grads.update(past=past.grad.numpy(), dest=dest.grad.numpy(), pos=pos.grad.numpy())
    return (out.detach().numpy(), [a.detach().numpy() for a in feats], [t.grad.numpy() for t in thetas], grads)


def rel(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def relu_masks(sd, f, pools):
    """the restatement's own ReLU masks in the layout its backward takes"""
    m = {c: [a > 0 for a in f["acts"][c][1:]] for c in ("encoder_past", "encoder_dest", "predictor")}
    for c in PT.POOLED if pools else ():
        m[c] = [np.concatenate([f["acts"][c][r][i] for r in range(pools)]) > 0 for i in range(1, TN.n_layers(sd, c))]
    return m


def close(b, name, got, ref, tol=1e-12):
    """``tol`` of the tensor's OWN largest entry.  One exception, the last bias gradient of non_local_phi: it is sum_j d phi_j
    = sum_i (sum_j d f_ij) theta_i, and sum_j d f_ij = sum_j s_ij ds_ij - (sum_k ds_ik s_ik)(sum_j s_ij) = 0 because a softmax
    row sums to 1 -- whatever the mask, the tensor is exactly 0 in exact arithmetic and holds rounding only (about 1e-18
    here), so it is held to ``tol`` of the largest of the terms it sums, g_z at phi's output"""
    scale = np.abs(ref).max()
    if name == f"non_local_phi.layers.{TN.n_layers(weights(), 'non_local_phi') - 1}.bias":
        scale = np.abs(b["gz"]["non_local_phi"][-1]).max()
    return np.abs(got - ref).max() <= tol * max(scale, 1e-300)


def restatement(sd, past, dest, pos, mask, pools, g_out):
    f = PT.forward(sd, past, dest, pos, mask, pools)
    return f, PT.backward(sd, relu_masks(sd, f, pools), past, dest, pos, mask, pools, g_out)


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("n", [1, 5, 17])
def test_restatement_equals_torch_autograd_in_float64(n, kind):
    sd = weights()
    past, dest, pos, g_out = inputs(n, seed=n)
    mask = mask_of(kind, n)
    out, feats, dthetas, grads = torch_reference(sd, past, dest, pos, mask, POOLS, g_out)
    f, b = restatement(sd, past, dest, pos, mask, POOLS, g_out)
    assert rel(f["out"], out) <= 1e-12
    assert len(f["feat"]) == POOLS + 1
    for a, ref in zip(f["feat"], feats):
        assert rel(a, ref) <= 1e-12
    assert set(b["grads"]) == set(grads) and len(grads) == 6 * 6 + 3
    for name, ref in grads.items():
        assert b["grads"][name].shape == ref.shape, name
        assert np.isfinite(b["grads"][name]).all() and np.isfinite(ref).all(), name
        assert close(b, name, b["grads"][name], ref), name
        assert (b["grads_err"][name] >= 0).all() and np.isfinite(b["grads_err"][name]).all(), name
    for r in range(POOLS):
        assert rel(b["pool"][r]["dtheta"], dthetas[r]) <= 1e-12
        # the shared weights: the one product over the stacked rounds is the sum of the rounds' own
        for name, terms in b["round_terms"].items():
            assert close(b, name, sum(terms), b["grads"][name]), name
    if kind == "zero_row":  # p = 0 there: nothing reaches that row's theta, in torch and in the restatement, and nothing is NaN
        row = n // 2
        for r in range(POOLS):
            assert (f["rounds"][r]["p"][row] == 0).all() and f["rounds"][r]["clamped"][row]
            assert (b["pool"][r]["dtheta"][row] == 0).all() and (dthetas[r][row] == 0).all()
            assert (b["pool"][r]["df"][row] == 0).all() and (b["pool"][r]["edf"][row] <= PT.TINY).all()
            assert np.array_equal(f["feat"][r + 1][row], f["feat"][r][row])  # the row's features pass unchanged
    if kind == "fractional" and n > 1:  # the sign(w) term is in play
        assert (f["rounds"][0]["w"] < 0).sum() == 1


def eval32(sd, past, dest, pos, mask, pools, g_out):
    """the same network in numpy float32 (its matmuls sum in their own order) -> out, hidden activations, features,
    gradients, and per round the pooling step's inputs and results (``stages``)"""
    f32 = np.float32

    def chain(c, x):
        acts, n = [x], TN.n_layers(sd, c)
        for i in range(n):
            x = (x @ sd[f"{c}.layers.{i}.weight"].T + sd[f"{c}.layers.{i}.bias"]).astype(f32)
            if i + 1 < n:
                x = np.maximum(x, f32(0))
                acts.append(x)
        return x, acts

    def chain_back(c, acts, g, grads):
        for i in range(TN.n_layers(sd, c) - 1, -1, -1):
            w, b = f"{c}.layers.{i}.weight", f"{c}.layers.{i}.bias"
            grads[w] = grads.get(w, 0) + (g.T @ acts[i]).astype(f32)
            grads[b] = grads.get(b, 0) + g.sum(axis=0, dtype=f32)
            g = (g @ sd[w]).astype(f32)
            if i > 0:
                g = np.where(acts[i] > 0, g, f32(0))
        return g
    mask = mask.astype(f32)
    fp, ap = chain("encoder_past", past)
    fd, ad = chain("encoder_dest", dest)
    feat = np.concatenate([fp, fd, pos], axis=1)
    feats, rounds = [feat], []
    for _ in range(pools):
        (th, ath), (ph, aph), (g, ag) = (chain(c, feat) for c in PT.POOLED)
        f = (th @ ph.T).astype(f32)
        e = np.exp(f - f.max(axis=1, keepdims=True), dtype=f32)
        s = e / e.sum(axis=1, keepdims=True, dtype=f32)
        w = s * mask
        l1 = np.abs(w).sum(axis=1, keepdims=True, dtype=f32)
        den = np.maximum(l1, f32(1e-12))
        p = w / den
        rounds.append((th, ath, ph, aph, g, ag, s, w, l1, den, p))
        feat = ((p @ g).astype(f32) + feat).astype(f32)
        feats.append(feat)
    out, apr = chain("predictor", feat)
    grads, stages = {}, []
    G_ = chain_back("predictor", apr, g_out, grads)
    for r in range(pools - 1, -1, -1):
        th, ath, ph, aph, g, ag, s, w, l1, den, p = rounds[r]
        dp = (G_ @ g.T).astype(f32)
        r1 = (dp * p).sum(axis=1, keepdims=True, dtype=f32)
        dw = np.where(l1 > f32(1e-12), (dp - np.sign(w) * r1) / den, dp / f32(1e-12)).astype(f32)
        ds = np.where(mask == 0, f32(0), dw * mask)
        df = s * (ds - (ds * s).sum(axis=1, keepdims=True, dtype=f32))
        dth, dph, dg = (df @ ph).astype(f32), (df.T @ th).astype(f32), (p.T @ G_).astype(f32)
        stages.insert(0, dict(theta=th, phi=ph, g=g, feat=feats[r], out=feats[r + 1], G=G_, p=p, df=df, dtheta=dth, dphi=dph,
                              dg=dg))
        parts = [chain_back("non_local_theta", ath, dth, grads), chain_back("non_local_phi", aph, dph, grads),
                 chain_back("non_local_g", ag, dg, grads)]
        G_ = ((G_ + parts[0]) + parts[1]) + parts[2]
    grads["past"] = chain_back("encoder_past", ap, np.ascontiguousarray(G_[:, :5]), grads)
    grads["dest"] = chain_back("encoder_dest", ad, np.ascontiguousarray(G_[:, 5:10]), grads)
    grads["pos"] = G_[:, 10:]
    hidden = {"encoder_past": ap[1:], "encoder_dest": ad[1:], "predictor": apr[1:]}
    for k, c in zip((1, 3, 5), PT.POOLED):
        hidden[c] = [np.concatenate([r[k][i] for r in rounds]) for i in range(1, len(rounds[0][k]))] if rounds else []
    return out, hidden, feats, grads, stages


@pytest.mark.parametrize("kind", MASKS)
def test_the_bound_holds_for_an_fp32_evaluation_and_is_not_vacuous(kind):
    """numpy's float32 matmul and sums run in their own order, its exp is not the device's: the bound holds for any order
    and allows 3 ulp for exp.  (The gradient of a weight shared by the rounds is accumulated per round here: one more
    addition than the kernel's single chain, inside gamma(pools N + 1).)

    Not vacuous: the LBEBM test's form, 1e-3 of each tensor's scale, is reached by everything before the first softmax (the
    features entering round 0: 2.6e-6).  Behind it the running bound cannot reach it with these weights -- measured here at
    N = 17 over the four masks: bound / scale 6.7e-3 after one round, 3.6 after two, 1e17 and more for the gradients of theta
    and phi -- while the float32 evaluation itself is within 6.4e-8 of the scale for every feature block and the output and
    1.8e-5 for every gradient.  So two further assertions stand in: the float32 evaluation is within 1e-6 (values; margin 16
    on the measured figure) and 1e-4 (gradients; margin 5, the project's cross-check figure) of each tensor's scale; and every
    pooling step, forward and backward, restated from ITS OWN float32 inputs (``pool_stage``) is within that step's bound.
    That bound, as a share of each tensor's scale, measured here: out 1.1e-5, p 1e-4, d g 2.8e-4, d f 1.8e-3, d phi 1.3e-2,
    d theta 3.2e-2 (d f sums to exactly nothing along a row, so d theta and d phi are cancelling sums: their bound is that
    of their terms).  out, p and d g are asserted below the LBEBM form's 1e-3; d f, d phi and d theta below 0.1: a wrong
    sign, mask, transposition or missing term moves a tensor by the order of its scale, a decade and more above."""
    sd = weights()
    n = 17
    past, dest, pos, g_out = inputs(n, seed=3)
    mask = mask_of(kind, n)
    out, hidden, feats, grads, stages = eval32(sd, past, dest, pos, mask, POOLS, g_out)
    f = PT.forward(sd, past, dest, pos, mask, POOLS)
    worst = {}

    def held(kind_, got, ref, err, what):
        d = np.abs(got.astype(np.float64) - ref)
        assert (d <= err).all(), what
        worst[kind_] = max(worst.get(kind_, 0.0), float((d[err > 0] / err[err > 0]).max()) if (err > 0).any() else 0.0)
        return d.max() / np.abs(ref).max(), err.max() / np.abs(ref).max()
    assert held("running", out, f["out"], f["out_err"], "out")[0] <= 1e-6
    for i, (a, ref, err) in enumerate(zip(feats, f["feat"], f["feat_err"])):
        d, e = held("running", a, ref, err, "feat")
        assert d <= 1e-6 and (e <= 1e-3 or i > 0)
    b = PT.backward(sd, TN.masks_of(hidden), past, dest, pos, mask, POOLS, g_out)
    for name, err in b["grads_err"].items():
        held("running", grads[name], b["grads"][name], err, name)
        assert close(b, name, grads[name], b["grads"][name], 1e-4), name
    tight = {}
    for r, st in enumerate(stages):
        rd, pb = PT.pool_stage(st["theta"], st["phi"], st["g"], st["feat"], mask, st["G"])
        assert not rd["unsure"].any()
        for key, ref, err in (("out", rd["out"], rd["eout"]), ("p", rd["p"], rd["ep"]), ("df", pb["df"], pb["edf"]),
                              ("dtheta", pb["dtheta"], pb["edtheta"]), ("dphi", pb["dphi"], pb["edphi"]),
                              ("dg", pb["dg"], pb["edg"])):
            tight[key] = max(tight.get(key, 0.0), held("stage", st[key], ref, err, (r, key))[1])
    print(f"{kind}: float32 error / bound: running {worst['running']:.3f}, stage {worst['stage']:.3f}; stage bound / scale "
          + ", ".join(f"{k} {v:.1e}" for k, v in tight.items()))
    assert max(tight[k] for k in ("out", "p", "dg")) <= 1e-3 and max(tight.values()) <= 0.1


def test_enable_native_training_contract():
    import eigentrajectory_amd as ET
    from eigentrajectory_amd._lib import ETLibraryError
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    m = PN.native_module(CFG)
    past, dest, mask = torch.zeros(3, 4), torch.zeros(3, 2), torch.ones(3, 3)
    assert m.native_training is False and m.training and not hasattr(m, "enable_native_training")
    with pytest.raises(RuntimeError, match="eval"):
        m.predict(past, dest, mask, dest)
    keys = list(m.state_dict())
    assert ET.enable_native_training(m) is m and m.native_training is True
    assert list(m.state_dict()) == keys and not any("native" in k for k in keys)
    assert "native_training" not in dict(m.named_parameters()) and "native_training" not in dict(m.named_buffers())
    with pytest.raises(ETLibraryError, match="no CPU path"):  # training mode now reaches the native path
        m.predict(past, dest, mask, dest)
    m.eval()
    with pytest.raises(ETLibraryError, match="no CPU path"):  # eval mode: the inference path, whatever the flag
        m.predict(past, dest, mask, dest)
    with pytest.raises(NotImplementedError, match="only predict"):
        m(past, dest)
    assert ET.enable_native_training(m.train(), False) is m and m.native_training is False
    with pytest.raises(RuntimeError, match="eval"):
        m.predict(past, dest, mask, dest)
    ET.enable_native_training(m)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in weights().items()}, strict=True)  # the reference's keys
    assert m.native_training is True and PN.native_module(CFG).native_training is False  # per instance
    assert m.chain_parameter_names() == [k for c in PT.CHAINS for k in keys if k.split(".")[0] == c]
    assert all(p is m.get_parameter(k) for p, k in zip(m.chain_parameters(), m.chain_parameter_names()))
    assert not any(k.startswith(("encoder_latent", "decoder")) for k in m.chain_parameter_names())
    # through the wrapper, and for the other predictors
    wrapped = ET.EigenTrajectory(PN.native_module(CFG), get_hook_func("pecnet"), default_hyper_params(k=4, num_samples=3))
    assert ET.enable_native_training(wrapped) is wrapped and wrapped.baseline_model.native_training is True
    lb = PN.native_module("lbebm_gen")
    assert ET.enable_native_training(lb) is lb and lb.native_training is True
    assert ET.enable_native_training(lb, False) is lb and lb.native_training is False
    with pytest.raises(NotImplementedError, match="SGCN has no native backward pass"):
        ET.enable_native_training(ET.SGCN())
    with pytest.raises(NotImplementedError, match="no native backward pass"):
        ET.enable_native_training(torch.nn.Linear(2, 2))


def _params(**kw):
    """et_mlp_params of the ET PECNet whose every pointer is a (never dereferenced) non-NULL host address"""
    from eigentrajectory_amd import _lib
    p = _lib.MLPParams()
    p.fdim, p.nonlocal_pools, p.non_local_dim, p.out_width, p.pos_width = 16, 3, 128, 120, 2
    nl = [34, 256, 128, 64]
    chains = dict(encoder_past=[6, 512, 256, 16], encoder_dest=[2, 8, 16, 16], non_local_theta=nl + [128],
                  non_local_phi=nl + [128], non_local_g=nl + [34], predictor=[34, 1024, 512, 256, 120])
    chains.update({k: v for k, v in kw.items() if k in chains})
    for name, widths in chains.items():
        c = getattr(p, name)
        c.n_layers = len(widths) - 1
        for i, w in enumerate(widths[:_lib.MLP_MAX_LAYERS + 1]):
            c.widths[i] = w
        for i in range(min(c.n_layers, _lib.MLP_MAX_LAYERS)):
            c.w[i] = c.b[i] = 8
    for k, v in kw.items():
        if k not in chains:
            setattr(p, k, v)
    return p


def test_training_entry_points_are_declared_bound_and_check_their_arguments():
    from eigentrajectory_amd import _lib
    lib = _lib.lib()
    protos = H.functions()
    for name in ("et_pecnet_train_saved_bytes", "et_pecnet_train_workspace_bytes", "et_pecnet_train_fwd",
                 "et_pecnet_train_bwd"):
        assert name in protos and name in _lib.SIGNATURES and hasattr(lib, name)
    assert H.struct_fields("et_pecnet_grads") == [f[0] for f in _lib.PECNetGrads._fields_]
    assert C.sizeof(_lib.PECNetGrads) == 6 * C.sizeof(_lib.MLPChainGrads)
    INVALID, UNSUPPORTED, WORKSPACE = 1, 3, 4

    def grads(p, fill=8):
        g = _lib.PECNetGrads()
        for chain in PT.CHAINS:
            for i in range(min(getattr(p, chain).n_layers, _lib.MLP_MAX_LAYERS)):
                getattr(g, chain).dw[i] = getattr(g, chain).db[i] = fill
        return g

    def fwd(p, n=3, past=8, pos=8, saved=8):
        return lib.et_pecnet_train_fwd(C.byref(p), past, 1, n, 8, 1, n, pos, 1, n, None, n, 8, saved, None, 0, None)

    def bwd(p, n=3, g=None, ws=None, nbytes=0, rs=1):
        g = grads(p) if g is None else g
        return lib.et_pecnet_train_bwd(C.byref(p), 8, rs, n, 8, 1, n, 8, 1, n, None, n, 8, 8, C.byref(g), None, None, None, ws,
                                       nbytes, None)

    for call in (fwd, bwd):
        assert call(_params(predictor=[34, 2048, 120])) == UNSUPPORTED            # a width of 2048
        assert call(_params(non_local_g=[34, 8, 8, 8, 8, 8, 34])) == UNSUPPORTED  # five hidden layers
        assert call(_params(non_local_phi=[34, 64, 127])) == UNSUPPORTED          # not non_local_dim wide
        assert call(_params(pos_width=0)) == UNSUPPORTED                          # an LBEBM parameter block
        assert call(_params(nonlocal_pools=9)) == UNSUPPORTED
        assert call(_params(), n=4097) == UNSUPPORTED                             # beyond the pooling's range
        p = _params()
        p.non_local_theta.w[0] = None
        assert call(p) == INVALID
        assert call(_params(), n=-1) == INVALID
    assert fwd(_params(), n=0) == 0                # nothing to do
    assert fwd(_params(), past=None) == INVALID and fwd(_params(), pos=None) == INVALID
    assert fwd(_params(), saved=None) == INVALID
    assert lib.et_pecnet_train_fwd(None, 8, 1, 3, 8, 1, 3, 8, 1, 3, None, 3, 8, 8, None, 0, None) == INVALID
    assert bwd(_params(), rs=-1) == INVALID
    p = _params()
    g = grads(p)
    g.non_local_g.db[3] = None
    assert bwd(p, g=g) == INVALID
    p0 = _params(nonlocal_pools=0)                 # without rounds theta / phi / g are neither checked nor written
    assert bwd(p0, g=g) == WORKSPACE
    assert bwd(_params()) == WORKSPACE             # refused before the launch
    saved = lambda p, n: int(lib.et_pecnet_train_saved_bytes(C.byref(p), n))
    ws = lambda p, n: int(lib.et_pecnet_train_workspace_bytes(C.byref(p), n))
    # N = 100: the encoders' outputs and the hidden layers of encoder_past, encoder_dest, predictor as for LBEBM ...
    base = 16 + 16 + 512 + 256 + 8 + 16 + 1024 + 512 + 256
    hidden = 3 * (256 + 128 + 64)                  # ... theta, phi and g each
    # saved: + 4 feature blocks of F = 34 (three rounds and the predictor), per round theta, phi (128), g (34), the hidden
    assert saved(_params(), 100) == 4 * 100 * (base + 4 * 34 + 3 * (128 + 128 + 34 + hidden))
    # workspace: + G and three input gradients (4 x 34), the same per-round blocks, p and df (2 x 100 per row)
    assert ws(_params(), 100) == 4 * 100 * (base + 4 * 34 + 3 * (128 + 128 + 34 + hidden) + 2 * 100)
    assert bwd(_params(), ws=8, nbytes=ws(_params(), 100) - 4, n=100) == WORKSPACE
    assert saved(p0, 100) == ws(p0, 100) == 4 * 100 * base
    for size in (saved, ws):
        assert size(_params(), 0) == 0 and size(_params(out_width=119), 100) == 0 and size(_params(pos_width=0), 100) == 0
    # N = 3: (3, 16) takes 48 floats, (3, 34) 104 (102 -> 104), (12, 34) 408, (9, 34) 308 (306 -> 308), (3, 3) 12 (9 -> 12)
    assert saved(_params(), 3) == 4 * (2 * 48 + 3 * (base - 32) + 408 + 9 * (128 + 128 + hidden) + 308)
    assert ws(_params(), 3) == 4 * (2 * 48 + 3 * (base - 32) + 4 * 104 + 9 * (128 + 128 + hidden) + 308 + 2 * 12)
    # the LBEBM entries keep refusing this block
    assert int(lib.et_lbebm_train_workspace_bytes(C.byref(_params()), 100)) == 0
