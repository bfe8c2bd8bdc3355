"""CPU checks of native ET-LBEBM training (eigentrajectory_amd/lbebm.py, csrc/et_mlp_train.hip): the float64 restatement
(tests/_mlp_train_np.py) against torch's CPU autograd, its error bound against an fp32 evaluation, the opt-in flag's
contract, and the three C entry points' declarations and argument checks (none of which launches anything)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from . import _abi_header as H
from . import _golden as G
from . import _mlp_train_np as TN
from . import _pecnet_np as PN

Z = G.load("g24_pecnet.npz")
CFG = "lbebm_gen"  # encoder_past 4 -> 24 -> 12 -> 5, encoder_dest 2 -> 24 -> 12 -> 5, predictor 10 -> 24 -> 12 -> 12
ZERO_UNITS = (("encoder_past", 0, 3), ("predictor", 1, 2))  # (chain, layer, unit): weight row and bias set to zero


def weights(zero_units=False):
    sd = {k: v.copy() for k, v in PN.weights(Z, CFG).items()}
    if zero_units:
        for chain, layer, unit in ZERO_UNITS:
            sd[f"{chain}.layers.{layer}.weight"][unit] = 0.0
            sd[f"{chain}.layers.{layer}.bias"][unit] = 0.0
    return sd


def inputs(n, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 4)).astype(np.float32), rng.standard_normal((n, 2)).astype(np.float32),
            rng.standard_normal((n, 12)).astype(np.float32))


def torch_chain(sd, chain, x, keep):
    n = TN.n_layers(sd, chain)
    for i in range(n):
        x = F.linear(x, sd[f"{chain}.layers.{i}.weight"], sd[f"{chain}.layers.{i}.bias"])
        if i + 1 < n:
            x = torch.relu(x)
            keep.append(x)
    return x


def torch_reference(sd_np, past, dest, g_out):
    """float64 torch autograd -> out, hidden activations per chain, gradients by name (+ past, dest)"""
    sd = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in sd_np.items()
          if k.split(".")[0] in TN.CHAINS}
    past = torch.tensor(past, dtype=torch.float64, requires_grad=True)
    dest = torch.tensor(dest, dtype=torch.float64, requires_grad=True)
    acts = {c: [] for c in TN.CHAINS}
    feat = torch.cat([torch_chain(sd, "encoder_past", past, acts["encoder_past"]),
                      torch_chain(sd, "encoder_dest", dest, acts["encoder_dest"])], dim=1)
    out = torch_chain(sd, "predictor", feat, acts["predictor"])
    out.backward(torch.tensor(g_out, dtype=torch.float64))
    grads = {k: v.grad.numpy() for k, v in sd.items()}
    grads.update(past=past.grad.numpy(), dest=dest.grad.numpy())
    return out.detach().numpy(), {c: [a.detach().numpy() for a in acts[c]] for c in acts}, grads


def rel(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


@pytest.mark.parametrize("zero_units", [False, True])
@pytest.mark.parametrize("n", [1, 5, 17])
def test_restatement_equals_torch_autograd_in_float64(n, zero_units):
    sd = weights(zero_units)
    past, dest, g_out = inputs(n, seed=n)
    out, acts, grads = torch_reference(sd, past, dest, g_out)
    f = TN.forward(sd, past, dest)
    assert rel(f["out"], out) <= 1e-12
    for c in TN.CHAINS:
        assert len(f["acts"][c]) == len(acts[c]) + 1
        for a, b in zip(f["acts"][c][1:], acts[c]):
            assert rel(a, b) <= 1e-12
    b = TN.backward(sd, TN.masks_of({c: f["acts"][c][1:] for c in TN.CHAINS}), past, dest, g_out)
    assert set(b["grads"]) == set(grads) and len(grads) == 20
    for name, ref in grads.items():
        assert b["grads"][name].shape == ref.shape, name
        assert rel(b["grads"][name], ref) <= 1e-12, name
        assert (b["grads_err"][name] >= 0).all() and np.isfinite(b["grads_err"][name]).all()
    if zero_units:  # z is exactly 0 there: relu'(0) = 0, nothing passes, in torch and in the restatement
        for chain, layer, unit in ZERO_UNITS:
            assert (f["z"][chain][layer][:, unit] == 0).all() and (f["acts"][chain][layer + 1][:, unit] == 0).all()
            for g in (grads, b["grads"]):
                assert (g[f"{chain}.layers.{layer}.weight"][unit] == 0).all() and g[f"{chain}.layers.{layer}.bias"][unit] == 0
            assert (b["gz"][chain][layer][:, unit] == 0).all() and (b["gz_err"][chain][layer][:, unit] == 0).all()


def test_the_bound_holds_for_an_fp32_evaluation_and_is_not_vacuous():
    """numpy's float32 matmul sums in its own order; the bound holds for any order.  It stays three orders of magnitude
    below the tensor's scale: a wrong layer, mask or transposition (an error of the order of the scale) is far outside."""
    sd = weights()
    past, dest, g_out = inputs(17, seed=3)
    f = TN.forward(sd, past, dest)

    def chain32(chain, x):
        acts = []
        n = TN.n_layers(sd, chain)
        for i in range(n):
            x = (x @ sd[f"{chain}.layers.{i}.weight"].T + sd[f"{chain}.layers.{i}.bias"]).astype(np.float32)
            if i + 1 < n:
                x = np.maximum(x, np.float32(0))
                acts.append(x)
        return x, acts

    fp, ap = chain32("encoder_past", past)
    fd, ad = chain32("encoder_dest", dest)
    out, apr = chain32("predictor", np.concatenate([fp, fd], axis=1))
    assert (np.abs(out - f["out"]) <= f["out_err"]).all()
    for chain, acts in (("encoder_past", ap), ("encoder_dest", ad), ("predictor", apr)):
        for a, ref, err in zip(acts, f["acts"][chain][1:], f["acts_err"][chain][1:]):
            assert (np.abs(a - ref) <= err).all()
    assert f["out_err"].max() <= 1e-3 * np.abs(f["out"]).max()
    b = TN.backward(sd, TN.masks_of({"encoder_past": ap, "encoder_dest": ad, "predictor": apr}), past, dest, g_out)
    for name, err in b["grads_err"].items():
        assert err.max() <= 1e-3 * np.abs(b["grads"][name]).max(), name


def test_native_training_flag_contract():
    from eigentrajectory_amd._lib import ETLibraryError
    m = PN.native_module(CFG)
    past, dest = torch.zeros(3, 4), torch.zeros(3, 2)
    assert m.native_training is False and m.training
    with pytest.raises(RuntimeError, match="eval"):
        m.predict(past, dest)
    keys = list(m.state_dict())
    assert m.enable_native_training() is m and m.native_training is True
    assert list(m.state_dict()) == keys and not any("native" in k for k in keys)
    assert "native_training" not in dict(m.named_parameters()) and "native_training" not in dict(m.named_buffers())
    with pytest.raises(ETLibraryError, match="no CPU path"):
        m.predict(past, dest)
    m.eval()
    with pytest.raises(ETLibraryError, match="no CPU path"):  # eval mode: the inference path, whatever the flag
        m.predict(past, dest)
    with pytest.raises(NotImplementedError, match="only predict"):
        m(past, dest)
    m.train().enable_native_training(False)
    assert m.native_training is False
    with pytest.raises(RuntimeError, match="eval"):
        m.predict(past, dest)
    m.enable_native_training()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in PN.weights(Z, CFG).items()}, strict=True)  # reference keys
    assert m.native_training is True
    assert m.chain_parameter_names() == [k for k in keys if k.split(".")[0] in TN.CHAINS]
    assert all(p is m.get_parameter(k) for p, k in zip(m.chain_parameters(), m.chain_parameter_names()))
    p = PN.native_module("pecnet_gen")
    assert not hasattr(p, "enable_native_training")
    with pytest.raises(RuntimeError, match="eval"):
        p.predict(torch.zeros(3, 4), dest, torch.ones(3, 3), dest)


def _params(**kw):
    """et_mlp_params of an LBEBM whose every pointer is a (never dereferenced) non-NULL host address"""
    from eigentrajectory_amd import _lib
    p = _lib.MLPParams()
    p.fdim, p.nonlocal_pools, p.non_local_dim, p.out_width, p.pos_width = 16, 0, 0, 120, 0
    chains = dict(encoder_past=[6, 512, 256, 16], encoder_dest=[2, 8, 16, 16], predictor=[32, 1024, 512, 256, 120])
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
    for name in ("et_lbebm_train_workspace_bytes", "et_lbebm_train_fwd", "et_lbebm_train_bwd"):
        assert name in protos and name in _lib.SIGNATURES and hasattr(lib, name)
    for struct, mirror in (("et_mlp_chain_grads", _lib.MLPChainGrads), ("et_lbebm_grads", _lib.LBEBMGrads)):
        assert H.struct_fields(struct) == [f[0] for f in mirror._fields_], struct
    assert C.sizeof(_lib.MLPChainGrads) == 2 * _lib.MLP_MAX_LAYERS * 8 and C.sizeof(_lib.LBEBMGrads) == 3 * C.sizeof(_lib.MLPChainGrads)
    INVALID, UNSUPPORTED, WORKSPACE = 1, 3, 4

    def grads(p, fill=8):
        g = _lib.LBEBMGrads()
        for chain in ("encoder_past", "encoder_dest", "predictor"):
            for i in range(min(getattr(p, chain).n_layers, _lib.MLP_MAX_LAYERS)):
                getattr(g, chain).dw[i] = getattr(g, chain).db[i] = fill
        return g

    def fwd(p, n=3, past=8, saved=8):
        return lib.et_lbebm_train_fwd(C.byref(p), past, 1, n, 8, 1, n, n, 8, saved, None, 0, None)

    def bwd(p, n=3, g=None, ws=None, nbytes=0, rs=1):
        g = grads(p) if g is None else g
        return lib.et_lbebm_train_bwd(C.byref(p), 8, rs, n, 8, 1, n, n, 8, 8, C.byref(g), None, None, ws, nbytes, None)

    for call in (fwd, bwd):
        assert call(_params(predictor=[32, 2048, 120])) == UNSUPPORTED            # a width of 2048
        assert call(_params(predictor=[32, 8, 8, 8, 8, 8, 120])) == UNSUPPORTED   # five hidden layers
        assert call(_params(encoder_past=[6, 512, 17])) == UNSUPPORTED            # not fdim wide
        assert call(_params(out_width=119)) == UNSUPPORTED
        assert call(_params(pos_width=2)) == UNSUPPORTED                          # a PECNet parameter block
        p = _params()
        p.encoder_dest.w[0] = None
        assert call(p) == INVALID
        assert call(_params(), n=-1) == INVALID
    assert fwd(_params(), n=0) == 0                # nothing to do
    assert fwd(_params(), past=None) == INVALID and fwd(_params(), saved=None) == INVALID
    assert lib.et_lbebm_train_fwd(None, 8, 1, 3, 8, 1, 3, 3, 8, 8, None, 0, None) == INVALID
    assert bwd(_params(), rs=-1) == INVALID
    p = _params()
    g = grads(p)
    g.predictor.db[3] = None
    assert bwd(p, g=g) == INVALID
    assert bwd(_params()) == WORKSPACE             # refused before the launch
    assert bwd(_params(), ws=8, nbytes=4 * 100 * (16 + 16 + 512 + 256 + 8 + 16 + 1024 + 512 + 256) - 4, n=100) == WORKSPACE
    ws = lambda p, n: int(lib.et_lbebm_train_workspace_bytes(C.byref(p), n))
    # the two encoders' outputs, then the hidden layers of encoder_past, encoder_dest (8, 16 in this block), predictor
    assert ws(_params(), 100) == 4 * 100 * (16 + 16 + 512 + 256 + 8 + 16 + 1024 + 512 + 256)
    assert ws(_params(), 0) == 0 and ws(_params(out_width=119), 100) == 0 and ws(_params(pos_width=2), 100) == 0
    assert ws(_params(), 3) == 4 * (2 * 48 + 3 * (512 + 256 + 8 + 16 + 1024 + 512 + 256))  # (3, 16) takes 48 floats
    assert ws(_params(encoder_dest=[2, 7, 16]), 3) == 4 * (2 * 48 + 3 * (512 + 256 + 1024 + 512 + 256) + 24)  # 21 -> 24
