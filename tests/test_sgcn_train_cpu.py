"""SGCN training without a GPU: the float64 restatement (tests/_sgcn_train_np.py) against torch's float64 autograd of the
stock-torch twin (tests/_sgcn_twin.py) and against the reference's float64 gradients (fixture G29), the collapsed-attention
chain rule, the seed and band conditions of the GPU tests' scenes, the enable_native_training contract, the host-side
argument checks of the new C entries and their declarations."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from . import _abi_header as H
from . import _golden as G
from . import _sgcn_np as SN
from . import _sgcn_train_cases as CS
from . import _sgcn_train_np as TN
from . import _sgcn_twin as TW

G29 = G.load("g29_sgcn_train.npz")
G29_CASES = sorted({k.split(".")[0] for k in G29.files})
F64 = 1e-9   # float64 against float64: of each tensor's largest entry


def _restated(name, v, d_out):
    ids, idt = SN.bridge_identities(v.shape[0], v.shape[1])
    return TN.run(SN.random_state(name), v, ids, idt, d_out), ids, idt


def _equal(got, want, key, tm=None):
    """within F64 of the tensor's largest entry -- or, for a one-element tensor, itself a sum that can cancel (a PReLU
    slope's gradient in a scene of one), within F64 of the sum of its terms' magnitudes ``tm``"""
    scale = max(float(np.abs(want).max()), 1e-300)
    if tm is not None and np.size(want) == 1:
        scale = max(scale, float(np.max(tm)))
    tol = F64 * scale
    assert float(np.abs(got - want).max()) <= tol, key


@pytest.mark.parametrize("name,n", [("k1", 3), ("k2_wide", 2), ("et", 5), ("kmax", 3), ("deep", 4)])
def test_restatement_equals_autograd_of_the_twin(name, n):
    v, d_out = CS.scene(name, n), CS.d_out(name, n)
    R, ids, idt = _restated(name, v, d_out)
    out, grads = TW.gradients(SN.random_state(name), v, ids, idt, d_out)
    _equal(R["out"].val, out, "out")
    ref, _, _ = SN.forward(SN.random_state(name), v, ids, idt)
    _equal(R["out"].val, ref, "forward")
    for k, g in grads.items():
        if "key.bias" in k:   # step 7: an exact zero here, below rounding in autograd through the un-collapsed attention
            assert not R["grads"][k].val.any()
            assert np.abs(g).max() <= 1e-12 * np.abs(grads[k.replace("key.bias", "key.weight")]).max()
            continue
        _equal(R["grads"][k].val, g, k, R["grads"][k].tm)
        assert (R["grads"][k].err >= 0).all() and np.isfinite(R["grads"][k].err).all()


@pytest.mark.parametrize("case", G29_CASES)
def test_restatement_equals_the_reference_g29(case):
    name = str(G29[f"{case}.config"])
    R, _, _ = _restated(name, G29[f"{case}.v"], G29[f"{case}.d_out"])
    assert all(f["undecided"] == 0 for f in R["decisions"].values()) or case == "et_real"
    want = CS.g29_gradients(G29, case, SN.random_state(name))
    for k, g in want.items():
        if "key.bias" not in k:
            _equal(R["grads"][k].val, g, k, R["grads"][k].tm)
    ref_out = G29[f"{case}.out32"]
    assert np.abs(R["out"].val - ref_out).max() <= SN.TOL * np.abs(ref_out).max()


def test_seeds_keep_the_bands_within_their_caps():
    """with the restatement ALONE: every scene the GPU tests use, none filtered out; the exact cases' bands are empty"""
    def fig(name, v):
        R = _restated(name, v, CS.d_out(name, v.shape[1]))[0]
        assert not TN.vacuous(R["grads"], v.shape[1]), (name, v.shape, TN.vacuous(R["grads"], v.shape[1]))   # the bounds can tell a wrong gradient
        return R["decisions"]
    for name in CS.EXACT_CONFIGS:
        for n in CS.EXACT_N:
            assert CS.within_caps(fig(name, CS.scene(name, n)), exact=True), (name, n)
    for name, n in CS.RAGGED:
        assert CS.within_caps(fig(name, CS.scene(name, n))), (name, n)
    for which in CS.LAYOUTS:
        name, sizes, C_obs, nrm = CS.layout(which)
        for s, lo, n, v in SN.scenes_of(sizes, C_obs, nrm):
            assert CS.within_caps(fig(name, v)), (which, s)


def test_enable_native_training_contract():
    import eigentrajectory_amd as ET
    from eigentrajectory_amd._lib import ETLibraryError
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    a, b = CS.module("et"), CS.module("et")
    keys = sorted(a.state_dict())
    assert a.native_training is False and "native_training" not in vars(a)
    assert ET.enable_native_training(a) is a and a.native_training is True and b.native_training is False  # per instance
    assert sorted(a.state_dict()) == keys and len(keys) == 97 and not any("native" in k for k in keys)
    assert "native_training" not in dict(a.named_buffers()) and "native_training" not in dict(a.named_parameters())
    v, ident = torch.zeros((1, 8, 3, 1)), [torch.eye(3)[None], torch.ones(3, 1, 1)]
    with pytest.raises(RuntimeError, match="training-mode forward is not implemented"):
        b(v, ident)   # without the flag: as before
    with pytest.raises(ETLibraryError, match="no CPU path"):
        a(v, ident)   # with it: the library is reached
    with pytest.raises(ETLibraryError, match="no CPU path"):
        a.eval()(v, ident)
    with pytest.raises(RuntimeError, match="no input gradient"):
        a.train()(v.clone().requires_grad_(True), ident)
    assert ET.enable_native_training(a, False) is a and a.native_training is False
    with pytest.raises(RuntimeError, match="training-mode forward is not implemented"):
        a(v, ident)
    wrapped = ET.EigenTrajectory(CS.module("et"), get_hook_func("sgcn"), default_hyper_params(static_dist=0.3))
    assert ET.enable_native_training(wrapped) is wrapped and wrapped.baseline_model.native_training is True
    cfg = SN.module_cfg("et")
    for kw, field in ((dict(in_dims=2), "in_dims"), (dict(dropout=0.1), "dropout"), (dict(position_channel=True), "position_channel")):
        with pytest.raises(NotImplementedError, match="SGCN has no native backward pass outside its native family") as exc:
            ET.enable_native_training(ET.SGCN(**{**cfg, **kw}))
        assert field in str(exc.value) and all(nm in str(exc.value) for nm in ("LBEBM", "PECNet", "SocialImplicitLight", "SGCN"))
    with pytest.raises(NotImplementedError, match="SGCN has no native backward pass"):
        ET.enable_native_training(ET.SGCN())


def _params(**kw):
    from eigentrajectory_amd import _lib
    p = _lib.SGCNParams()
    p.n_asym, p.embedding_dims, p.n_gcn_layers, p.obs_len, p.pred_len, p.n_tcn = 7, 64, 1, 8, 6, 5
    p.in_dims, p.out_dims, p.num_heads, p.dropout = 1, 20, 4, 0.0
    for a in range(2):
        for f in ("emb_w", "emb_b", "q_w", "q_b", "k_w", "k_b"):
            setattr(p.att[a], f, 8)
    p.fus_w = p.fus_b = p.fus_a = p.fusion_w = p.out_w = p.out_b = 8
    for j in range(8):
        for dst in (p.asym_s[j], p.asym_t[j]):
            dst.conv1_w = dst.conv2_w = dst.conv2_b = dst.act = 8
        p.tcn_w[j] = p.tcn_b[j] = p.tcn_a[j] = 8
    for g in range(4):
        p.gcn[g].w = p.gcn[g].act = 8
    for k, val in kw.items():
        setattr(p, k, val)
    return p


def test_arguments_are_validated_on_the_host():
    """every refusal below is answered before a launch: the calls run without a device"""
    from eigentrajectory_amd import _lib
    lib = _lib.lib()
    UNSUPPORTED, INVALID, WORKSPACE = (H.defines()[k] for k in ("ET_ERR_UNSUPPORTED", "ET_ERR_INVALID_ARG", "ET_ERR_WORKSPACE"))
    big = 1 << 40
    G_ = int(lib.et_sgcn_grad_floats(C.byref(_params())))
    assert G_ == 21050 == sum(int(np.prod(s)) for s in SN.state_shapes("et").values())
    need = int(lib.et_sgcn_train_workspace_bytes(C.byref(_params()), 3, 9, 1))
    assert need > int(lib.et_sgcn_workspace_bytes(C.byref(_params()), 3, 9, 1)) > 0 and need % 16 == 0

    def graph(p, ids=8, idt=8, s_t=1, t_t=1, n=3, d=8, grads=8, gf=G_, ws=8, nbytes=big):
        return lib.et_sgcn_backward_graph(C.byref(p), ids, s_t, idt, t_t, n, d, grads, gf, ws, nbytes, None)

    def scenes(p, n=3, off=None, ns=0, n2=9, mx=3, d=8, grads=8, gf=G_, ws=8, nbytes=big):
        return lib.et_sgcn_backward_scenes(C.byref(p), n, off, ns, n2, mx, d, grads, gf, ws, nbytes, None)

    def fwd_graph(p, v=8, ids=8, idt=8, n=3, out=8, ws=8, nbytes=big):
        return lib.et_sgcn_train_forward_graph(C.byref(p), v, ids, 1, idt, 1, n, out, None, None, ws, nbytes, None)

    def fwd_scenes(p, c=8, nrm=8, n=3, out=8, ws=8, nbytes=big):
        return lib.et_sgcn_train_forward_scenes(C.byref(p), c, nrm, n, None, 0, 9, 3, out, None, None, ws, nbytes, None)

    for call in (graph, scenes, fwd_graph, fwd_scenes):
        for bad in (dict(in_dims=2), dict(num_heads=2), dict(embedding_dims=32), dict(dropout=0.5), dict(n_asym=9),
                    dict(n_tcn=0), dict(pred_len=33, obs_len=35), dict(obs_len=9), dict(out_dims=65)):
            assert call(_params(**bad)) == UNSUPPORTED, (call.__name__, bad)
        p = _params()
        p.gcn[2].act = None
        assert call(p) == INVALID
        assert call(_params(), ws=None) == WORKSPACE and call(_params(), nbytes=need - 1) == WORKSPACE
        assert call(_params(), n=-1) == INVALID and call(_params(), n=_lib.SGCN_MAX_N + 1) == INVALID
    assert graph(_params(), d=None) == INVALID and graph(_params(), grads=None) == INVALID and graph(_params(), gf=G_ - 1) == INVALID
    assert graph(_params(), ids=None) == INVALID and graph(_params(), s_t=2) == INVALID and graph(_params(), n=0) == INVALID
    assert scenes(_params(), d=None) == INVALID and scenes(_params(), grads=None) == INVALID and scenes(_params(), gf=3) == INVALID
    assert scenes(_params(), n2=-1) == INVALID and scenes(_params(), off=8, ns=0) == INVALID
    assert fwd_graph(_params(), v=None) == INVALID and fwd_graph(_params(), out=None) == INVALID
    assert fwd_scenes(_params(), c=None) == INVALID and fwd_scenes(_params(), out=None) == INVALID
    assert lib.et_sgcn_backward_graph(None, 8, 1, 8, 1, 3, 8, 8, G_, 8, big, None) == INVALID
    assert lib.et_sgcn_train_workspace_bytes(C.byref(_params(dropout=0.5)), 3, 9, 1) == 0
    assert lib.et_sgcn_train_workspace_bytes(C.byref(_params()), 0, 0, 1) == 0 and lib.et_sgcn_grad_floats(C.byref(_params(in_dims=2))) == 0


def test_abi_names_declared_and_mirrored():
    from eigentrajectory_amd import _lib, ops
    header = H.text()
    for name in ("et_sgcn_train_workspace_bytes", "et_sgcn_grad_floats", "et_sgcn_train_layout", "et_sgcn_train_forward_graph",
                 "et_sgcn_train_forward_scenes", "et_sgcn_backward_graph", "et_sgcn_backward_scenes"):
        assert re.search(rf"\b{name}\(", header) and name in _lib.SYMBOLS and hasattr(_lib.lib(), name), name
    d = H.defines()
    assert (d["ET_SGCN_BWD_CHUNK"], d["ET_SGCN_BWD_ROWS"], d["ET_SGCN_BWD_ITEMS"]) == (_lib.SGCN_BWD_CHUNK, _lib.SGCN_BWD_ROWS,
                                                                                       _lib.SGCN_BWD_ITEMS)
    assert d["ET_SGCN_TRAIN_LAYOUT_FIELDS"] == _lib.SGCN_TRAIN_LAYOUT_FIELDS
    off = (C.c_int64 * _lib.SGCN_TRAIN_LAYOUT_FIELDS)()
    lib, p = _lib.lib(), _params()
    assert lib.et_sgcn_train_layout(C.byref(p), 3, 9, 1, off, _lib.SGCN_TRAIN_LAYOUT_FIELDS) == 0
    assert list(off) == sorted(off)[:0] + list(off) and off[-1] * 4 == lib.et_sgcn_train_workspace_bytes(C.byref(p), 3, 9, 1)
    assert off[4] >= 8 * 4 * 9 and off[6] >= 3 * 4 * 64 and off[12] == (2 * 8 + 2 * 5 * 6) * 64   # the strides, the tail's floats
    assert lib.et_sgcn_train_layout(C.byref(p), 3, 9, 1, off, 5) == d["ET_ERR_INVALID_ARG"]
    assert lib.et_sgcn_train_layout(C.byref(_params(dropout=0.5)), 3, 9, 1, off, 24) == d["ET_ERR_UNSUPPORTED"]
    for fn in ("sgcn_train_workspace", "sgcn_train_forward_graph", "sgcn_train_forward_scenes", "sgcn_backward_graph",
               "sgcn_backward_scenes", "sgcn_grad_views", "sgcn_train_views"):
        assert callable(getattr(ops, fn))
