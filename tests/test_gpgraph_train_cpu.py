"""GP-Graph-SGCN training without a GPU: the float64 restatement (tests/_gpgraph_train_np.py) against torch's float64 autograd
of the stock-torch twin (tests/_gpgraph_twin.py) -- the zero of the distance's backward at D == 0 and the straight-through
path included -- and against the reference's float64 gradients (fixture G30), the seed, band and non-vacuity conditions of
the GPU tests' scenes, the enable_native_training contract, the host-side argument checks of the new C entries and their
declarations."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from . import _abi_header as H
from . import _golden as G
from . import _gpgraph_np as GN
from . import _gpgraph_train_cases as CS
from . import _gpgraph_train_np as GT
from . import _gpgraph_twin as TW
from . import _sgcn_np as SN

G30 = G.load("g30_gpgraph_sgcn_train.npz")
G30_CASES = sorted({k.split(".")[0] for k in G30.files})
F64 = 1e-9   # float64 against float64: of each tensor's largest entry


def _equal(got, want, key, tm=None, floor=0.0):
    """within F64 of the tensor's largest entry -- or, for a sum that can cancel (a one-element tensor; group_cnn's bias, whose
    exact gradient is zero), within F64 of the sum of its terms' magnitudes"""
    scale = max(float(np.abs(want).max()), 1e-300, floor)
    if tm is not None and np.size(want) == 1:
        scale = max(scale, float(np.max(tm)))
    assert float(np.abs(got - want).max()) <= F64 * scale, (key, float(np.abs(got - want).max()), scale)


def _against(R, out, grads):
    _equal(R["out"].val, out, "out")
    wmax = float(np.abs(grads["group_gen.group_cnn.0.weight"]).max())
    for k, g in grads.items():
        if "key.bias" in k:   # an exact zero here, below rounding in autograd through the un-collapsed attention
            assert not R["grads"][k].val.any()
            assert np.abs(g).max() <= 1e-12 * np.abs(grads[k.replace("key.bias", "key.weight")]).max()
            continue
        # group_cnn's bias: its exact gradient is zero (the distance reads differences), both sides are noise below the weight's
        _equal(R["grads"][k].val, g, k, R["grads"][k].tm, floor=wmax if k == "group_gen.group_cnn.0.bias" else 0.0)
        assert (R["grads"][k].err >= 0).all() and np.isfinite(R["grads"][k].err).all()


@pytest.mark.parametrize("name,n", [("k1", 3), ("k2_wide", 2), ("et", 5), ("kmax", 3), ("deep", 4), ("et", 17)])
def test_restatement_equals_autograd_of_the_twin(name, n):
    va, vr = CS.scene(name, n)
    sd = CS.case_state(name, [va])
    d_out = CS.d_out(name, n)
    R = GT.run(sd, va, vr, d_out)
    out, idx, grads = TW.gradients(sd, va, vr, d_out)
    assert np.array_equal(idx, R["indices"])
    _equal(R["out"].val, GN.forward(sd, va, vr)["out"], "forward")
    _against(R, out, grads)
    for k in ("group_gen.th", "group_gen.group_cnn.0.weight", "group_mix.st_gcns_mix.1.weight"):   # the straight-through path is open
        assert np.abs(grads[k]).max() > 0, k


def test_coincident_pedestrians_and_the_diagonal():
    """D == 0 on the diagonal and between two pedestrians with the same v_abs: the norm's backward is 0 there in torch (the
    twin), and the restatement takes 0; the pair is close (d = 0 <= th) and shares a group"""
    name, n = "et", 5
    va, vr = CS.scene(name, n)
    va, vr = va.copy(), vr.copy()
    va[:, 3] = va[:, 1]
    vr[:, :, 3] = vr[:, :, 1]
    sd = CS.case_state(name, [va])
    d_out = CS.d_out(name, n)
    R = GT.run(sd, va, vr, d_out)
    assert R["dist"][1, 3] == 0 and R["indices"][1] == R["indices"][3]
    out, idx, grads = TW.gradients(sd, va, vr, d_out)
    assert np.array_equal(idx, R["indices"]) and all(np.isfinite(g).all() for g in grads.values())
    _against(R, out, grads)


@pytest.mark.parametrize("case", G30_CASES)
def test_restatement_equals_the_reference_g30(case):
    name = str(G30[f"{case}.config"])
    va, vr, d_out = G30[f"{case}.v_abs"], G30[f"{case}.v_rel"], G30[f"{case}.d_out"]
    sd = CS.case_state(name, [va])
    assert float(sd["group_gen.th"][0]) == float(G30[f"{case}.th"])
    R = GT.run(sd, va, vr, d_out)
    assert np.array_equal(R["indices"], G30[f"{case}.indices"])
    assert all(f[kind]["undecided"] == 0 for f in R["decisions"] for kind in ("mask", "prelu")) and R["pairs"]["undecided"] == 0
    want = CS.g30_gradients(G30, case, sd)
    wmax = float(np.abs(want["group_gen.group_cnn.0.weight"]).max())
    biggest = max(float(np.abs(g).max()) for g in want.values())
    for k, g in want.items():
        if va.shape[1] == 1 and k.startswith("group_gen"):   # one pedestrian: P = [[1]], an exact zero (the reference: noise)
            assert not R["grads"][k].val.any() and np.abs(g).max() <= 1e-12 * biggest, k
        elif "key.bias" not in k:
            _equal(R["grads"][k].val, g, k, R["grads"][k].tm, floor=wmax if k == "group_gen.group_cnn.0.bias" else 0.0)
    ref_out = G30[f"{case}.out32"]
    assert np.abs(R["out"].val - ref_out).max() <= SN.TOL * np.abs(ref_out).max()


def _figures(name, sd, va, vr, exact=False, single=True):
    n = va.shape[1]
    R = GT.run(sd, va, vr, CS.d_out(name, n))
    assert CS.within_caps(R["decisions"], R["pairs"], exact=exact), (name, n, R["decisions"], R["pairs"])
    if single:
        assert not GT.vacuous(R["grads"], n, R["n_groups"]), (name, n, GT.vacuous(R["grads"], n, R["n_groups"]))
        gb, gw = R["grads"]["group_gen.group_cnn.0.bias"], R["grads"]["group_gen.group_cnn.0.weight"]
        assert np.abs(gb.val).max() <= 1e-9 * np.abs(gw.val).max(), (name, n)   # group_cnn's bias: an exactly zero gradient
        if n >= 3:
            assert 1 < R["n_groups"] < n, (name, n, R["n_groups"])
    return R


def test_seeds_keep_the_bands_within_their_caps_and_the_bounds_tell():
    """with the restatement ALONE: every scene the GPU tests use, none filtered out.  Undecided mask logits and PReLU arguments
    within CAP_SCENE per pass, none in the exact cases; no undecided pair anywhere; every multi-element tensor's bound below half
    its largest entry (group_cnn's weight included; its bias has an exactly zero gradient, tests/_gpgraph_train_np.vacuous); 1 <
    G < n for n >= 3, and over the ragged cases a pooled pass with G <= 64 and one with G > 64; a real share of the pairs within 3 tau of th; a group of three or more; a merge that is not the connected
    components"""
    big_group = differs = 0
    groups = []
    for name in CS.EXACT_CONFIGS:
        for n in CS.EXACT_N:
            va, vr = CS.scene(name, n)
            R = _figures(name, CS.case_state(name, [va]), va, vr, exact=True)
            if n >= 2:
                assert R["pairs"]["near"] >= 1, (name, n, R["pairs"])   # the soft assignment is not saturated everywhere
    for name, n in CS.RAGGED:
        va, vr = CS.scene(name, n)
        R = _figures(name, CS.case_state(name, [va]), va, vr)
        assert R["pairs"]["near"] >= 0.1 * R["pairs"]["entries"], (name, n, R["pairs"])
        groups.append(R["n_groups"])
        big_group += int(np.bincount(R["indices"]).max() >= 3)
        close = R["dist"] <= R["th"]
        differs += int(not np.array_equal(GN.compact(GN.merge_union_find(close)), R["indices"]))
    assert big_group >= 1 and differs >= 1
    assert min(groups) <= 64 < max(groups), groups   # pooled passes on both sides of the wavefront edge
    for which in CS.LAYOUTS:
        name, sizes, C_obs, nrm = CS.layout(which)
        scenes = [GN.bridge_input(v) for _, _, _, v in SN.scenes_of(sizes, C_obs, nrm)]
        sd = CS.case_state(name, [va for va, _ in scenes])
        for va, vr in scenes:
            _figures(name, sd, va, vr, single=False)


def test_enable_native_training_contract():
    import eigentrajectory_amd as ET
    from eigentrajectory_amd._lib import ETLibraryError
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.gpgraph import GPGraph, GPGraphSGCN, GPGraphSTGCNN
    from eigentrajectory_amd.utils import default_hyper_params
    a, b = CS.module("et"), CS.module("et")
    keys = sorted(a.state_dict())
    assert a.native_training is False and "native_training" not in vars(a)
    assert ET.enable_native_training(a) is a and a.native_training is True and b.native_training is False  # per instance
    assert sorted(a.state_dict()) == keys and len(keys) == 97 + 6 and not any("native" in k for k in keys)
    assert list(a.state_dict()) == list(CS.state("et")) == [k for k, _ in a.named_parameters()]
    assert "native_training" not in dict(a.named_buffers()) and "native_training" not in dict(a.named_parameters())
    assert a.baseline_model.native_training is False   # the base on its own stays what it was
    va, vr = torch.zeros((1, 1, 8, 3)), torch.zeros((1, 2, 8, 3))
    with pytest.raises(RuntimeError, match=re.escape("GPGraph: only inference is native (no backward, no straight-through gradient); "
                                                     "training-mode forward is not implemented -- call .eval() first")):
        b(va, vr)   # without the flag: as before, word for word
    with pytest.raises(ETLibraryError, match="no CPU path"):
        a(va, vr)   # with it: the library is reached
    with pytest.raises(ETLibraryError, match="no CPU path"):
        a.eval()(va, vr)
    with pytest.raises(RuntimeError, match="no input gradient"):
        a.train()(va, vr.clone().requires_grad_(True))
    assert ET.enable_native_training(a, False) is a and a.native_training is False
    with pytest.raises(RuntimeError, match="training-mode forward is not implemented"):
        a(va, vr)
    wrapped = ET.EigenTrajectory(CS.module("et"), get_hook_func("gpgraphsgcn"), default_hyper_params(static_dist=0.3))
    assert ET.enable_native_training(wrapped) is wrapped and wrapped.baseline_model.native_training is True
    assert ET.enable_native_training(GPGraphSGCN(obs_len=8, pred_len=6, in_dims=1, out_dims=20)).native_training is True
    names = ("LBEBM", "PECNet", "SocialImplicitLight", "SGCN")
    with pytest.raises(NotImplementedError, match="GPGraph has no native backward pass") as exc:
        ET.enable_native_training(GPGraphSTGCNN(obs_len=8, pred_len=6, in_dims=1, out_dims=20))
    assert "BatchNorm" in str(exc.value) and all(nm in str(exc.value) for nm in names)
    cfg = SN.module_cfg("et")
    base = lambda **kw: ET.SGCN(position_channel=True, **{**cfg, **kw})
    wrap = lambda bm, **kw: GPGraph(bm, in_channels=1, out_channels=20, obs_seq_len=8, pred_seq_len=6, **kw)
    for m, field in ((wrap(base(), d_type="learned"), "d_type"), (wrap(base(), d_th=0.5), "d_th"), (wrap(base(), mix_type="mean"), "mix_type"),
                     (wrap(base(), group_type=(True, False, True)), "group_type"), (wrap(base(), weight_share=False), "weight_share"),
                     (wrap(base(dropout=0.1)), "dropout"), (wrap(ET.SGCN(**cfg)), "position_channel")):
        with pytest.raises(NotImplementedError, match="GPGraph has no native backward pass outside its native family") as exc:
            ET.enable_native_training(m)
        assert field in str(exc.value) and all(nm in str(exc.value) for nm in names), (field, str(exc.value))
    with pytest.raises(NotImplementedError, match="SGCN has no native backward pass outside its native family") as exc:
        ET.enable_native_training(base())   # a bare two-channel SGCN: refused as before
    assert "position_channel" in str(exc.value)
    with pytest.raises(NotImplementedError, match="Linear has no native backward pass") as exc:
        ET.enable_native_training(torch.nn.Linear(2, 2))
    assert all(nm in str(exc.value) for nm in names)


def _params(**kw):
    from eigentrajectory_amd import _lib
    from .test_sgcn_train_cpu import _params as base_params
    p = _lib.GPGraphSGCNParams()
    p.base = base_params(**{k: v for k, v in kw.items() if hasattr(p.base, k)})
    p.group_w = p.group_b = p.th = p.mix_a = p.mix_w = p.mix_b = 8
    p.tau = 0.1
    for k, v in kw.items():
        if not hasattr(p.base, k):
            setattr(p, k, v)
    return p


def test_arguments_are_validated_on_the_host():
    """every refusal below is answered before a launch: the calls run without a device"""
    from eigentrajectory_amd import _lib
    lib = _lib.lib()
    UNSUPPORTED, INVALID, WORKSPACE = (H.defines()[k] for k in ("ET_ERR_UNSUPPORTED", "ET_ERR_INVALID_ARG", "ET_ERR_WORKSPACE"))
    big = 1 << 40
    G_ = int(lib.et_gpgraph_sgcn_grad_floats(C.byref(_params())))
    assert G_ == sum(int(np.prod(np.asarray(w).shape)) for w in CS.state("et").values()) == 21050 + 64 + 33 + 1 + 120 * 360 + 120
    need = int(lib.et_gpgraph_sgcn_train_workspace_bytes(C.byref(_params()), 3, 9, 1))
    assert need > int(lib.et_gpgraph_sgcn_workspace_bytes(C.byref(_params()), 3, 9, 1)) > 0 and need % 16 == 0

    def graph(p, n=3, d=8, grads=8, gf=G_, ws=8, nbytes=big):
        return lib.et_gpgraph_sgcn_backward_graph(C.byref(p), n, d, grads, gf, ws, nbytes, None)

    def scenes(p, n=3, off=None, ns=0, n2=9, mx=3, d=8, grads=8, gf=G_, ws=8, nbytes=big):
        return lib.et_gpgraph_sgcn_backward_scenes(C.byref(p), n, off, ns, n2, mx, d, grads, gf, ws, nbytes, None)

    def fwd_graph(p, va=8, vr=8, n=3, out=8, ws=8, nbytes=big):
        return lib.et_gpgraph_sgcn_train_forward_graph(C.byref(p), va, vr, n, out, None, None, None, None, ws, nbytes, None)

    def fwd_scenes(p, c=8, nrm=8, n=3, out=8, ws=8, nbytes=big):
        return lib.et_gpgraph_sgcn_train_forward_scenes(C.byref(p), c, nrm, n, None, 0, 9, 3, out, None, None, None, None, ws,
                                                        nbytes, None)

    for call in (graph, scenes, fwd_graph, fwd_scenes):
        for bad in (dict(in_dims=2), dict(num_heads=2), dict(dropout=0.5), dict(n_asym=9), dict(pred_len=33, obs_len=35), dict(out_dims=65)):
            assert call(_params(**bad)) == UNSUPPORTED, (call.__name__, bad)
        assert call(_params(th=None)) == INVALID and call(_params(mix_w=None)) == INVALID and call(_params(tau=0.0)) == INVALID
        assert call(_params(), ws=None) == WORKSPACE and call(_params(), nbytes=need - 1) == WORKSPACE
        assert call(_params(), n=-1) == INVALID and call(_params(), n=_lib.SGCN_MAX_N + 1) == INVALID
    assert graph(_params(), d=None) == INVALID and graph(_params(), grads=None) == INVALID and graph(_params(), gf=G_ - 1) == INVALID
    assert graph(_params(), n=0) == INVALID
    assert scenes(_params(), d=None) == INVALID and scenes(_params(), grads=None) == INVALID and scenes(_params(), gf=3) == INVALID
    assert scenes(_params(), n2=-1) == INVALID and scenes(_params(), off=8, ns=0) == INVALID
    assert fwd_graph(_params(), va=None) == INVALID and fwd_graph(_params(), out=None) == INVALID
    assert fwd_scenes(_params(), c=None) == INVALID and fwd_scenes(_params(), out=None) == INVALID
    assert lib.et_gpgraph_sgcn_backward_graph(None, 3, 8, 8, G_, 8, big, None) == INVALID
    # outside the family: no workspace, no gradient buffer
    assert lib.et_gpgraph_sgcn_train_workspace_bytes(C.byref(_params(dropout=0.5)), 3, 9, 1) == 0
    assert lib.et_gpgraph_sgcn_train_workspace_bytes(C.byref(_params()), 0, 0, 1) == 0
    assert lib.et_gpgraph_sgcn_grad_floats(C.byref(_params(in_dims=2))) == 0 and lib.et_gpgraph_sgcn_grad_floats(C.byref(_params(th=None))) == 0


def test_abi_names_declared_and_mirrored():
    from eigentrajectory_amd import _lib, ops
    header = H.text()
    for name in ("et_gpgraph_sgcn_train_workspace_bytes", "et_gpgraph_sgcn_grad_floats", "et_gpgraph_sgcn_train_layout",
                 "et_gpgraph_sgcn_train_forward_graph", "et_gpgraph_sgcn_train_forward_scenes", "et_gpgraph_sgcn_backward_graph",
                 "et_gpgraph_sgcn_backward_scenes"):
        assert re.search(rf"\b{name}\(", header) and name in _lib.SYMBOLS and hasattr(_lib.lib(), name), name
    d = H.defines()
    assert d["ET_GPGRAPH_BWD_ROWS"] == _lib.GPGRAPH_BWD_ROWS
    F = _lib.GPGRAPH_SGCN_TRAIN_LAYOUT_FIELDS
    assert d["ET_GPGRAPH_SGCN_TRAIN_LAYOUT_FIELDS"] == F
    off = (C.c_int64 * F)()
    lib, p = _lib.lib(), _params()
    assert lib.et_gpgraph_sgcn_train_layout(C.byref(p), 3, 9, 1, off, F) == 0
    places = [x for i, x in enumerate(off) if i not in (4, 6, 12)]   # (the two strides and the tail's floats per row)
    assert places == sorted(places) and len(set(places)) == len(places) and places[0] > 0
    assert off[F - 1] * 4 == lib.et_gpgraph_sgcn_train_workspace_bytes(C.byref(p), 3, 9, 1)
    assert off[4] >= 8 * 4 * 27 and off[6] >= 9 * 4 * 64 and off[12] == (2 * 8 + 2 * 5 * 6) * 64   # 3 passes: 27 entries, 9 rows
    assert lib.et_gpgraph_sgcn_train_layout(C.byref(p), 3, 9, 1, off, 5) == d["ET_ERR_INVALID_ARG"]
    assert lib.et_gpgraph_sgcn_train_layout(C.byref(_params(dropout=0.5)), 3, 9, 1, off, F) == d["ET_ERR_UNSUPPORTED"]
    for fn in ("gpgraph_sgcn_train_workspace", "gpgraph_sgcn_train_forward_graph", "gpgraph_sgcn_train_forward_scenes",
               "gpgraph_sgcn_backward_graph", "gpgraph_sgcn_backward_scenes", "gpgraph_sgcn_grad_views", "gpgraph_sgcn_train_views"):
        assert callable(getattr(ops, fn))
