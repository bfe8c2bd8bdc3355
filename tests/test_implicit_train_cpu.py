"""CPU checks of native Social-Implicit training (eigentrajectory_amd/implicit.py, csrc/et_implicit.hip "backward"): the
float64 restatement (tests/_implicit_train_np.py) against torch float64 autograd of a stock-torch twin
(tests/_implicit_twin.py) and against the reference's recorded gradients (tests/golden/g28_implicit_train.npz,
tools/make_golden_implicit_train.py), that no ReLU of any test input is undecided, the enable_native_training contract, the
new entry points' argument validation (host side, before any device work) and their declarations."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from . import _abi_header as H
from . import _golden as G
from . import _implicit_np as IN
from . import _implicit_train_cases as CS
from . import _implicit_train_np as TN
from . import _implicit_twin as TW
from .test_implicit_cpu import _params

from eigentrajectory_amd._lib import IMPLICIT_BWD_CHUNK as CHUNK  # noqa: E402

Z = CS.Z
G28 = G.load("g28_implicit_train.npz")
G28_CASES = sorted({k.split(".")[0] for k in G28.files})
# two float64 evaluations of the same sums, each within 2^-53 / 2^-24 = 2^-29 of the restatement's fp32 bound of the exact
# value, in any order of summation: 2^-28 of it apart, 2^-27 with room for the second-order terms
F64_SCALE = 2.0 ** -27


def g28_inputs(name):
    config = "gen" if name.startswith("gen") else "et"
    return config, Z[str(G28[f"{name}.v_key"])][0, 0], G28[f"{name}.G"][0], CS.CONFIGS[config]["bins"]


def twin_grads(sd, v, Gn, bins):
    """torch float64 autograd of the twin -> (out (S, T_out, N), {key: gradient, zeros where autograd left None})"""
    P = {k: torch.tensor(np.asarray(a, np.float64), requires_grad=True) for k, a in sd.items()}
    out = TW.forward(P, torch.tensor(np.asarray(v, np.float64))[None, None], bins)
    (out[0] * torch.tensor(np.asarray(Gn, np.float64))).sum().backward()
    return out[0].detach().numpy(), {k: (np.zeros(p.shape) if p.grad is None else p.grad.numpy()) for k, p in P.items()}


@pytest.mark.parametrize("name", ["pick2", "pick3", "edges", "lonely", "single", "gen0", "gen1", "movedbins", "s1", "t1"])
def test_restatement_equals_torch_float64_autograd(name):
    if name in G28_CASES:
        config, v, Gn, bins = g28_inputs(name)
    else:
        config, v, Gn, bins = CS.synthetic_cases(CHUNK)[name]
        bins = bins or CS.CONFIGS[config]["bins"]
    sd = CS.state(CS.module(config))
    r = TN.run(sd, v, Gn, bins)
    out, grads = twin_grads(sd, v, Gn, bins)
    assert np.abs(out - r["out"]).max() <= 1e-12 * np.abs(r["out"]).max()
    assert np.abs(r["out"] - IN.forward(sd, v, bins)).max() <= 1e-12 * np.abs(r["out"]).max()  # the inference restatement
    worst = 0.0
    for key in r["grads"]:
        ok, ratio, same = TN.compare(grads[key], r["grads"][key], r["grads_err"][key] * F64_SCALE)
        worst = max(worst, ratio)
        assert ok, (name, key, ratio)
    assert sorted(r["grads"]) == sorted(k for k in sd if not k.endswith("noise_w"))
    print(f"{name}: restatement against torch float64 autograd, {worst:.3f} of the float64 bound")


@pytest.mark.parametrize("name", G28_CASES)
def test_restatement_against_g28(name):
    """the reference's float64 gradients within the float64 bound, its fp32 gradients within the fp32 bound; visited = the
    zone has a member; NaN patterns equal; noise_w exactly 0"""
    config, v, Gn, bins = g28_inputs(name)
    sd = CS.state(CS.module(config))
    r = TN.run(sd, v, Gn, bins)
    n_bins = len(bins)
    assert r["undecided"] == 0
    assert np.array_equal(G28[f"{name}.visited"], r["visited"]) and not G28[f"{name}.nan_differs"].any()
    want, bound = TN.block(sd, r["grads"], n_bins), TN.block(sd, r["grads_err"], n_bins)
    g64, g32 = G28[f"{name}.grads64"], G28[f"{name}.grads32"]
    assert g64.dtype == np.float64 and g32.dtype == np.float32 and g64.shape == (n_bins, want.shape[1] + 1)
    assert not g64[:, -1].any() and not g32[:, -1].any()
    ok, ratio, same = TN.compare(g64[:, :-1], want, bound * F64_SCALE)
    assert ok and same, (name, ratio)
    ok32, ratio32, same32 = TN.compare(g32[:, :-1], want, bound)
    assert ok32 and same32, (name, ratio32)
    assert not g64[~r["visited"]].any()
    if name == "nan":
        assert np.isnan(g64).any() and np.isfinite(g64[r["visited"]]).any()
    print(f"{name}: {ratio:.3f} of the float64 bound, torch's fp32 gradients {ratio32:.3f} of the fp32 bound")


def test_no_relu_of_any_test_input_is_undecided():
    """every input of the GPU tests: the restatement alone decides every ReLU mask, so no GPU comparison hides behind one"""
    from eigentrajectory_amd._lib import IMPLICIT_BWD_CHUNK
    states = {c: CS.state(CS.module(c)) for c in CS.CONFIGS}
    for name, (config, v, Gn, bins) in CS.synthetic_cases(IMPLICIT_BWD_CHUNK).items():
        r = TN.run(states[config], v, Gn, bins or CS.CONFIGS[config]["bins"])
        assert r["undecided"] == 0, name
        assert np.isfinite(TN.block(states[config], r["grads_err"], len(r["visited"]))).all(), name
    for name in G28_CASES:
        config, v, Gn, bins = g28_inputs(name)
        assert TN.run(states[config], v, Gn, bins)["undecided"] == 0, name
    # an exact zero pre-activation (a zeroed channel) is decided: every term of it is an exact zero in the kernel too
    sd = dict(states["et"])
    for i in range(4):
        for pre in ("", "ped."):
            for kind in ("weight", "bias"):
                key = f"implicit_cells.{i}.{pre}feat.{kind}"
                sd[key] = sd[key].copy()
                sd[key][7] = 0
    v = Z["pick2.v"][0, 0]
    r = TN.run(sd, v, CS.grad_out("et", v.shape[1], 51))
    assert r["undecided"] == 0
    for i in range(4):
        assert not r["grads"][f"implicit_cells.{i}.feat.weight"][7].any() and not r["grads_err"][f"implicit_cells.{i}.feat.bias"][7]
    # and a pre-activation inside its bound is counted
    sd = dict(states["et"])
    key = "implicit_cells.2.ped.feat.bias"
    x = Z["single.v"][0, 0].astype(np.float64)[:, 0]
    w = np.asarray(sd["implicit_cells.2.ped.feat.weight"], np.float64)[3, 0]
    sd[key] = sd[key].copy()
    sd[key][3] = np.float32(-(w[1] * x[0] + w[2] * x[1]))  # channel 3 at t = 0: pre = a rounding error
    assert TN.run(sd, Z["single.v"][0, 0], CS.grad_out("et", 1, 52))["undecided"] >= 1


def test_enable_native_training_contract():
    import eigentrajectory_amd as ET
    from eigentrajectory_amd._lib import ETLibraryError
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    a, b = CS.module("et"), CS.module("et")
    keys = sorted(a.state_dict())
    assert a.native_training is False and "native_training" not in vars(a)
    assert ET.enable_native_training(a) is a and a.native_training is True and b.native_training is False  # per instance
    assert sorted(a.state_dict()) == keys and len(keys) == 4 * 19 and not any("native" in k for k in keys)
    assert "native_training" not in dict(a.named_buffers()) and "native_training" not in dict(a.named_parameters())
    v = torch.zeros((1, 1, 8, 3))
    assert b.training
    with pytest.raises(RuntimeError, match="training"):
        b(v)  # without the flag: as before
    with pytest.raises(ETLibraryError, match="no CPU path"):
        a(v)  # with it: the library is reached
    with pytest.raises(ETLibraryError, match="no CPU path"):
        a.eval()(v)  # eval mode: the inference path, whatever the flag
    with pytest.raises(ETLibraryError, match="no CPU path"):
        b.eval()(v)
    with pytest.raises(RuntimeError, match="no input gradient"):
        a.train()(v.clone().requires_grad_(True))
    assert ET.enable_native_training(a, False) is a and a.native_training is False
    with pytest.raises(RuntimeError, match="training"):
        a(v)
    wrapped = ET.EigenTrajectory(CS.module("et"), get_hook_func("implicit"), default_hyper_params(static_dist=0.3))
    assert ET.enable_native_training(wrapped) is wrapped and wrapped.baseline_model.native_training is True
    for other in (ET.SGCN(), torch.nn.Linear(2, 2)):
        with pytest.raises(NotImplementedError, match=f"{type(other).__name__} has no native backward pass") as exc:
            ET.enable_native_training(other)
        assert all(name in str(exc.value) for name in ("LBEBM", "PECNet", "SocialImplicitLight"))
    names = a.cell_parameter_names()
    assert names == [k for k, _ in a.named_parameters()] or sorted(names) == keys
    assert [p.shape for p in a.cell_parameters()] == [a.state_dict()[k].shape for k in names]


def test_backward_arguments_are_validated_on_the_host():
    """Every refusal below is answered before a launch: the calls run without a device."""
    from eigentrajectory_amd import _lib
    lib = _lib.lib()
    UNSUPPORTED, INVALID, WORKSPACE = (H.defines()[k] for k in ("ET_ERR_UNSUPPORTED", "ET_ERR_INVALID_ARG",
                                                                "ET_ERR_WORKSPACE"))
    big = 1 << 24

    def graph(p, v=8, n=3, fws=8, fbytes=big, g=8, layout=0, grads=8, ws=8, nbytes=big):
        return lib.et_implicit_backward_graph(C.byref(p), v, n, fws, fbytes, g, layout, grads, ws, nbytes, None)

    def scenes(p, n=3, fws=8, fbytes=big, g=8, grads=8, ws=8, nbytes=big):
        return lib.et_implicit_backward_scenes(C.byref(p), n, fws, fbytes, g, grads, ws, nbytes, None)

    for call in (graph, scenes):
        assert call(_params(spatial_output=65)) == UNSUPPORTED
        assert call(_params(temporal_input=17)) == UNSUPPORTED
        assert call(_params(temporal_output=17)) == UNSUPPORTED
        assert call(_params(spatial_input=2)) == UNSUPPORTED
        assert call(_params(n_bins=0)) == UNSUPPORTED and call(_params(n_bins=9)) == UNSUPPORTED
        p = _params()
        p.bins[2] = float("nan")
        assert call(p) == UNSUPPORTED
        p = _params()
        p.cells[1].global_t[3] = None
        assert call(p) == INVALID
        assert call(_params(), g=None) == INVALID and call(_params(), grads=None) == INVALID
        assert call(_params(), n=-1) == INVALID
        assert call(_params(), fws=None) == WORKSPACE and call(_params(), ws=None) == WORKSPACE
        assert call(_params(), fbytes=3 * 8 * 4 - 1) == WORKSPACE
        assert call(_params(), nbytes=4 * 1058 * 4 - 1) == WORKSPACE
    assert lib.et_implicit_backward_graph(None, 8, 3, 8, big, 8, 0, 8, 8, big, None) == INVALID
    assert lib.et_implicit_backward_scenes(None, 3, 8, big, 8, 8, 8, big, None) == INVALID
    assert graph(_params(), v=None) == INVALID and graph(_params(), layout=2) == INVALID and graph(_params(), layout=-1) == INVALID
    assert graph(_params(), n=_lib.SCENE_MAX_N + 1) == INVALID
    assert scenes(_params(temporal_input=2)) == UNSUPPORTED  # as the forward: v = [C_obs; obs_ori]
    assert scenes(_params(), fbytes=3 * (8 + 8) * 4 - 1) == WORKSPACE  # the table and every scene's v
    # workspace: one block per chunk of rows and cell
    ws = lambda p, n: int(lib.et_implicit_backward_workspace_bytes(C.byref(p), n))
    c = _lib.IMPLICIT_BWD_CHUNK
    assert ws(_params(), 1) == ws(_params(), c) == 4 * 1058 * 4 and ws(_params(), c + 1) == 2 * 4 * 1058 * 4
    assert ws(_params(), 0) == 0 and ws(_params(spatial_output=65), 5) == 0
    p = _params(spatial_output=64, temporal_input=16, temporal_output=16, n_bins=8)
    for b, val in enumerate(CS.BIG_BINS):
        p.bins[b] = val
    assert ws(p, 1) == 8 * 4802 * 4  # the largest block of the family


def test_backward_abi_names_declared_and_mirrored():
    from eigentrajectory_amd import _lib, ops
    header = H.text()
    for name in ("et_implicit_backward_workspace_bytes", "et_implicit_backward_graph", "et_implicit_backward_scenes"):
        assert re.search(rf"\b{name}\(", header) and name in _lib.SYMBOLS and hasattr(_lib.lib(), name), name
    d = H.defines()
    assert d["ET_IMPLICIT_BWD_CHUNK"] == _lib.IMPLICIT_BWD_CHUNK and d["ET_IMPLICIT_G_STN"] == 0 and d["ET_IMPLICIT_G_TNS"] == 1
    p = _params()
    assert ops.implicit_grad_size(p) == 1058 == sum(int(np.prod(s)) for s in TN.shapes(CS.state(CS.module("et"))).values())
    for fn in ("implicit_workspace", "implicit_backward_graph", "implicit_backward_scenes", "implicit_grad_views"):
        assert callable(getattr(ops, fn))
