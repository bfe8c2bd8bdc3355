"""CPU checks of the native Social-STGCNN predictor (eigentrajectory_amd/stgcnn.py, csrc/et_stgcnn.hip): the numpy
restatement (tests/_stgcnn_np.py) against the reference's recorded outputs (tests/golden/g19_stgcnn.npz,
tools/make_golden_stgcnn.py), the module's state_dict against the reference's, and the refusal to run in training mode."""
import os
import re

import numpy as np
import pytest
import torch

from . import _abi_header as H
from . import _golden as G
from . import _stgcnn_np as SN

Z = G.load("g19_stgcnn.npz")
PICKS = sorted({k.split(".")[0] for k in Z.files if k.startswith("pick")}, key=lambda t: int(t[4:]))


def net_state(prefix="net."):
    return {k[len(prefix):]: Z[k] for k in Z.files if k.startswith(prefix) and not k[len(prefix):].startswith("net_out")}


def et_module(**kw):
    from eigentrajectory_amd.stgcnn import SocialSTGCNN
    args = dict(n_stgcnn=1, n_txpcnn=5, input_feat=1, output_feat=20, seq_len=8, pred_seq_len=6, kernel_size=3)
    args.update(kw)
    return SocialSTGCNN(**args)


def scale_close(got, ref, tol):
    ref = np.asarray(ref, np.float64)
    assert np.abs(np.asarray(got, np.float64) - ref).max() <= tol * np.abs(ref).max()


def test_fixture_covers_the_cases_the_tests_need():
    assert len(PICKS) >= 5
    sizes = [Z[f"{t}.v"].shape[-1] for t in PICKS]
    assert max(sizes) == max(int(Z[f"{s}.scene_size"].max()) for s in G.SCENES)  # the largest scene of all splits
    assert any(bool(Z[f"{t}.coincident"]) for t in PICKS)                      # equal coefficients in one time row
    for s in G.SCENES:
        assert Z[f"{s}.ade"].shape == (int(Z[f"{s}.scene_size"].sum()),)
    bn = net_state()
    assert not np.allclose(bn["st_gcns.0.tcn.0.running_var"], 1.0) and not np.allclose(bn["prelus.0.weight"], 0.25)


def test_numpy_restatement_reproduces_the_reference():
    sd = net_state()
    for t in PICKS:
        v, a = Z[f"{t}.v"][0, 0], Z[f"{t}.a"]
        scale_close(SN.adjacency(v), a, 1e-6)
        raw = SN.forward(sd, v, a)
        scale_close(raw, Z[f"{t}.net_out"][0], 1e-5)
        scale_close(SN.forward(sd, v), Z[f"{t}.net_out"][0], 1e-5)  # adjacency formed row by row
        scale_close(SN.c_pred_refine(raw), Z[f"{t}.c_pred_refine"], 1e-5)
    gen = net_state("gen.")
    for i, t in enumerate(PICKS[:2]):
        scale_close(SN.forward(gen, Z[f"{t}.v"][0, 0], n_stgcnn=2, n_txpcnn=3), Z[f"gen.net_out{i}"][0], 1e-5)


def test_state_dict_names_and_shapes_are_the_references():
    for prefix, kw in (("net.", {}), ("gen.", dict(n_stgcnn=2, n_txpcnn=3, output_feat=12))):
        ref = net_state(prefix)
        mine = et_module(**kw).state_dict()
        assert sorted(mine) == sorted(ref)
        assert all(tuple(mine[k].shape) == ref[k].shape for k in ref)
    sd = et_module().state_dict()
    assert "tpcnn_ouput.weight" in sd and "tpcnns.4.weight" in sd and "prelus.4.weight" in sd  # unused, but kept
    assert "st_gcns.0.residual.0.weight" in sd and "st_gcns.0.tcn.3.running_var" in sd


def test_reference_checkpoint_loads():
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    net = et_module()
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in net_state().items()})
    assert torch.equal(net.st_gcns[0].tcn[0].running_mean, torch.from_numpy(Z["net.st_gcns.0.tcn.0.running_mean"]))
    hp = default_hyper_params(static_dist=G.static_dist("eth"))
    model = EigenTrajectory(et_module(), get_hook_func("stgcnn"), hp)
    ckpt = model.state_dict()
    for k, v in net_state().items():
        ckpt[f"baseline_model.{k}"] = torch.from_numpy(np.array(v))
    for k in ckpt:
        if k.startswith("ET_"):
            ckpt[k] = torch.from_numpy(Z[f"eth.ET.{k}"])
    model.load_state_dict(ckpt)  # a reference ET-STGCNN checkpoint's keys, unchanged
    assert torch.equal(model.baseline_model.tpcnn_ouput.bias, torch.from_numpy(Z["net.tpcnn_ouput.bias"]))


def test_training_mode_forward_raises():
    net = et_module()
    assert net.training
    v, a = torch.zeros((1, 1, 8, 3)), torch.zeros((8, 3, 3))
    with pytest.raises(RuntimeError, match="training"):
        net(v, a)


def test_stgcnn_abi_names_declared_and_listed():
    from eigentrajectory_amd import _lib
    header = H.text()
    for name in ("et_stgcnn_workspace_bytes", "et_stgcnn_forward_scenes", "et_stgcnn_forward_graph"):
        assert re.search(rf"\b{name}\(", header) and name in _lib.SYMBOLS, name
    names = H.struct_fields("et_stgcnn_layer")
    assert names == [f for f, _ in _lib.STGCNNLayer._fields_]
    if os.path.exists(_lib.LIB_PATH):
        p = _lib.STGCNNParams()
        assert _lib.lib().et_stgcnn_workspace_bytes(_lib.C.byref(p), _lib.i64(10), _lib.i64(10)) == 0  # not taken
