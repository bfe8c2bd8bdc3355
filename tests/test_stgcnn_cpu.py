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
ZB = G.load("g19b_stgcnn_generic.npz")
TOL = 1e-5  # the GPU tests' bound (tests/test_gpu_stgcnn.py)
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


def test_numpy_restatement_reproduces_the_generic_recorded_calls():
    """g19b: n_txpcnn = 1, 2 and 8, three and eight st_gcn layers, k = 1, a given non-symmetric a -- against the reference's
    float32 output within 1e-5 of the largest entry, against its float64 output of the same call within 1e-9 (two float64
    evaluations of one formula)"""
    assert [tuple(int(c) for c in ZB[f"c{i}.cfg"]) for i in range(4)] == [(1, 1, 20, 6), (1, 2, 5, 1), (3, 8, 7, 3), (8, 3, 4, 2)]
    assert G.manifest()["g19b_stgcnn_generic"]["configs"] == [[1, 1, 20, 6], [1, 2, 5, 1], [3, 8, 7, 3], [8, 3, 4, 2]]
    for i in range(4):
        n_st, n_tp, S, k = (int(c) for c in ZB[f"c{i}.cfg"])
        pre = f"c{i}.sd."
        sd = {key[len(pre):]: ZB[key] for key in ZB.files if key.startswith(pre)}
        mine = et_module(**SN.module_kw(n_st, n_tp, S, k)).state_dict()
        assert sorted(mine) == sorted(sd) and all(tuple(mine[key].shape) == sd[key].shape for key in sd)
        for call in ("s3", "s11", "ns"):
            v, a = ZB[f"c{i}.{call}.v"], ZB[f"c{i}.{call}.a"]
            assert v.shape == (1, 1, k + 2, a.shape[-1]) and ZB[f"c{i}.{call}.out"].shape == (1, S, k, a.shape[-1])
            raw = SN.forward(sd, v[0, 0], a, n_stgcnn=n_st, n_txpcnn=n_tp)
            scale_close(raw, ZB[f"c{i}.{call}.out"][0], 1e-5)
            scale_close(raw, ZB[f"c{i}.{call}.out64"][0], 1e-9)
            if call == "ns":
                assert np.abs(a - np.swapaxes(a, 1, 2)).max() > 0.5  # far from symmetric
                scale_close(SN.forward(sd, v[0, 0], a, n_stgcnn=n_st, n_txpcnn=n_tp, dtype=np.float32),
                            ZB[f"c{i}.{call}.out64"][0], 1e-5)
            else:
                scale_close(SN.adjacency(v[0, 0]), a, 1e-6)
                scale_close(SN.forward(sd, v[0, 0], n_stgcnn=n_st, n_txpcnn=n_tp), ZB[f"c{i}.{call}.out64"][0], 1e-5)
        assert len(np.unique(ZB[f"c{i}.s11.v"][0, 0, 0])) == 10  # the coincident pair


def test_arena_restatement_gives_the_tabulated_sizes():
    for name, cfg in SN.CONFIGS.items():
        assert (SN.arena_per_ped(*cfg), SN.lds_max_n(*cfg)) == SN.ARENA[name], name


@pytest.mark.parametrize("k", [1, 6, 32])
def test_exact_split_is_exact(k):
    """the float32 mean of rows 0-1 of nrm over every scene equals the float64 mean exactly, in numpy's order, in a plain
    left-to-right float32 sum and in its reverse, and scene_input equals the float64 difference exactly; every row has ties
    and one scene has a row in which all pedestrians coincide"""
    sizes = [1, 2, 3, 32, 33, 34, 0, 71, 2, 773, 4096]
    C_obs, nrm = SN.exact_split(sizes, k, 3)
    assert C_obs.dtype == nrm.dtype == np.float32 and C_obs.shape == (k, sum(sizes)) and nrm.shape == (4, sum(sizes))
    assert np.array_equal(nrm[:2] * 64, np.round(nrm[:2] * 64)) and np.abs(nrm[:2]).max() <= 64
    lo, centres, coincident = 0, [], 0
    for n in sizes:
        if n == 0:
            continue
        rows = nrm[:2, lo:lo + n]
        m64 = rows.astype(np.float64).mean(axis=1)
        assert np.array_equal(rows.mean(axis=1, dtype=np.float32).astype(np.float64), m64)
        for order in (rows, rows[:, ::-1]):
            acc = np.zeros(2, np.float32)
            for col in order.T:
                acc = acc + col
            assert acc.dtype == np.float32 and np.array_equal((acc / np.float32(n)).astype(np.float64), m64)
        v = SN.scene_input(C_obs, nrm, lo, lo + n)
        assert v.dtype == np.float32 and np.array_equal(v[:k], C_obs[:, lo:lo + n])
        assert np.array_equal(v[k:].astype(np.float64), rows.astype(np.float64) - m64[:, None])
        if n >= 4:
            assert all(len(np.unique(r)) < n for r in v)  # ties in every row
        coincident += any(len(np.unique(r)) == 1 for r in v) and n >= 4
        centres += list(m64)
        lo += n
    assert len(set(centres)) == len(centres) and coincident == 1


def _generic_net(name, seed=0):
    net = et_module(**SN.module_kw(*SN.CONFIGS[name]))
    return SN.random_state(net, seed), net


def test_random_state_leaves_no_default():
    sd, net = _generic_net("gen")
    fresh = et_module(**SN.module_kw(*SN.CONFIGS["gen"])).state_dict()
    again = _generic_net("gen")[0]
    assert any(not np.array_equal(val, _generic_net("gen", 1)[0][key]) for key, val in sd.items())
    slopes = []
    for key, val in sd.items():
        if key.endswith("num_batches_tracked"):
            continue
        assert np.array_equal(val, net.state_dict()[key].numpy()) and val.dtype == np.float32
        assert not np.any(val == fresh[key].numpy()), key  # every entry moved
        assert np.array_equal(val, again[key]), key         # and a function of the seed alone
        if key.endswith("running_var"):
            assert 0.5 <= val.min() and val.max() <= 2.0
        if key.endswith("running_mean"):
            assert np.all(val != 0)
        if val.shape == (1,):
            slopes.append(float(val[0]))
    assert len(slopes) == 2 * 2 + 3 and len(set(slopes)) == len(slopes) and all(abs(s - 0.25) > 1e-4 for s in slopes)


@pytest.mark.parametrize("name", list(SN.CONFIGS))
def test_float32_restatement_is_within_an_eighth_of_the_tolerance(name):
    """the reference arithmetic's own float32 rounding, on the inputs and sizes the GPU tests run: TOL is at least 8 times
    it.  The kernels are not involved."""
    cfg = SN.CONFIGS[name]
    sd, _ = _generic_net(name)
    sizes = SN.split_sizes(name)
    C_obs, nrm = SN.exact_split(sizes, cfg[3], 1)
    lo, worst = 0, 0.0
    for n in sizes:
        if n:
            v = SN.scene_input(C_obs, nrm, lo, lo + n)
            r64 = SN.forward(sd, v, n_stgcnn=cfg[0], n_txpcnn=cfg[1])
            r32 = SN.forward(sd, v, n_stgcnn=cfg[0], n_txpcnn=cfg[1], dtype=np.float32)
            assert r32.dtype == np.float32 and np.isfinite(r64).all()
            err = float(np.abs(r32 - r64).max() / np.abs(r64).max())
            worst = max(worst, err)
            assert err <= TOL / 8, (name, n, err)
        lo += n
    print(f"{name}: float32 restatement within {worst:.2e} of the float64 one")


def test_bn_eps_reaches_the_restatement():
    sd, _ = _generic_net("gen")
    v = SN.scene_input(*SN.exact_split([5], 6, 2), 0, 5)
    a, b = (SN.forward(sd, v, n_stgcnn=2, n_txpcnn=3, eps=e) for e in (1e-5, 1e-3))
    assert np.abs(a - b).max() > 1e-4 * np.abs(a).max()


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
