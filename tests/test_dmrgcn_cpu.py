"""CPU checks of the native DMRGCN predictor (eigentrajectory_amd/dmrgcn.py, csrc/et_dmrgcn.hip): the numpy restatement
(tests/_dmrgcn_np.py) against the reference's recorded outputs (tests/golden/g23_dmrgcn.npz, tools/make_golden_dmrgcn.py),
that the fixture tells open from closed bins, the module's state_dict against the reference's, the entry points' argument
validation (host side, before any device work) and the refusal to run in training mode."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from . import _abi_header as H
from . import _dmrgcn_np as DN
from . import _golden as G

Z = G.load("g23_dmrgcn.npz")
PICKS = sorted({k.split(".")[0] for k in Z.files if k.startswith("pick")}, key=lambda t: int(t[4:]))
TOL = 1e-5  # of the largest entry; the reference's own fp32 run against its fp64 run differs by 3.5e-7


def net_state(prefix="net."):
    return {k[len(prefix):]: Z[k] for k in Z.files if k.startswith(prefix) and not k[len(prefix):].startswith("net_out")}


def et_module(**kw):
    from eigentrajectory_amd.dmrgcn import SocialDMRGCN
    args = dict(n_stgcn=1, n_tpcnn=4, input_feat=1, output_feat=20, seq_len=8, pred_seq_len=6, kernel_size=3)
    args.update(kw)
    return SocialDMRGCN(**args)


def scale_err(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


def test_fixture_covers_the_cases_the_tests_need():
    sizes = [Z[f"{t}.v"].shape[-1] for t in PICKS]
    assert max(sizes) == max(int(Z[f"{s}.scene_size"].max()) for s in G.SCENES)  # the largest scene of all splits
    assert {str(Z[f"{t}.split"]) for t in PICKS} == set(G.SCENES)
    assert any(bool(Z[f"{t}.coincident"]) and sz <= 30 for t, sz in zip(PICKS, sizes))
    assert any(bool(Z[f"{t}.boundary"]) for t in PICKS)
    for s in G.SCENES:
        n = int(Z[f"{s}.scene_size"].sum())
        assert Z[f"{s}.ade"].shape == Z[f"{s}.fde"].shape == (n,) and Z[f"{s}.robust"].shape == Z[f"{s}.scene_size"].shape
    sd = net_state()
    slopes = [float(v.reshape(-1)[0]) for k, v in sd.items() if v.size == 1]
    assert len(slopes) == 2 + 3 * 4 and len(set(slopes)) == len(slopes) and 0.25 not in slopes  # every PReLU its own slope
    a = Z["grid.a"][0]
    assert Z["grid.v"].shape == (1, 1, 8, 12) and Z["single.v"].shape == (1, 1, 8, 1)
    for r in range(2):
        for s in DN.SPLIT[r][1:]:
            assert (a[r] == np.float32(s)).any(), (r, s)  # pairs exactly on every split value
    assert ((a[0][1] == 0) & ~np.eye(12, dtype=bool)).any()


def test_numpy_restatement_reproduces_the_reference():
    sd = net_state()
    worst = 0.0
    for t in PICKS + ["grid", "single"]:
        v, a = Z[f"{t}.v"][0, 0], Z[f"{t}.a"][0]
        assert np.array_equal(DN.adjacency(v), a), t  # the bridge's fp32 distances, bit for bit
        raw = DN.forward(sd, v, a)
        errs = (scale_err(raw, Z[f"{t}.net_out"][0]), scale_err(DN.forward(sd, v), Z[f"{t}.net_out"][0]),
                scale_err(DN.c_pred_refine(raw), Z[f"{t}.c_pred_refine"]))
        worst = max(worst, *errs)
        assert max(errs) <= TOL, (t, errs)
    gen = net_state("gen.")
    for i, t in enumerate(PICKS[:2]):
        err = scale_err(DN.forward(gen, Z[f"{t}.v"][0, 0], n_stgcn=2, n_tpcnn=2), Z[f"gen.net_out{i}"][0])
        worst = max(worst, err)
        assert err <= TOL, (t, err)
    print(f"restatement against the reference: {worst:.2e} of the largest entry")


def test_closed_intervals_miss_the_bound_on_the_grid_scene():
    """a distance equal to a split value is in NO bin (clip_adjacency_matrix zeroes both ends): the variant with <= differs"""
    sd = net_state()
    v = Z["grid.v"][0, 0]
    assert scale_err(DN.forward(sd, v, closed=True), Z["grid.net_out"][0]) > TOL
    assert scale_err(DN.forward(sd, v), Z["grid.net_out"][0]) <= TOL


def test_state_dict_names_and_shapes_are_the_references():
    for prefix, kw in (("net.", {}), ("gen.", dict(n_stgcn=2, n_tpcnn=2, output_feat=12))):
        ref = net_state(prefix)
        net = et_module(**kw)
        mine = net.state_dict()
        assert sorted(mine) == sorted(ref)
        assert all(tuple(mine[k].shape) == ref[k].shape for k in ref)
        net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in ref.items()}, strict=True)
        assert torch.equal(net.tpcnns[0].residual[0].bias, torch.from_numpy(ref["tpcnns.0.residual.0.bias"]))
    sd = et_module().state_dict()
    assert "st_dmrgcns.0.gcns.1.conv.weight" in sd and "st_dmrgcns.0.residual.0.weight" in sd
    assert "tpcnns.3.gtacn.0.1.weight" in sd and "tpcnns.1.residual.0.weight" not in sd
    assert not any("running" in k for k in sd)  # no BatchNorm anywhere
    assert et_module().split == [[0, 0.25, 0.5, 0.75, 1], [0, 0.5, 1, 2, 4]]


def test_reference_checkpoint_loads_into_the_wrapper():
    from eigentrajectory_amd import EigenTrajectory, SocialDMRGCN
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    assert SocialDMRGCN is type(et_module())
    g2 = G.load("g2_fit_all_scenes.npz")
    hp = default_hyper_params(static_dist=G.static_dist("eth"))
    model = EigenTrajectory(et_module(), get_hook_func("dmrgcn"), hp)
    ckpt = model.state_dict()
    for k, v in net_state().items():
        ckpt[f"baseline_model.{k}"] = torch.from_numpy(np.array(v))
    for k in ckpt:
        if k.startswith("ET_"):
            ckpt[k] = torch.from_numpy(g2[f"eth.{k}"])
    model.load_state_dict(ckpt, strict=True)  # a reference ET-DMRGCN checkpoint's keys, unchanged
    assert torch.equal(model.baseline_model.st_dmrgcns[0].prelu.weight, torch.from_numpy(Z["net.st_dmrgcns.0.prelu.weight"]))


def test_training_mode_forward_raises():
    net = et_module()
    assert net.training
    with pytest.raises(RuntimeError, match="training"):
        net(torch.zeros((1, 1, 8, 3)), torch.zeros((1, 2, 8, 3, 3)))


def _params(**kw):
    """et_dmrgcn_params of the ET configuration whose every pointer is a (never dereferenced) non-NULL host address"""
    from eigentrajectory_amd import _lib
    p = _lib.DMRGCNParams()
    p.n_stgcn, p.n_tpcnn, p.input_feat, p.output_feat, p.seq_len, p.pred_seq_len, p.kernel_size = 1, 4, 1, 20, 8, 6, 3
    for r, s in enumerate(DN.SPLIT):
        for b, val in enumerate(s):
            p.split[r][b] = val
    dummy = C.addressof(C.c_float(0.0)) or 8
    for i in range(_lib.DMRGCN_MAX_STGCN):
        l = p.st_dmrgcns[i]
        for r in range(2):
            l.gcn_w[r], l.gcn_b[r] = dummy, dummy
        l.tcn_prelu = l.tcn_w = l.tcn_b = l.prelu = dummy
        if i == 0:
            l.res_w = l.res_b = dummy
    for j in range(_lib.DMRGCN_MAX_TPCNN):
        t = p.tpcnns[j]
        for m in range(2):
            t.conv_w[m], t.conv_b[m], t.conv_a[m] = dummy, dummy, dummy
        t.gta_w = t.gta_b = t.gta_a = dummy
        if j == 0:
            t.res_w = t.res_b = dummy
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_arguments_are_validated_on_the_host():
    """Every refusal below is answered before a launch: the calls run without a device."""
    from eigentrajectory_amd import _lib
    lib = _lib.lib()
    UNSUPPORTED, INVALID = H.defines()["ET_ERR_UNSUPPORTED"], H.defines()["ET_ERR_INVALID_ARG"]

    def graph(p):
        return lib.et_dmrgcn_forward_graph(C.byref(p), 8, 8, 3, 8, None, 0, None)

    def scenes(p):
        return lib.et_dmrgcn_forward_scenes(C.byref(p), 8, 8, 3, None, 0, 8, None, None, 0, None)

    for call in (graph, scenes):
        assert call(_params(output_feat=65)) == UNSUPPORTED
        assert call(_params(seq_len=9)) == UNSUPPORTED
        assert call(_params(n_stgcn=_lib.DMRGCN_MAX_STGCN + 1)) == UNSUPPORTED
        assert call(_params(input_feat=2)) == UNSUPPORTED
        p = _params()
        for b, val in enumerate((4.0, 2.0, 1.0, 0.5, 0.0)):  # descending
            p.split[1][b] = val
        assert call(p) == UNSUPPORTED
        p = _params()
        p.split[0][2] = p.split[0][1]  # a bin of no width
        assert call(p) == UNSUPPORTED
        p = _params()
        p.st_dmrgcns[0].gcn_w[1] = None
        assert call(p) == INVALID
        p = _params()
        p.tpcnns[3].gta_b = None
        assert call(p) == INVALID
        p = _params()
        p.tpcnns[0].res_w = None  # K != k in the first block: the residual is a convolution
        assert call(p) == INVALID
    # N = 0 is nothing to do; a missing input is refused
    assert lib.et_dmrgcn_forward_graph(None, 8, 8, 3, 8, None, 0, None) == INVALID
    assert lib.et_dmrgcn_forward_graph(C.byref(_params()), None, None, 0, None, None, 0, None) == 0
    assert lib.et_dmrgcn_forward_graph(C.byref(_params()), None, 8, 3, 8, None, 0, None) == INVALID
    assert lib.et_dmrgcn_forward_scenes(C.byref(_params()), None, 8, 3, None, 0, 8, None, None, 0, None) == INVALID
    # workspace: none while the largest scene fits the LDS arena (S = 20, k = 6: 576 floats per pedestrian, 26 pedestrians)
    ws = lambda p, n, mx: int(lib.et_dmrgcn_workspace_bytes(C.byref(p), n, mx))
    assert ws(_params(), 5000, 26) == 0 and ws(_params(), 5000, 27) == 5000 * 576 * 4
    assert ws(_params(output_feat=65), 5000, 100) == 0  # outside the family: not taken
    assert ws(_params(n_stgcn=2), 100, 100) == 100 * (12 * 8 + 3 * 210) * 4  # C_in = S: 10 (S + 1) contracted rows


def test_dmrgcn_abi_names_declared_and_mirrored():
    from eigentrajectory_amd import _lib
    header = H.text()
    for name in ("et_dmrgcn_workspace_bytes", "et_dmrgcn_forward_graph", "et_dmrgcn_forward_scenes"):
        assert re.search(rf"\b{name}\(", header) and name in _lib.SYMBOLS, name
    for struct, mirror in (("et_dmrgcn_layer", _lib.DMRGCNLayer), ("et_dmrgcn_tpcnn", _lib.DMRGCNTpcnn),
                           ("et_dmrgcn_params", _lib.DMRGCNParams)):
        assert H.struct_fields(struct) == [f for f, _ in mirror._fields_], struct
    d = H.defines()
    assert (d["ET_DMRGCN_MAX_STGCN"], d["ET_DMRGCN_MAX_TPCNN"], d["ET_DMRGCN_BINS"]) == (
        _lib.DMRGCN_MAX_STGCN, _lib.DMRGCN_MAX_TPCNN, _lib.DMRGCN_BINS)
    assert d["ET_DMRGCN_MAX_STGCN"] >= 2 and d["ET_ABI_VERSION"] == 3
    assert C.sizeof(_lib.DMRGCNParams) == 7 * 4 + 10 * 4 + 4 + 4 * 10 * 8 + 8 * 11 * 8  # ints, split, padding, pointer tables


@pytest.mark.parametrize("scene", ["eth", "zara1", "zara2"])
def test_most_scenes_are_robust(scene):
    """the end-to-end GPU test compares pedestrian by pedestrian on the robust scenes only: they must be nearly all"""
    assert float(Z[f"{scene}.robust"].mean()) >= 0.95
