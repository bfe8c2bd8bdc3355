"""CPU checks of the native Social-Implicit predictor (eigentrajectory_amd/implicit.py, csrc/et_implicit.hip): the numpy
restatement (tests/_implicit_np.py) against the reference's recorded outputs (tests/golden/g25_implicit.npz,
tools/make_golden_implicit.py), the zone rule on the bin values and their fp32 neighbours, that the fixture tells the local
stream's raw reshape from a transpose, that an output column depends on its compacted neighbours -2 .. +2 only, the
module's state_dict against the reference's, what raises, the dispatch of evaluate_split and the entry points' argument
validation (host side, before any device work)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from . import _abi_header as H
from . import _golden as G
from . import _implicit_np as IN

Z = G.load("g25_implicit.npz")
PICKS = sorted({k.split(".")[0] for k in Z.files if k.startswith("pick")}, key=lambda t: int(t[4:]))
HAND = ["single", "edges", "lonely", "nan"]
GEN = dict(spatial_input=1, spatial_output=12, temporal_input=10, temporal_output=5, bins=[0, 0.5, 2],
           noise_weight=[0.05, 1, 4])
TOL = 1e-5  # of the largest entry, the project's bound for a fp32 result against fp64


def net_state(prefix="net."):
    return {k[len(prefix):]: Z[k] for k in Z.files if k.startswith(prefix + "implicit_cells.")}


def et_module(**kw):
    from eigentrajectory_amd.implicit import SocialImplicitLight
    args = dict(spatial_input=1, spatial_output=20, temporal_input=8, temporal_output=6, bins=[0, 0.01, 0.1, 1.2],
                noise_weight=[0.05, 1, 4, 8])
    args.update(kw)
    return SocialImplicitLight(**args)


def scale_err(got, ref):
    """largest difference over the largest entry, the NaNs in the same places"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    return float(np.nanmax(np.abs(got - ref)) / np.nanmax(np.abs(ref)))


def test_fixture_covers_the_cases_the_tests_need():
    sizes = [Z[f"{t}.v"].shape[-1] for t in PICKS]
    assert max(sizes) == max(int(Z[f"{s}.scene_size"].max()) for s in G.SCENES)  # the largest scene of all splits
    assert {str(Z[f"{t}.split"]) for t in PICKS} == set(G.SCENES)
    assert any(len(np.unique(Z[f"{t}.zone"])) >= 3 for t in PICKS)
    for s in G.SCENES:
        n = int(Z[f"{s}.scene_size"].sum())
        assert Z[f"{s}.ade"].shape == Z[f"{s}.fde"].shape == (n,) and Z[f"{s}.robust"].shape == Z[f"{s}.scene_size"].shape
    sd = net_state()
    scalars = [float(v[0]) for k, v in sd.items() if k.endswith(("global_w", "local_w", "noise_w"))]
    assert len(scalars) == 12 and len(set(scalars)) == 12 and 0.0 not in scalars  # zero weights would make every output 0
    assert all(np.abs(Z[f"{t}.net_out"]).max() > 1e-2 for t in PICKS + HAND[:3])
    assert Z["single.v"].shape == (1, 1, 8, 1) and Z["edges.v"].shape == (1, 1, 8, 16)
    first = Z["edges.v"][0, 0, 0]
    f32 = np.float32
    for b in (0.01, 0.1, 1.2):  # each bin value, both signs of it, and its fp32 neighbours either side
        for val in (f32(b), -f32(b), np.nextafter(f32(b), f32(0)), np.nextafter(f32(b), f32(9))):
            assert (first == val).any(), val
    assert (first == 0).sum() == 2 and np.signbit(first[first == 0]).tolist() == [False, True]
    z = Z["edges.zone"]
    assert all(z[i] != z[i + 1] for i in range(15)) and sorted(np.bincount(z).tolist()) == [4, 4, 4, 4]
    assert 1 in np.bincount(Z["lonely.zone"]).tolist()  # a zone with a single member
    nan_at = np.flatnonzero(np.isnan(Z["nan.v"][0, 0, 0]))
    assert len(nan_at) == 1 and int(Z["nan.zone"][nan_at[0]]) == 3  # bucketize leaves a NaN in the last zone
    cols = np.isnan(Z["nan.net_out"][0]).any(axis=(0, 1))
    # the NaN reaches its zone-mates within two compacted places, whole columns of them, and no one else
    same = np.flatnonzero(Z["nan.zone"] == 3).tolist()
    at = same.index(int(nan_at[0]))
    assert np.flatnonzero(cols).tolist() == same[max(0, at - 2):at + 3] and len(same) > len(np.flatnonzero(cols))
    assert np.isnan(Z["nan.net_out"][0][:, :, cols]).all()


def test_numpy_restatement_reproduces_the_reference():
    sd = net_state()
    worst = 0.0
    for t in PICKS + HAND:
        v = Z[f"{t}.v"][0, 0]
        raw = IN.forward(sd, v)
        errs = (scale_err(raw, Z[f"{t}.net_out"][0]), scale_err(IN.c_pred_refine(raw), Z[f"{t}.c_pred_refine"]))
        worst = max(worst, *errs)
        assert max(errs) <= TOL, (t, errs)
    gen = net_state("gen.")
    for i in range(2):
        err = scale_err(IN.forward(gen, Z[f"gen.v{i}"][0, 0], bins=GEN["bins"]), Z[f"gen.net_out{i}"][0])
        worst = max(worst, err)
        assert err <= TOL, (i, err)
    print(f"restatement against the reference: {worst:.2e} of the largest entry")


def test_zones_are_fp32_comparisons():
    for t in PICKS + HAND:
        assert np.array_equal(IN.zones(Z[f"{t}.v"][0, 0]), Z[f"{t}.zone"]), t
    f32 = np.float32
    row = np.asarray([[0.0, -0.0, 0.01, np.nextafter(f32(0.01), f32(0)), -0.01, 0.1, 1.2, np.nextafter(f32(1.2), f32(0)), 7,
                       np.nan]], np.float32)
    assert IN.zones(row).tolist() == [0, 0, 1, 0, 1, 2, 3, 2, 3, 3]  # a value equal to a bin is in the bin's own zone
    assert IN.zones(row, [0.5, 2]).tolist() == [-1, -1, -1, -1, -1, -1, 0, 0, 1, 1]  # below bins[0]: no zone
    # (the bins are fp32 values: 0.1f lies above 0.1, and it is 0.1f that the first coefficient is compared with)
    assert float(f32(0.1)) > 0.1 and IN.zones(np.asarray([[0.1]], np.float32))[0] == 2


def test_a_transpose_in_place_of_the_raw_reshape_misses_the_bound():
    """the local stream's (T_out, S) block is reinterpreted as (S, T_out) (model.py:40); S = 20 != T_out = 6 scrambles it"""
    sd = net_state()
    for t in ["edges", PICKS[0]]:
        v = Z[f"{t}.v"][0, 0]
        assert scale_err(IN.forward(sd, v, transpose=True), Z[f"{t}.net_out"][0]) > 100 * TOL
        assert scale_err(IN.forward(sd, v), Z[f"{t}.net_out"][0]) <= TOL
    gen = net_state("gen.")
    assert scale_err(IN.forward(gen, Z["gen.v0"][0, 0], bins=GEN["bins"], transpose=True), Z["gen.net_out0"][0]) > 100 * TOL


def test_a_column_depends_on_its_compacted_neighbours_only():
    """what the kernel's neighbour table rests on: the scene cut down to a pedestrian's two predecessors and two
    successors of its own zone gives the same column; a pedestrian alone in its zone differs from the same pedestrian
    between two zone-mates whose other rows are zero (u of a zero column is relu(bias) + bias, not the padding's 0)"""
    sd = net_state()
    for t in ["edges", "lonely", PICKS[2]]:
        v = Z[f"{t}.v"][0, 0]
        z, whole = IN.zones(v), IN.forward(sd, v)
        for w in range(v.shape[1]):
            same = np.flatnonzero(z == z[w]).tolist()
            at = same.index(w)
            keep = same[max(0, at - 2):at + 3]
            got = IN.forward(sd, v[:, keep])[:, :, keep.index(w)]
            assert np.abs(got - whole[:, :, w]).max() <= 1e-12 * np.abs(whole).max(), (t, w)
    v = Z["lonely.v"][0, 0]
    w = int(np.flatnonzero(Z["lonely.zone"] == 1)[0])
    padded = np.concatenate([np.zeros((8, 1), np.float32), v[:, [w]], np.zeros((8, 1), np.float32)], axis=1)
    padded[0, [0, 2]] = 0.05  # the same zone, otherwise zero columns
    alone, between = IN.forward(sd, v[:, [w]])[:, :, 0], IN.forward(sd, padded)[:, :, 1]
    assert np.abs(alone - between).max() > 1e-3 * np.abs(alone).max()
    assert scale_err(IN.forward(sd, v)[:, :, w], alone) <= 1e-12


def test_state_dict_names_and_shapes_are_the_references():
    for prefix, kw in (("net.", {}), ("gen.", GEN)):
        ref = net_state(prefix)
        net = et_module(**kw)
        mine = net.state_dict()
        assert sorted(mine) == sorted(ref)
        assert all(tuple(mine[k].shape) == ref[k].shape for k in ref)
        net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in ref.items()}, strict=True)
        assert torch.equal(net.implicit_cells[1].ped.tpcnn.bias, torch.from_numpy(ref["implicit_cells.1.ped.tpcnn.bias"]))
        assert torch.equal(net.implicit_cells[2].local_w, torch.from_numpy(ref["implicit_cells.2.local_w"]))
    net = et_module()
    sd = net.state_dict()
    for name in ("feat", "highway_input", "highway", "tpcnn"):
        for kind in ("weight", "bias"):
            assert f"implicit_cells.3.{name}.{kind}" in sd and f"implicit_cells.0.ped.{name}.{kind}" in sd
    assert all(f"implicit_cells.2.{s}" in sd for s in ("noise_w", "global_w", "local_w")) and len(sd) == 4 * 19
    assert not any("bins" in k or "noise_weight" in k for k in sd)  # plain attributes
    assert net.bins == [0, 0.01, 0.1, 1.2] and net.noise_weight == [0.05, 1, 4, 8]
    assert float(net.implicit_cells[0].global_w.detach()) == 0.0  # the reference's initial value
    assert sum(v.size for v in net_state().values()) == 4 * 1059


def test_reference_checkpoint_loads_into_the_wrapper():
    from eigentrajectory_amd import EigenTrajectory, SocialImplicitLight
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    assert SocialImplicitLight is type(et_module())
    g2 = G.load("g2_fit_all_scenes.npz")
    hp = default_hyper_params(static_dist=G.static_dist("eth"))
    model = EigenTrajectory(et_module(), get_hook_func("implicit"), hp)
    ckpt = model.state_dict()
    for k, v in net_state().items():
        ckpt[f"baseline_model.{k}"] = torch.from_numpy(np.array(v))
    for k in ckpt:
        if k.startswith("ET_"):
            ckpt[k] = torch.from_numpy(g2[f"eth.{k}"])
    model.load_state_dict(ckpt, strict=True)  # a reference ET-Implicit checkpoint's keys, unchanged
    assert torch.equal(model.baseline_model.implicit_cells[3].global_w, torch.from_numpy(Z["net.implicit_cells.3.global_w"]))


def test_constructor_errors_and_training_mode():
    with pytest.raises(ValueError, match="bins"):
        et_module(bins=[])
    with pytest.raises(ValueError, match="noise"):
        et_module(noise_weight=[0.05, 1])
    with pytest.raises(ValueError, match="positive"):
        et_module(temporal_output=0)
    assert len(et_module(bins=[0, 1], noise_weight=[1, 2, 3]).implicit_cells) == 2
    et_module(spatial_output=65), et_module(spatial_input=2)  # outside the kernel's family: they construct
    net = et_module()
    assert net.training
    with pytest.raises(RuntimeError, match="training"):
        net(torch.zeros((1, 1, 8, 3)))


def test_evaluate_split_dispatch():
    """the implicit pairing gets past the dispatch (and stops at the missing device); under other hooks it does not"""
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd._lib import ETLibraryError
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    obs, pred = torch.zeros(3, 8, 2), torch.zeros(3, 12, 2)
    model = EigenTrajectory(et_module(), get_hook_func("implicit"), default_hyper_params(static_dist=0.3)).eval()
    if not torch.cuda.is_available():
        with pytest.raises((ETLibraryError, RuntimeError, ValueError)) as exc:
            model.evaluate_split(obs, pred, [[0, 3]])
        assert not isinstance(exc.value, NotImplementedError)
    model.train()
    with pytest.raises(RuntimeError, match="training mode"):
        model.evaluate_split(obs, pred, [[0, 3]])
    for predictor, hooks in ((et_module(), "stgcnn"), (et_module(), "dmrgcn"), (torch.nn.Linear(2, 2), "implicit")):
        model = EigenTrajectory(predictor, get_hook_func(hooks), default_hyper_params(static_dist=0.3)).eval()
        with pytest.raises(NotImplementedError, match="SocialImplicitLight.*'implicit'"):
            model.evaluate_split(obs, pred, [[0, 3]])


def _params(**kw):
    """et_implicit_params of the ET configuration whose every pointer is a (never dereferenced) non-NULL host address"""
    from eigentrajectory_amd import _lib
    p = _lib.ImplicitParams()
    p.spatial_input, p.spatial_output, p.temporal_input, p.temporal_output, p.n_bins = 1, 20, 8, 6, 4
    for b, val in enumerate(IN.BINS):
        p.bins[b] = val
    dummy = C.addressof(C.c_float(0.0)) or 8
    for i in range(_lib.IMPLICIT_MAX_BINS):
        c = p.cells[i]
        for j in range(8):
            c.global_t[j] = c.local_t[j] = dummy
        c.noise_w = c.global_w = c.local_w = dummy
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_arguments_are_validated_on_the_host():
    """Every refusal below is answered before a launch: the calls run without a device."""
    from eigentrajectory_amd import _lib
    lib = _lib.lib()
    UNSUPPORTED, INVALID, WORKSPACE = (H.defines()[k] for k in ("ET_ERR_UNSUPPORTED", "ET_ERR_INVALID_ARG",
                                                                "ET_ERR_WORKSPACE"))

    def graph(p):
        return lib.et_implicit_forward_graph(C.byref(p), 8, 3, 8, 8, 1 << 20, None)

    def scenes(p):
        return lib.et_implicit_forward_scenes(C.byref(p), 8, 8, 3, None, 0, 8, None, None, 8, 1 << 20, None)

    for call in (graph, scenes):
        assert call(_params(spatial_output=65)) == UNSUPPORTED
        assert call(_params(temporal_input=17)) == UNSUPPORTED
        assert call(_params(temporal_output=17)) == UNSUPPORTED
        assert call(_params(spatial_input=2)) == UNSUPPORTED
        assert call(_params(n_bins=0)) == UNSUPPORTED and call(_params(n_bins=9)) == UNSUPPORTED
        p = _params()
        for b, val in enumerate((1.2, 0.1, 0.01, 0.0)):  # descending
            p.bins[b] = val
        assert call(p) == UNSUPPORTED
        p = _params()
        p.bins[2] = float("nan")
        assert call(p) == UNSUPPORTED
        p = _params()
        p.cells[3].local_t[6] = None
        assert call(p) == INVALID
        p = _params()
        p.cells[0].global_w = None
        assert call(p) == INVALID
    assert scenes(_params(temporal_input=2)) == UNSUPPORTED  # v = [C_obs; obs_ori] has no coefficient row
    # N = 0 is nothing to do; a missing input and a missing or short workspace are refused
    assert lib.et_implicit_forward_graph(None, 8, 3, 8, 8, 1 << 20, None) == INVALID
    assert lib.et_implicit_forward_graph(C.byref(_params()), None, 0, None, None, 0, None) == 0
    assert lib.et_implicit_forward_graph(C.byref(_params()), None, 3, 8, 8, 1 << 20, None) == INVALID
    assert lib.et_implicit_forward_graph(C.byref(_params()), 8, 3, 8, None, 0, None) == WORKSPACE
    assert lib.et_implicit_forward_graph(C.byref(_params()), 8, _lib.SCENE_MAX_N + 1, 8, 8, 1 << 30, None) == INVALID
    assert lib.et_implicit_forward_scenes(C.byref(_params()), None, 8, 3, None, 0, 8, None, None, 8, 1 << 20, None) == INVALID
    assert lib.et_implicit_forward_scenes(C.byref(_params()), 8, 8, 3, None, 0, 8, None, None, 8, 3 * 64 - 1, None) == WORKSPACE
    assert lib.et_implicit_forward_scenes(C.byref(_params()), 8, 8, 0, 8, 0, 8, None, None, None, 0, None) == 0
    assert lib.et_implicit_forward_scenes(C.byref(_params()), 8, 8, 3, 8, 0, 8, None, None, 8, 1 << 20, None) == INVALID
    # workspace: per pedestrian the neighbour row (8 int32) and the scene's v (T floats)
    ws = lambda p, n: int(lib.et_implicit_workspace_bytes(C.byref(p), n))
    assert ws(_params(), 5000) == 5000 * (8 + 8) * 4 and ws(_params(), 0) == 0
    assert ws(_params(spatial_output=65), 5000) == 0  # outside the family: not taken


def test_implicit_abi_names_declared_and_mirrored():
    from eigentrajectory_amd import _lib
    header = H.text()
    for name in ("et_implicit_workspace_bytes", "et_implicit_forward_graph", "et_implicit_forward_scenes"):
        assert re.search(rf"\b{name}\(", header) and name in _lib.SYMBOLS, name
    for struct, mirror in (("et_implicit_cell", _lib.ImplicitCell), ("et_implicit_params", _lib.ImplicitParams)):
        assert H.struct_fields(struct) == [f for f, _ in mirror._fields_], struct
    d = H.defines()
    assert d["ET_IMPLICIT_MAX_BINS"] == _lib.IMPLICIT_MAX_BINS == 8 and d["ET_ABI_VERSION"] == 3
    assert C.sizeof(_lib.ImplicitCell) == 19 * 8
    assert C.sizeof(_lib.ImplicitParams) == 5 * 4 + 8 * 4 + 4 + 8 * 19 * 8  # ints, bins, padding, the cells' pointer tables


@pytest.mark.parametrize("scene", G.SCENES)
def test_most_scenes_are_robust(scene):
    """the end-to-end GPU test compares pedestrian by pedestrian on the robust scenes only: they must be nearly all"""
    assert float(Z[f"{scene}.robust"].mean()) >= 0.95
