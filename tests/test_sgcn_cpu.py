"""CPU checks of the native SGCN predictor (eigentrajectory_amd/sgcn.py, csrc/et_sgcn.hip): the fp64 numpy restatement
(tests/_sgcn_np.py) against the reference's recorded outputs and logits (tests/golden/g20_sgcn_net.npz,
tools/make_golden_sgcn_net.py) across the network's hard threshold, the synthetic inputs of the GPU tests against the caps
on undecided entries, the module's state_dict against the reference's, and the refusals (training mode, dropout)."""
import os
import re

import numpy as np
import pytest
import torch

from . import _abi_header as H
from . import _golden as G
from . import _sgcn_np as SN

Z = G.load("g20_sgcn_net.npz")
PICKS = sorted({k.split(".")[0] for k in Z.files if k.startswith("pick")}, key=lambda t: int(t[4:]))
GEN_ARGS = dict(number_asymmetric_conv_layer=3, n_tcn=2, out_dims=12)


def net_state(prefix="net."):
    return {k[len(prefix):]: Z[k] for k in Z.files
            if k.startswith(prefix) and not k[len(prefix):].startswith(("net_out", "logit_", "pick"))}


def et_module(**kw):
    from eigentrajectory_amd.sgcn import SGCN
    args = dict(number_asymmetric_conv_layer=7, embedding_dims=64, number_gcn_layers=1, dropout=0, obs_len=8, pred_len=6,
                n_tcn=5, in_dims=1, out_dims=20)
    args.update(kw)
    return SGCN(**args)


def test_fixture_covers_the_cases_the_tests_need():
    sizes = {t: Z[f"{t}.v"].shape[2] for t in PICKS}
    for s in G.SCENES:  # the largest scene of every split
        assert any(str(Z[f"{t}.split"]) == s and sizes[t] == int(Z[f"{s}.scene_size"].max()) for t in PICKS), s
        assert Z[f"{s}.ade"].shape == Z[f"{s}.fde"].shape == (int(Z[f"{s}.scene_size"].sum()),)
        assert Z[f"{s}.min_abs_logit"].shape == Z[f"{s}.scene_size"].shape
    assert max(sizes.values()) == 57 and min(sizes.values()) <= 2
    mins = {t: float(Z[f"{str(Z[f'{t}.split'])}.min_abs_logit"][int(Z[f"{t}.index"])]) for t in PICKS}
    assert any(m < SN.DELTA for m in mins.values())  # a scene with an undecided entry
    for t in PICKS:  # the bridge's quirk: the temporal identity is (N, 1, 1) of ones, not eye(T)
        n = sizes[t]
        assert Z[f"{t}.identity_s"].shape == (1, n, n) and Z[f"{t}.identity_t"].shape == (n, 1, 1)
        assert np.array_equal(Z[f"{t}.identity_t"], np.ones((n, 1, 1), np.float32))
        assert min(float(np.abs(Z[f"{t}.logit_s"]).min()), float(np.abs(Z[f"{t}.logit_t"]).min())) == mins[t]
    slopes = [v for k, v in net_state().items() if v.shape == (1,)]
    assert len(slopes) == 24 and not any(np.allclose(v, 0.25) for v in slopes)  # no default PReLU slope left
    # the share of scenes without an undecided entry the end-to-end GPU test relies on
    for s in G.SCENES:
        decided = float((Z[f"{s}.min_abs_logit"] >= SN.DELTA).mean())
        assert decided >= (0.65 if s == "univ" else 0.90), (s, decided)


def test_numpy_restatement_reproduces_the_reference():
    """parts (a) to (c) with the reference's recorded fp32 logits and outputs in the implementation's place"""
    sd = net_state()
    und = total = 0
    for t in PICKS:
        fig = SN.check_against(sd, Z[f"{t}.v"][0, :, :, 0], Z[f"{t}.identity_s"], Z[f"{t}.identity_t"], Z[f"{t}.net_out"],
                               Z[f"{t}.logit_s"], Z[f"{t}.logit_t"])
        und, total = und + fig["undecided"], total + fig["entries"]
    assert und <= SN.CAP_SPLIT * total
    gen = net_state("gen.")
    assert SN.n_layers(gen) == (3, 2) and SN.n_layers(sd) == (7, 5)
    for i in range(2):
        t = str(Z[f"gen.pick{i}"])
        SN.check_against(gen, Z[f"{t}.v"][0, :, :, 0], Z[f"{t}.identity_s"], Z[f"{t}.identity_t"], Z[f"gen.net_out{i}"],
                         Z[f"gen.logit_s{i}"], Z[f"gen.logit_t{i}"])


def test_decide_overrides_only_inside_the_band():
    sd = net_state()
    t = PICKS[0]
    v, ids, idt = Z[f"{t}.v"][0, :, :, 0], Z[f"{t}.identity_s"], Z[f"{t}.identity_t"]
    own, ls, lt = SN.forward(sd, v, ids, idt)
    flipped = (~(SN.sigmoid(ls) > 0.5), ~(SN.sigmoid(lt) > 0.5))
    same, _, _ = SN.forward(sd, v, ids, idt, decide=(*flipped, 0.0))       # empty band: the given decisions are ignored
    assert np.array_equal(same, own)
    other, _, _ = SN.forward(sd, v, ids, idt, decide=(*flipped, 1e-2))     # a wide band: they are taken
    assert np.abs(other - own).max() > 1e-4 * np.abs(own).max()


def test_fp32_decisions_at_the_rounding_threshold():
    """sigmoid_fp32(l) > 0.5 holds exactly from the first l whose exp(-l) rounds to 1 - 2^-23 or less, that is from
    l = -log(1 - 1.5 * 2^-24) = 8.94e-8 on: 1 + (1 - 2^-24) rounds (to even) to 2 and 1 / 2 is not above 0.5, while
    1 / (2 - 2^-23) rounds up to 0.5 + 2^-24.  No negative logit and no zero is kept; away from the threshold the
    decision is the sign"""
    edge = -np.log1p(-1.5 * 2.0 ** -24)
    assert abs(edge - 8.9407e-8) < 1e-12
    l = np.linspace(-4e-7, 4e-7, 800001).astype(np.float32)
    keep = SN.decisions_fp32(l)
    assert np.array_equal(keep, l.astype(np.float64) > edge)
    wide = np.random.default_rng(0).normal(0, 3, 200000).astype(np.float32)
    assert np.array_equal(SN.decisions_fp32(wide), wide > 0)
    assert not SN.decisions_fp32(np.float32([0.0, -0.0, -1e-30, 1e-30, -np.inf])).any() and SN.decisions_fp32(np.float32([np.inf]))[0]


def test_synthetic_scenes_stay_within_the_caps():
    """the ragged scenes of the GPU test: each within the per-scene cap, all of them together within the per-split one"""
    sd = net_state()
    und_all = total_all = 0
    for n in SN.RAGGED:
        ids, idt = SN.bridge_identities(8, n)
        _, ls, lt = SN.forward(sd, SN.synthetic_v(n), ids, idt)
        und, total = SN.undecided(ls, lt)
        assert und <= SN.CAP_SCENE * total, (n, und, total)
        und_all, total_all = und_all + und, total_all + total
    assert und_all <= SN.CAP_SPLIT * total_all, (und_all, total_all)


def test_synthetic_split_stays_within_the_caps():
    sd = net_state()
    C_obs, nrm = SN.synthetic_split(SN.SPLIT_SIZES, SN.SPLIT_SEED)
    lo = und_all = total_all = 0
    for n in SN.SPLIT_SIZES:
        ids, idt = SN.bridge_identities(8, n)
        _, ls, lt = SN.forward(sd, SN.scene_input(C_obs, nrm, lo, lo + n), ids, idt)
        und, total = SN.undecided(ls, lt)
        assert und <= SN.CAP_SCENE * total, (n, und, total)
        und_all, total_all, lo = und_all + und, total_all + total, lo + n
    assert und_all <= SN.CAP_SPLIT * total_all, (und_all, total_all)


def test_state_dict_names_and_shapes_are_the_references():
    for prefix, kw in (("net.", {}), ("gen.", GEN_ARGS)):
        ref = net_state(prefix)
        net = et_module(**kw)
        mine = net.state_dict()
        assert sorted(mine) == sorted(ref)
        assert all(tuple(mine[k].shape) == ref[k].shape for k in ref)
        net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in ref.items()}, strict=True)
        assert torch.equal(net.output.bias, torch.from_numpy(ref["output.bias"]))
    sd = et_module().state_dict()
    assert "sparse_weighted_adjacency_matrices.spatial_attention.scaled_factor" not in sd
    assert et_module().sparse_weighted_adjacency_matrices.spatial_attention.scaled_factor == 8.0
    assert "sparse_weighted_adjacency_matrices.interaction_mask.temporal_asymmetric_convolutions.6.conv1.weight" in sd
    assert "sparse_weighted_adjacency_matrices.interaction_mask.spatial_asymmetric_convolutions.0.conv1.bias" not in sd
    assert "stsgcn.temporal_spatial_sparse_gcn.1.embedding.weight" in sd and "tcns.4.1.weight" in sd
    from eigentrajectory_amd import SGCN
    assert SGCN is type(et_module())
    SGCN()  # the reference's defaults construct (their forward is outside the native family)


def test_reference_checkpoint_loads():
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    g2 = G.load("g2_fit_all_scenes.npz")
    hp = default_hyper_params(static_dist=G.static_dist("eth"))
    model = EigenTrajectory(et_module(), get_hook_func("sgcn"), hp)
    ckpt = model.state_dict()
    for k, v in net_state().items():
        ckpt[f"baseline_model.{k}"] = torch.from_numpy(np.array(v))
    for k in ckpt:
        if k.startswith("ET_"):
            ckpt[k] = torch.from_numpy(g2[f"eth.{k}"])
    model.load_state_dict(ckpt, strict=True)  # a reference ET-SGCN checkpoint's keys, unchanged
    assert torch.equal(model.baseline_model.fusion_.weight, torch.from_numpy(Z["net.fusion_.weight"]))


def test_training_mode_and_dropout_raise():
    v, ident = torch.zeros((1, 8, 3, 1)), [torch.eye(3)[None], torch.ones((3, 1, 1))]
    net = et_module()
    assert net.training
    with pytest.raises(RuntimeError, match="training"):
        net(v, ident)
    with pytest.raises(RuntimeError, match="dropout"):
        et_module(dropout=0.1).eval()(v, ident)


def test_evaluate_split_refuses_other_predictors():
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    hp = default_hyper_params(static_dist=G.static_dist("eth"))
    obs, pred, sse = torch.zeros((3, 8, 2)), torch.zeros((3, 12, 2)), [[0, 3]]
    for predictor, hooks in ((torch.nn.Linear(2, 2), "sgcn"), (et_module(), "stgcnn"), (torch.nn.Linear(2, 2), "pecnet")):
        model = EigenTrajectory(predictor, get_hook_func(hooks), hp).eval()
        with pytest.raises(NotImplementedError, match="SocialSTGCNN.*SGCN"):
            model.evaluate_split(obs, pred, sse)


def test_sgcn_abi_names_declared_and_listed():
    from eigentrajectory_amd import _lib
    header = H.text()
    for name in ("et_sgcn_workspace_bytes", "et_sgcn_forward_scenes", "et_sgcn_forward_graph"):
        assert re.search(rf"\b{name}\(", header) and name in _lib.SYMBOLS, name
    for struct, mirror in (("et_sgcn_attention", _lib.SGCNAttention), ("et_sgcn_asym", _lib.SGCNAsym),
                           ("et_sgcn_gcn", _lib.SGCNGcn)):
        assert H.struct_fields(struct) == [f for f, _ in mirror._fields_], struct
    names = H.struct_fields("et_sgcn_params")
    assert names == [f for f, _ in _lib.SGCNParams._fields_]
    assert f"#define ET_SGCN_MAX_LAYERS {_lib.SGCN_MAX_LAYERS}" in header and f"#define ET_SGCN_MAX_N {_lib.SGCN_MAX_N}" in header
    if os.path.exists(_lib.LIB_PATH):
        p = _lib.SGCNParams()
        assert _lib.lib().et_sgcn_workspace_bytes(_lib.C.byref(p), _lib.i64(10), _lib.i64(100), 1) == 0  # not taken
        assert all(hasattr(_lib.lib(), name) for name in _lib.SYMBOLS if name.startswith("et_sgcn_"))


# ------------------------------------------------- the configurations of tests/test_gpu_sgcn_shapes.py (SN.CONFIGS)
_REF64 = {}


def ref64(name, layout):
    """the fp64 restatement on every non-empty scene of a layout, computed once: [(v, ids, idt, out, logit_s, logit_t)]"""
    if (name, layout) not in _REF64:
        sd = SN.random_state(name)
        rows = []
        for _, _, n, v in SN.scenes_of(*SN.layout_inputs(name, layout)):
            ids, idt = SN.bridge_identities(v.shape[0], n)
            rows.append((v, ids, idt, *SN.forward(sd, v, ids, idt)))
        _REF64[name, layout] = rows
    return _REF64[name, layout]


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


def test_configs_name_the_paths_and_the_layouts():
    c = SN.CONFIGS
    assert (c["k1"]["asym"], c["k1"]["tcn"], c["k1"]["k"], c["k1"]["S"]) == (1, 1, 1, 1)
    assert c["k2_wide"]["asym"] % 2 == 0 and c["k2_wide"]["S"] == 64
    assert (c["deep"]["asym"], c["deep"]["tcn"]) == (8, 8)
    assert 8 < c["k12"]["k"] + 2 < 34 and c["k12"]["S"] % 2 == 1
    assert c["kmax"]["k"] == 32
    assert (c["et"]["asym"], c["et"]["tcn"], c["et"]["k"], c["et"]["S"]) == (7, 5, 6, 20)
    assert SN.EDGE_SIZES == (1, 2, 3, 0, 63, 64, 65) and SN.BIG == (257,) and SN.LIMIT == (512,)
    assert len(SN.MANY) == 300 and set(SN.MANY) == {1, 2, 3} and SN.MANY[:4] == (1, 2, 3, 1)
    assert set(SN.USED) == set(c) and all("edge" in u and "g3" in u and "g65" in u for u in SN.USED.values())
    assert {n for n, u in SN.USED.items() if "big" in u} == {n for n, u in SN.USED.items() if "limit" in u} == {"k1", "k2_wide"}
    assert {n for n, u in SN.USED.items() if "many" in u} == {"k1", "et"}
    assert set(SN.SEEDS) == {(n, l) for n, u in SN.USED.items() for l in u}


@pytest.mark.parametrize("name", list(SN.CONFIGS))
def test_config_loads_strictly_and_leaves_no_default(name):
    from eigentrajectory_amd.sgcn import SGCN
    sd = SN.random_state(name)
    net = SGCN(**SN.module_cfg(name))
    assert list(net.state_dict()) == list(sd) == list(SN.state_shapes(name))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    c = SN.CONFIGS[name]
    assert SN.n_layers(sd) == (c["asym"], c["tcn"]) and (net.obs_len, net.pred_len, net.out_dims) == (c["k"] + 2, c["k"], c["S"])
    assert all(v.dtype == np.float32 for v in sd.values())
    slopes = [float(v[0]) for k, v in sd.items() if SN.is_slope(k)]
    assert all(sd[k].shape == (1,) for k in sd if SN.is_slope(k)) and len(slopes) == 5 + 2 * c["asym"] + c["tcn"]  # spa_fusion, 4 gcns and every layer's own
    assert len(set(slopes)) == len(slopes) and all(abs(a - 0.25) > 0.02 and a > 0.04 for a in slopes)
    assert all(np.abs(v).min() > 0 for k, v in sd.items() if k.endswith("bias"))
    f = sd["fusion_.weight"][:, :, 0, 0]
    assert np.abs(f - f.T).max() > 0.05
    for k in sd:
        if k.endswith("conv1.weight"):
            assert np.abs(sd[k][..., 0] - sd[k.replace("conv1", "conv2")][:, :, 0]).max() > 0.05
    for other in SN.CONFIGS:  # no two configurations share a draw
        if other != name:
            assert not np.array_equal(SN.random_state(other)["fusion_.weight"], sd["fusion_.weight"])
    assert all(np.array_equal(v, SN.random_state(name)[k]) for k, v in sd.items())  # seeded


@pytest.mark.parametrize("name", list(SN.CONFIGS))
def test_float32_mode_meets_the_weight_conditions(name):
    """the restatement in fp32 (dtype=np.float32: the same statements, the arithmetic's own error) against itself in fp64,
    on every scene of every layout the GPU test runs: logits within DELTA / 2; with the decisions fixed to the fp64 ones (an
    infinite band) the output within TOL / 4 of the largest entry"""
    sd = SN.random_state(name)
    for layout in SN.USED[name]:
        worst_l = worst_o = 0.0
        for v, ids, idt, out, ls, lt in ref64(name, layout):
            o32, ls32, lt32 = SN.forward(sd, v, ids, idt, decide=(SN.sigmoid(ls) > 0.5, SN.sigmoid(lt) > 0.5, np.inf),
                                         dtype=np.float32)
            assert o32.dtype == ls32.dtype == lt32.dtype == np.float32  # nothing promoted on the way
            worst_l = max(worst_l, float(np.abs(ls32 - ls).max()), float(np.abs(lt32 - lt).max()))
            worst_o = max(worst_o, rel(o32, out))
        print(f"sgcn {name} {layout}: float32-mode logit error {worst_l:.2e} (bound {SN.DELTA / 2:.1e}), output error "
              f"{worst_o:.2e} (bound {SN.TOL / 4:.1e})")
        assert worst_l <= SN.DELTA / 2, (name, layout, worst_l)
        assert worst_o <= SN.TOL / 4, (name, layout, worst_o)


@pytest.mark.parametrize("name", list(SN.CONFIGS))
def test_shape_layouts_stay_within_the_caps(name):
    """test_synthetic_scenes_stay_within_the_caps for every (configuration, layout, seed) of the shapes test: each scene
    within CAP_SCENE (a scene of one pedestrian at k = 1 has 48 entries: no undecided entry at all), each launch within
    CAP_SPLIT; no scene is left out"""
    for layout in SN.USED[name]:
        und_all = total_all = 0
        rows = ref64(name, layout)
        assert len(rows) == sum(1 for n in SN.LAYOUTS[layout] if n)
        for v, _, _, _, ls, lt in rows:
            und, total = SN.undecided(ls, lt)
            T_, n = v.shape
            assert total == 4 * T_ * n * n + 4 * n * T_ * T_
            assert und <= SN.CAP_SCENE * total, (name, layout, n, und, total)
            und_all, total_all = und_all + und, total_all + total
        print(f"sgcn {name} {layout}: undecided {und_all} of {total_all}")
        assert und_all <= SN.CAP_SPLIT * total_all, (name, layout, und_all, total_all)


def _without_last_asym(sd, na):
    return {k: v for k, v in sd.items() if f"asymmetric_convolutions.{na - 1}." not in k}


def _asym_reversed(sd, na):
    out = {}
    for k, v in sd.items():
        m = re.search(r"asymmetric_convolutions\.(\d+)\.", k)
        out[k if not m else k.replace(m.group(0), f"asymmetric_convolutions.{na - 1 - int(m.group(1))}.")] = v
    return out


@pytest.mark.parametrize("name", list(SN.CONFIGS))
def test_mutants_of_the_restatement_move_the_output(name):
    """six wrong forms of the network, each more than 1e-3 of the largest entry away from the right one on the scene of 3
    -- the seeded weights are not degenerate (a slope, a bias, an order or a shortcut does matter); where a form cannot be
    expressed (a reversed order of one layer, the residual of tcns[j >= 1] with one tcn) it is the identity"""
    sd = SN.random_state(name)
    c = SN.CONFIGS[name]
    (v, ids, idt, out, _, _), = ref64(name, "g3")
    T_, n = v.shape
    fus = dict(sd)
    fus["fusion_.weight"] = np.ascontiguousarray(sd["fusion_.weight"].transpose(1, 0, 2, 3))
    eye_t = np.broadcast_to(np.eye(T_, dtype=np.float32), (n, T_, T_))
    mutants = {
        "last asym layer skipped": (_without_last_asym(sd, c["asym"]), idt, ()),
        "asym layers reversed": (_asym_reversed(sd, c["asym"]), idt, ()),
        "no residual in tcns[j >= 1]": (sd, idt, ("no_tcn_residual",)),
        "fusion_ transposed": (fus, idt, ()),
        "spa_fusion without its shortcut": (sd, idt, ("no_fusion_shortcut",)),
        "temporal identity eye(T)": (sd, eye_t, ()),
    }
    assert SN.n_layers(mutants["last asym layer skipped"][0]) == (c["asym"] - 1, c["tcn"])
    identity = {"asym layers reversed": c["asym"] == 1, "no residual in tcns[j >= 1]": c["tcn"] == 1}
    for what, (msd, midt, variant) in mutants.items():
        got = SN.forward(msd, v, ids, midt, variant=variant)[0]
        moved = rel(got, out)
        print(f"sgcn {name} mutant '{what}': {moved:.2e}")
        if identity.get(what, False):
            assert np.array_equal(got, out), (name, what)
        else:
            assert moved > 1e-3, (name, what, moved)
