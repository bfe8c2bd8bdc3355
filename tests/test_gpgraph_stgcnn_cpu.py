"""CPU checks of the native GP-Graph-STGCNN predictor (eigentrajectory_amd/gpgraph.py, csrc/et_gpgraph_stgcnn.hip): the
fp64 numpy restatement (tests/_gpgraph_stgcnn_np.py) against the reference's recorded distances, group indices, pass inputs
and outputs (tests/golden/g22_gpgraph_stgcnn_net.npz, tools/make_golden_gpgraph_stgcnn.py), the fp32 bounds on the inputs of
passes 1 and 2 on the reference's own values, the module's state_dict against the reference's, the refusals, and the ABI's
names; and, across the family (tests/_gpgraph_stgcnn_np.py: CONFIGS), the conditions on the seeded inputs of
tests/test_gpu_gpgraph_stgcnn_shapes.py: the restated arena and workspace figures, no undecided pair, 1 < G < n, merges that
are not the connected components, the restatement's own fp32 error, weights that show a wrong statement, and fixture G34
(tests/golden/g34_gpgraph_stgcnn_family.npz) reproduced."""
import os
import re

import numpy as np
import pytest
import torch

from . import _abi_header as H
from . import _golden as G
from . import _gpgraph_np as GN
from . import _gpgraph_stgcnn_np as GS

Z = G.load("g22_gpgraph_stgcnn_net.npz")
PICKS = sorted({k.split(".")[0] for k in Z.files if k.startswith("pick")}, key=lambda t: int(t[4:]))
_GEN_RESULTS = re.compile(r"^(pick|out|indices|v_intra|v_group|cond)\d")
HAND = {"pair": [0, 0], "chain": [0, 0, 1], "triangle": [0, 0, 0], "four": [0, 1, 0, 1], "twins": [0, 0, 1]}


def net_state(prefix="net."):
    return {k[len(prefix):]: Z[k] for k in Z.files if k.startswith(prefix) and not _GEN_RESULTS.match(k[len(prefix):])}


def et_module(**kw):
    from eigentrajectory_amd.gpgraph import GPGraphSTGCNN
    args = dict(obs_len=8, pred_len=6, in_dims=1, out_dims=20)
    args.update(kw)
    return GPGraphSTGCNN(**args)


def gen_module():
    from eigentrajectory_amd.gpgraph import GPGraph
    from eigentrajectory_amd.stgcnn import SocialSTGCNN
    base = SocialSTGCNN(n_stgcnn=2, n_txpcnn=3, input_feat=1, output_feat=12, seq_len=8, pred_seq_len=6, kernel_size=3,
                        graph_per_time_row=True)
    return GPGraph(base, in_channels=1, out_channels=12, obs_seq_len=8, pred_seq_len=6)


def direct_picks():
    """the picks whose recorded output can be compared with directly: well conditioned and with robust ties only"""
    return [t for t in PICKS if float(Z[f"{t}.cond"]) <= GS.COND and bool(Z[f"{t}.ties_robust"])]


def test_fixture_covers_the_cases_the_tests_need():
    sizes = {t: Z[f"{t}.v"].shape[-1] for t in PICKS}
    g19 = G.load("g19_stgcnn.npz")
    assert np.array_equal(Z["eth.scene_size"], g19["eth.scene_size"])
    n = int(Z["eth.scene_size"].sum())
    assert Z["eth.ade"].shape == Z["eth.fde"].shape == (n,)
    for key in ("margin", "cond", "ties_robust", "n_groups"):
        assert Z[f"eth.{key}"].shape == Z["eth.scene_size"].shape
    good = (Z["eth.margin"] > GN.BAND_D) & Z["eth.ties_robust"] & (Z["eth.cond"] <= GS.COND)
    assert good.mean() >= 0.9
    for s in G.SCENES:
        assert any(str(Z[f"{t}.split"]) == s for t in PICKS), s
    assert max(sizes.values()) == 57 and min(sizes.values()) <= 2
    hand = {str(Z[f"{t}.name"]): Z[f"{t}.indices"].tolist() for t in PICKS if str(Z[f"{t}.split"]) == "hand"}
    assert hand == HAND
    th = GN.threshold(net_state())
    assert th != 1.0 and float(Z["th_margin"]) > 10 * GN.BAND_D
    must = [t for t in PICKS if str(Z[f"{t}.split"]) == "hand" or sizes[t] <= 2]
    assert len(must) == 6 and set(must) <= set(direct_picks())
    for t in PICKS:
        n, g = sizes[t], int(Z[f"{t}.indices"].max()) + 1
        assert Z[f"{t}.v"].shape == (8, n) and Z[f"{t}.v_intra"].shape == (8, n) and Z[f"{t}.v_group"].shape == (8, g)
        assert Z[f"{t}.out"].shape == Z[f"{t}.out0"].shape == Z[f"{t}.out2"].shape == (1, 20, 6, n)
        assert Z[f"{t}.out1"].shape == (1, 20, 6, g)
        assert GN.pair_margin(Z[f"{t}.dist"].astype(np.float64), th) > GN.BAND_D
    twins = next(t for t in PICKS if str(Z[f"{t}.split"]) == "hand" and str(Z[f"{t}.name"]) == "twins")
    assert np.array_equal(Z[f"{twins}.v"][:, 0], Z[f"{twins}.v"][:, 1])
    assert np.array_equal(Z[f"{twins}.v_intra"][:, 0], Z[f"{twins}.v_intra"][:, 1])  # the whole-column tie survives v'
    assert any(int(Z[f"{t}.indices"].max()) + 1 < sizes[t] for t in PICKS)


@pytest.mark.parametrize("t", PICKS)
def test_restatement_reproduces_the_reference(t):
    """fed the reference's recorded v' and group means, the restatement gives its three passes and its output within 1e-5
    of the largest entry (expected: ~3e-7); its own distances and indices are the recorded ones"""
    sd = net_state()
    v = Z[f"{t}.v"]
    res = GS.forward(sd, v, inputs=(Z[f"{t}.v_group"], Z[f"{t}.v_intra"]), indices=Z[f"{t}.indices"])
    assert GS.rel_err(Z[f"{t}.dist"], res["dist"]) <= GS.TOL_D
    assert np.array_equal(GS.forward(sd, v)["indices"], Z[f"{t}.indices"])
    errs = [GS.rel_err(Z[f"{t}.out{m}"][0], res["outs"][m]) for m in range(3)] + [GS.rel_err(Z[f"{t}.out"][0], res["out"])]
    print(t, v.shape, errs)
    assert max(errs) <= GS.TOL, errs


def test_restatement_reproduces_the_generic_loop_counts():
    sd = net_state("gen.")
    assert GS.n_layers(GN.split_state(sd)[0]) == (2, 3)
    for i in range(2):
        t = str(Z[f"gen.pick{i}"])
        res = GS.forward(sd, Z[f"{t}.v"], inputs=(Z[f"gen.v_group{i}"], Z[f"gen.v_intra{i}"]), indices=Z[f"gen.indices{i}"])
        assert res["out"].shape == (12, 6, Z[f"{t}.v"].shape[1])
        assert GS.rel_err(Z[f"gen.out{i}"][0], res["out"]) <= GS.TOL


@pytest.mark.parametrize("t", PICKS)
def test_input_bounds_hold_for_the_references_own_values(t):
    r1, r2 = GS.check_inputs(Z[f"{t}.v"], Z[f"{t}.v_intra"], Z[f"{t}.v_group"], Z[f"{t}.indices"])
    print(t, r1, r2)
    assert r1 <= 1.0 and r2 <= 1.0, (r1, r2)


def test_masked_laplacian_and_ties():
    from . import _stgcnn_np as ST
    u = np.array([0.0, 1.0, 3.0, 3.0])
    assert np.array_equal(GS.laplacian_row(u), ST.laplacian_row(u))
    same = np.array([[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 1, 1], [0, 0, 1, 1]], bool)
    L = GS.laplacian_row(u, same)
    assert np.allclose(L[:2, :2], [[0.5, -0.5], [-0.5, 0.5]]) and np.all(L[:2, 2:] == 0)   # the mask enters the degree
    assert np.all(L[2:, 2:] == 0)                                                           # a tie: a_inv = 0, L = I - I
    assert np.all(GS.laplacian_row(u, np.eye(4, dtype=bool)) == 0)
    x = np.array([[0.0, 0.0, 1.0], [2.0, 2.0, 5.0]], np.float32)
    assert GS.ties(x).sum() == 4
    assert GS.ties_robust(x, x[:, :1], x)                       # columns 0 and 1 are identical as a whole
    y = np.array([[0.0, 0.0, 1.0], [2.0, 2.0, 5.0], [1.0, 4.0, 7.0]], np.float32)
    assert not GS.ties_robust(y, y[:, :1], y)                   # a non-zero tie between different columns
    z = np.array([[0.0, 0.0, 1.0], [2.0, 3.0, 5.0]], np.float32)
    assert GS.ties_robust(z, z[:, :1], z)                       # a tie at zero


def test_state_dict_names_and_shapes_are_the_references():
    for ref, net in ((net_state(), et_module()), (net_state("gen."), gen_module())):
        mine = net.state_dict()
        assert sorted(mine) == sorted(ref)
        assert all(tuple(mine[k].shape) == ref[k].shape for k in ref)
        net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in ref.items()}, strict=True)
        assert torch.equal(net.group_gen.th.detach(), torch.from_numpy(ref["group_gen.th"]))
    sd = et_module().state_dict()
    assert tuple(sd["baseline_model.st_gcns.0.gcn.conv.weight"].shape) == (20, 1, 1, 1)  # S channels, not S K
    assert tuple(sd["group_mix.st_gcns_mix.1.weight"].shape) == (120, 360, 1, 1)
    from eigentrajectory_amd import GPGraphSTGCNN, get_GPGraph_STGCNN_model
    assert type(get_GPGraph_STGCNN_model(obs_len=8, pred_len=6, in_dims=1, out_dims=20)) is GPGraphSTGCNN
    get_GPGraph_STGCNN_model()  # the reference's defaults construct


def test_stgcnn_without_the_new_keyword_is_unchanged():
    from eigentrajectory_amd.stgcnn import SocialSTGCNN
    g19 = G.load("g19_stgcnn.npz")
    ref = {k[4:]: g19[k] for k in g19.files if k.startswith("net.")}
    args = dict(n_stgcnn=1, n_txpcnn=5, input_feat=1, output_feat=20, seq_len=8, pred_seq_len=6, kernel_size=3)
    plain = SocialSTGCNN(**args)
    assert plain.graph_per_time_row is False
    assert sorted(plain.state_dict()) == sorted(ref)
    assert all(tuple(v.shape) == ref[k].shape for k, v in plain.state_dict().items())
    rows = SocialSTGCNN(graph_per_time_row=True, **args)
    changed = [k for k, v in rows.state_dict().items() if tuple(v.shape) != ref[k].shape]
    assert changed == ["st_gcns.0.gcn.conv.weight", "st_gcns.0.gcn.conv.bias"]


def test_reference_checkpoint_loads():
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    g2 = G.load("g2_fit_all_scenes.npz")
    hp = default_hyper_params(static_dist=G.static_dist("eth"))
    model = EigenTrajectory(et_module(), get_hook_func("gpgraphstgcnn"), hp)
    ckpt = model.state_dict()
    for k, v in net_state().items():
        assert f"baseline_model.{k}" in ckpt, k
        ckpt[f"baseline_model.{k}"] = torch.from_numpy(np.array(v))
    for k in ckpt:
        if k.startswith("ET_"):
            ckpt[k] = torch.from_numpy(g2[f"eth.{k}"])
    model.load_state_dict(ckpt, strict=True)  # a reference ET-GPGraph-STGCNN checkpoint's keys, unchanged
    assert torch.equal(model.baseline_model.group_gen.th.detach(), torch.from_numpy(Z["net.group_gen.th"]))
    assert any(k.startswith("baseline_model.baseline_model.st_gcns.") for k in ckpt)


def test_training_mode_and_unsupported_variants_raise():
    from eigentrajectory_amd.gpgraph import GPGraph
    from eigentrajectory_amd.stgcnn import SocialSTGCNN
    v = torch.zeros((1, 1, 8, 3))
    net = et_module()
    assert net.training
    with pytest.raises(RuntimeError, match="training"):
        net(v, v)
    net.eval().baseline_model.train()  # the wrapper in eval mode, its base put back into training mode
    with pytest.raises(RuntimeError, match="training"):
        net(v, v)

    def base(**kw):
        args = dict(n_stgcnn=1, n_txpcnn=5, input_feat=1, output_feat=20, seq_len=8, pred_seq_len=6, kernel_size=3,
                    graph_per_time_row=True)
        args.update(kw)
        return SocialSTGCNN(**args)

    for kw in (dict(d_type="learned"), dict(d_type="euclidean"), dict(d_type="estimate_th"), dict(d_th=1.0),
               dict(mix_type="mean"), dict(mix_type="cnn"), dict(group_type=(True, False, True)), dict(weight_share=False)):
        bad = GPGraph(base(), in_channels=1, out_channels=20, obs_seq_len=8, pred_seq_len=6, **kw).eval()
        with pytest.raises(NotImplementedError, match="ET configuration"):
            bad(v, v)
    with pytest.raises(NotImplementedError, match="ET configuration"):  # ET-STGCNN's gcn is not GP-Graph's base
        GPGraph(base(graph_per_time_row=False), in_channels=1, out_channels=20, obs_seq_len=8, pred_seq_len=6).eval()(v, v)
    with pytest.raises(NotImplementedError, match="GPGraphSTGCNN"):     # the per-time-row base on its own
        base().eval()(v, torch.zeros((8, 3, 3)))


def test_evaluate_split_refuses_wrong_pairings():
    from eigentrajectory_amd import EigenTrajectory, GPGraphSGCN
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    hp = default_hyper_params(static_dist=G.static_dist("eth"))
    obs, pred, sse = torch.zeros((3, 8, 2)), torch.zeros((3, 12, 2)), [[0, 3]]
    sgcn_based = GPGraphSGCN(obs_len=8, pred_len=6, in_dims=1, out_dims=20)
    for predictor, hooks in ((et_module(), "gpgraphsgcn"), (sgcn_based, "gpgraphstgcnn"), (et_module(), "stgcnn")):
        model = EigenTrajectory(predictor, get_hook_func(hooks), hp).eval()
        with pytest.raises(NotImplementedError, match="SocialSTGCNN.*SGCN.*GPGraph"):
            model.evaluate_split(obs, pred, sse)


def test_gpgraph_stgcnn_abi_names_declared_and_listed():
    from eigentrajectory_amd import _lib
    header = H.text()
    names = ("et_gpgraph_stgcnn_workspace_bytes", "et_gpgraph_stgcnn_forward_graph", "et_gpgraph_stgcnn_forward_scenes")
    for name in names:
        assert re.search(rf"\b{name}\(", header) and name in _lib.SYMBOLS, name
    assert H.struct_fields("et_gpgraph_stgcnn_params") == [f for f, _ in _lib.GPGraphSTGCNNParams._fields_]
    assert _lib.GPGraphSTGCNNParams._fields_[0] == ("base", _lib.STGCNNParams)
    assert list(_lib.SYMBOLS) == list(H.functions())
    if os.path.exists(_lib.LIB_PATH):
        p = _lib.GPGraphSTGCNNParams()
        assert _lib.lib().et_gpgraph_stgcnn_workspace_bytes(_lib.C.byref(p), _lib.i64(10), _lib.i64(100), 1) == 0  # not taken
        assert all(hasattr(_lib.lib(), name) for name in names)
        # a base outside the STGCNN family: status 3, before any pointer is looked at
        assert _lib.lib().et_gpgraph_stgcnn_forward_graph(_lib.C.byref(p), None, None, _lib.i64(3), None, None, None, None,
                                                          None, 0, None) == 3


# ------------------------------------------------------------------------------------------------- across the family
# The conditions that keep tests/test_gpu_gpgraph_stgcnn_shapes.py from hiding behind its inputs, on the restatement alone.
Z34 = G.load("g34_gpgraph_stgcnn_family.npz")
_CASES = {}


def family_cases():
    """every scene the GPU file compares -> {tag: (name, v_abs, v_rel, th, kind)}; kind: layout name, "graph" or "extreme\""""
    if _CASES:
        return _CASES
    for name in GS.CONFIGS:
        layouts = [(layout, GS.layout_case(name, layout)) for layout in GS.USED[name]]
        if "limit" in GS.USED[name]:
            layouts.append(("around", GS.around_case(name)))
        if name == "j17":
            layouts.append(("nan", GS.layout_case(name, "nan")))
        for layout, (sizes, C_obs, nrm, th) in layouts:
            for s, lo, n, v in GS.scenes_of(sizes, C_obs, nrm):
                if layout != "around" or n < GS.MAX_N:  # (the scene of 512 is layout limit's, bit for bit)
                    _CASES[f"{name}.{layout}[{s}]"] = (name, v, v, th, layout)
        for which, odd in GS.graph_cases(name):
            va, vr, th = GS.graph_case(name, which, odd)
            _CASES[f"{name}.{which}{'odd' if odd else ''}"] = (name, va, vr, th, "graph")
        for above in (False, True) if name in GS.EXTREMES else ():
            sizes, C_obs, nrm, th = GS.extreme_case(name, above)
            v = GS.scenes_of(sizes, C_obs, nrm)[0][3]
            _CASES[f"{name}.{'above' if above else 'below'}"] = (name, v, v, th, "extreme")
    return _CASES


def test_family_arena_and_workspace_figures():
    for name, cfg in GS.CONFIGS.items():
        assert (GS.arena_per_ped(*cfg), GS.lds_max_n(*cfg)) == GS.ARENA[name], name
        L = GS.ARENA[name][1]
        sizes = GS.layout_sizes(name, "edge")
        assert sizes[3] == 0 and sizes[:3] == (1, 2, 3)
        if name not in ("s1", "max"):
            assert L - 1 in sizes and L in sizes and L + 1 in sizes and L + 1 <= GS.MAX_N
        assert max(sizes) <= GS.MAX_SCENE.get(name, GS.MAX_N)
    assert GS.ARENA["s1"][1] > GS.MAX_N  # no scene ever leaves LDS
    # by hand, et (T = 8, k = 6, S = 20), one scene of 3: 6 -> 8, + 3 -> 12, + 3 -> 16, + 24 = 40, + 192 = 232, + 9 -> 244,
    # + 9 -> 256, + 72 = 328, + 6 * 9 * 20 = 1408, no arena
    et = GS.CONFIGS["et"]
    assert GS.workspace_floats(et, 3, 9, 1) == 1408
    where, total = GS.workspace_offsets(et, 34, 34 * 34, 1)   # a scene of 34 may be there: 456 floats for each of 3 N rows
    assert total - where["arena"] == 456 * 3 * 34 and GS.workspace_floats(et, 34, 34 * 34 - 1, 1) == where["arena"]
    for name in GS.CONFIGS:  # in the scene of L + 1 the group pass sits in LDS while passes 0 and 2 sit in the workspace
        which = "g3" if name == "max" else "gL1"
        if GS.graph_n(name, which) is None:
            assert name == "s1"
            continue
        va, vr, th = GS.graph_case(name, which)
        n = va.shape[1]
        assert n == GS.ARENA[name][1] + 1
        G_ = int(GS.grouping(GN.split_state(GS.with_threshold(name, th))[1], va)[1].max()) + 1
        assert G_ <= GS.ARENA[name][1] < n, (name, G_)


def test_family_seed_conditions():
    """no undecided pair; 1 < G < n for n >= 3 (the extreme thresholds: G = n and G = 1); the merge is not the connected
    components on at least three scenes, one of them above 256; in the scenes above 256 a group with members on both sides
    of index 256 and a surviving label >= 256 (a scene of 257 can have only one of the two: both occur among the scenes of
    257, and both in every scene of 512); the restatement's fp32 mode, fed its own fp32-rounded inputs of passes 1
    and 2, within TOL / 4 of its fp64 mode"""
    differs, differs_big, worst, large = 0, 0, {}, []
    for tag, (name, va, vr, th, kind) in family_cases().items():
        sd = GS.with_threshold(name, th)
        rel = None if vr is va else vr
        own = GS.forward(sd, va, v_rel=rel)
        n, g = va.shape[1], own["n_groups"]
        assert GN.pair_margin(own["dist"], float(th)) > GS.BAND_D, tag
        close = own["dist"] <= float(th)
        raw = GN.merge_literal(close)
        assert np.array_equal(GN.compact(raw), own["indices"]), tag
        if kind == "extreme":
            assert g == (1 if tag.endswith("above") else n), (tag, g)
        elif n >= 3:
            assert 1 < g < n, (tag, g, n)
            if len(np.unique(GN.merge_union_find(close))) != g:
                differs += 1
                differs_big += int(n > 256)
        if n > 256 and kind != "extreme":
            idx = own["indices"]
            straddles = bool(np.isin(idx[256:], idx[:256]).any())
            survives = bool(raw.max() >= 256)
            # (a scene of 257 has one pedestrian above 255: merged, its group straddles; alone, its label survives)
            assert (straddles and survives) if n > 257 else (straddles or survives), (tag, straddles, survives)
            large.append((n, straddles, survives))
        given = tuple(np.asarray(x, np.float32) for x in own["inputs"])
        a = GS.forward(sd, va, inputs=given, indices=own["indices"], v_rel=rel)
        b = GS.forward(sd, va, inputs=given, indices=own["indices"], v_rel=rel, dtype=np.float32)
        err = GS.rel_err(b["out"], a["out"])
        worst[name] = max(worst.get(name, 0.0), err)
        assert err <= GS.TOL / 4, (tag, err)
    print("gpgraph-stgcnn family: the restatement's fp32 mode against its fp64 mode, per configuration:",
          {k: f"{v:.2e}" for k, v in worst.items()}, "; merges that are not the connected components:", differs, differs_big)
    assert differs >= 3 and differs_big >= 1, (differs, differs_big)
    assert any(s for n, s, _ in large if n == 257) and any(v for n, _, v in large if n == 257), large


def test_family_weights_are_not_degenerate():
    """each wrong statement moves the fp64 output by more than 100 TOL on the configuration that exists for it"""
    va, vr, th = GS.graph_case("s1", "g13")
    sd = GS.with_threshold("s1", th)
    assert "baseline_model.st_gcns.0.residual.0.weight" not in sd   # S = 1: the first block's residual is the identity
    assert GS.rel_err(GS.forward(sd, va, variant=("no_identity",))["out"], GS.forward(sd, va)["out"]) > 100 * GS.TOL
    va, vr, th = GS.graph_case("j17", "g13")
    sd = GS.with_threshold("j17", th)
    assert GS.rel_err(GS.forward(sd, va, variant=("first_row",))["out"], GS.forward(sd, va)["out"]) > 100 * GS.TOL
    for name in GS.CONFIGS:
        for which in GS.ODD:
            va, vr, th = GS.graph_case(name, which, True)
            sd = GS.with_threshold(name, th)
            assert not np.array_equal(va, vr)
            assert GS.rel_err(GS.forward(sd, va)["out"], GS.forward(sd, va, v_rel=vr)["out"]) > 100 * GS.TOL, (name, which)


def test_family_fixture_is_reproduced():
    """G34 (tools/make_golden_gpgraph_stgcnn.py --family): the generated state is the recorded one (fp64 sums), the inputs
    and thresholds are GS.graph_case's, the restatement's indices are the reference's, and fed the reference's recorded v'
    and group means its output is within TOL of the recorded one"""
    cases = sorted({k.rsplit(".", 1)[0] for k in Z34.files if k.endswith(".out")})
    assert len(cases) == 4 * 6 + 2
    for name in GS.CONFIGS:
        sums = np.asarray([np.asarray(v, np.float64).sum() for v in GS.random_state(name).values()])
        assert np.array_equal(sums, Z34[f"{name}.sums"]), name
    for tag in cases:
        name, which = tag.split(".")
        odd = which.endswith("odd")
        va, vr, th = GS.graph_case(name, which[:-3] if odd else which, odd)
        assert np.array_equal(va, Z34[f"{tag}.v_abs"]) and np.array_equal(vr, Z34[f"{tag}.v_rel"]) and th == Z34[f"{tag}.th"]
        assert odd == (not np.array_equal(va, vr))
        sd = GS.with_threshold(name, th)
        own = GS.forward(sd, va, v_rel=vr)
        assert np.array_equal(own["indices"], Z34[f"{tag}.indices"]), tag
        assert GS.rel_err(Z34[f"{tag}.dist"], own["dist"]) <= GS.TOL_D
        r1, r2 = GS.check_inputs(vr, Z34[f"{tag}.v_intra"], Z34[f"{tag}.v_group"], Z34[f"{tag}.indices"])
        assert r1 <= 1.0 and r2 <= 1.0, (tag, r1, r2)
        res = GS.forward(sd, va, inputs=(Z34[f"{tag}.v_group"], Z34[f"{tag}.v_intra"]), indices=Z34[f"{tag}.indices"], v_rel=vr)
        err = GS.rel_err(Z34[f"{tag}.out"], res["out"])
        assert err <= GS.TOL, (tag, err)
        if which == "g3":
            assert float(Z34[f"{tag}.cond"]) <= GS.COND and bool(Z34[f"{tag}.ties_robust"]), tag
