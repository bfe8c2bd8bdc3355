"""CPU checks of the native GP-Graph-SGCN predictor (eigentrajectory_amd/gpgraph.py, csrc/et_gpgraph.hip): the fp64 numpy
restatement (tests/_gpgraph_np.py) against the reference's recorded distances, group indices, logits and outputs
(tests/golden/g21_gpgraph_sgcn_net.npz, tools/make_golden_gpgraph_sgcn.py) across the network's hard decisions, the row form
of the merge against the reference's literal loop, the recorded and synthetic inputs of the GPU tests against the bands and
caps, the module's state_dict against the reference's, the refusals, and the ABI's names."""
import os
import re

import numpy as np
import pytest
import torch

from . import _abi_header as H
from . import _golden as G
from . import _gpgraph_np as GN
from . import _sgcn_np as SN

Z = G.load("g21_gpgraph_sgcn_net.npz")
PICKS = sorted({k.split(".")[0] for k in Z.files if k.startswith("pick")}, key=lambda t: int(t[4:]))
SPLITS = ("eth", "hotel", "zara1")
GEN_ARGS = dict(number_asymmetric_conv_layer=3, n_tcn=2, out_dims=12)
_GEN_RESULTS = re.compile(r"^(pick|out|indices|dist|logit_)")


def net_state(prefix="net."):
    return {k[len(prefix):]: Z[k] for k in Z.files if k.startswith(prefix) and not _GEN_RESULTS.match(k[len(prefix):])}


def recorded(t, prefix=None, i=None):
    """a pick's recorded results in check_against's form (None where only the near-zero logits are stored)"""
    if prefix:
        return {"out": Z[f"gen.out{i}"][0], "indices": Z[f"gen.indices{i}"], "dist": Z[f"gen.dist{i}"],
                "logit_s": [Z[f"gen.logit_s{i}_{m}"] for m in range(3)], "logit_t": [Z[f"gen.logit_t{i}_{m}"] for m in range(3)]}
    if f"{t}.logit_s0" not in Z.files:
        return None
    return {"out": Z[f"{t}.out"][0], "indices": Z[f"{t}.indices"], "dist": Z[f"{t}.dist"],
            "logit_s": [Z[f"{t}.logit_s{m}"] for m in range(3)], "logit_t": [Z[f"{t}.logit_t{m}"] for m in range(3)]}


def et_module(**kw):
    from eigentrajectory_amd.gpgraph import GPGraphSGCN
    args = dict(obs_len=8, pred_len=6, in_dims=1, out_dims=20)
    args.update(kw)
    return GPGraphSGCN(**args)


def gen_module():
    from eigentrajectory_amd.gpgraph import GPGraph
    from eigentrajectory_amd.sgcn import SGCN
    base = SGCN(embedding_dims=64, number_gcn_layers=1, dropout=0, obs_len=8, pred_len=6, in_dims=1, position_channel=True,
                **GEN_ARGS)
    return GPGraph(base, in_channels=1, out_channels=12, obs_seq_len=8, pred_seq_len=6)


def test_fixture_covers_the_cases_the_tests_need():
    sizes = {t: Z[f"{t}.v_abs"].shape[-1] for t in PICKS}
    g20 = G.load("g20_sgcn_net.npz")
    for s in G.SCENES:  # the largest scene of every split
        assert any(str(Z[f"{t}.split"]) == s and sizes[t] == int(g20[f"{s}.scene_size"].max()) for t in PICKS), s
    for s in SPLITS:
        n = int(Z[f"{s}.scene_size"].sum())
        assert np.array_equal(Z[f"{s}.scene_size"], g20[f"{s}.scene_size"])
        assert Z[f"{s}.ade"].shape == Z[f"{s}.fde"].shape == (n,)
        assert Z[f"{s}.margin"].shape == Z[f"{s}.min_abs_logit"].shape == Z[f"{s}.n_groups"].shape == Z[f"{s}.scene_size"].shape
        assert (Z[f"{s}.n_groups"] < Z[f"{s}.scene_size"]).mean() > 0.5  # the threshold groups: most scenes pool something
    assert max(sizes.values()) == 57 and min(sizes.values()) <= 2
    hand = {str(Z[f"{t}.name"]): Z[f"{t}.indices"].tolist() for t in PICKS if str(Z[f"{t}.split"]) == "hand"}
    assert hand == {"pair": [0, 0], "chain": [0, 0, 1], "triangle": [0, 0, 0], "four": [0, 1, 0, 1]}
    th = GN.threshold(net_state())
    assert th != 1.0 and float(Z["th_margin"]) > 10 * GN.BAND_D
    for t in PICKS:
        n = sizes[t]
        assert Z[f"{t}.v_abs"].shape == (1, 1, 8, n) and Z[f"{t}.v_rel"].shape == (1, 2, 8, n)
        assert np.array_equal(Z[f"{t}.v_rel"][0, 1], Z[f"{t}.v_abs"][0, 0])
        assert np.array_equal(Z[f"{t}.v_rel"][0, 0], np.broadcast_to(np.arange(1, 9, dtype=np.float32)[:, None], (8, n)))
        assert Z[f"{t}.out"].shape == (1, 20, 6, n) and Z[f"{t}.indices"].shape == (n,) and Z[f"{t}.dist"].shape == (n, n)
        g = int(Z[f"{t}.indices"].max()) + 1
        assert Z[f"{t}.out1"].shape == (6, g, 20) and Z[f"{t}.out0"].shape == Z[f"{t}.out2"].shape == (6, n, 20)
    slopes = [v for k, v in net_state().items() if v.shape == (1,) and not k.endswith(".th")]
    assert len(slopes) == 25 and not any(np.allclose(v, 0.25) for v in slopes)  # no default PReLU slope left, the mix one too
    # a recorded scene where the loop and connected components disagree
    differ = 0
    for t in PICKS:
        close = Z[f"{t}.dist"] <= np.float32(th)
        lit, uf = GN.compact(GN.merge_literal(close)), GN.compact(GN.merge_union_find(close))
        assert np.array_equal(lit, Z[f"{t}.indices"]), t
        differ += int(lit.max() != uf.max())
    assert differ >= 3  # (the chain, the four, the univ scene)


def test_bands_and_caps_hold_for_the_reference_alone():
    """conditions on the inputs: no recorded pick, hand-built or synthetic scene has an undecided pair, at most 2 % of a
    split's scenes have one, and the undecided sigmoid entries stay within SN's caps"""
    assert all(GN.pair_margin(Z[f"{t}.dist"].astype(np.float64), GN.threshold(net_state())) > GN.BAND_D for t in PICKS)
    for s in SPLITS:
        assert (Z[f"{s}.margin"] <= GN.BAND_D).mean() <= GN.CAP_UNDECIDED_SCENES, s
        assert (Z[f"{s}.min_abs_logit"] >= SN.DELTA).mean() >= 0.90, s  # the share the end-to-end GPU test relies on


def test_numpy_restatement_reproduces_the_reference():
    """the recorded fp32 distances, indices, logits and outputs in the implementation's place"""
    sd = net_state()
    und = total = 0
    for t in PICKS:
        got = recorded(t)
        va, vr = Z[f"{t}.v_abs"][0, 0], Z[f"{t}.v_rel"][0]
        if got is not None:
            fig = GN.check_against(sd, va, vr, got)
            assert fig["compared"] and not fig["pair_undecided"]
            und, total = und + fig["undecided"], total + fig["entries"]
            continue
        # the large pick: its near-zero logits only -- the reference's decisions inside the band, the outputs to TOL
        own = GN.forward(sd, va, vr)
        assert np.array_equal(own["indices"], Z[f"{t}.indices"])
        assert np.abs(Z[f"{t}.dist"] - own["dist"]).max() <= GN.TOL_D * own["dist"].max()
        decs = []
        for m in range(3):
            pair = []
            for kind, l64 in (("s", own["passes"][m][1]), ("t", own["passes"][m][2])):
                at, val = Z[f"{t}.near_{kind}{m}"]
                at = at.astype(np.int64)
                assert np.abs(l64.ravel()[at] - val).max() <= SN.DELTA if at.size else True
                assert int((np.abs(l64) < 0.5 * GN.SN.DELTA).sum()) <= at.size  # every entry of the band is among them
                dec = SN.sigmoid(l64) > 0.5
                dec.ravel()[at] = SN.decisions_fp32(val)
                pair.append(dec)
                u = int((np.abs(l64) < SN.DELTA).sum())
                und, total = und + u, total + l64.size
            decs.append(tuple(pair))
        ref = GN.forward(sd, va, vr, decide=(decs, SN.DELTA, None, 0.0))
        err = np.abs(Z[f"{t}.out"][0] - ref["out"]).max() / np.abs(ref["out"]).max()
        print(f"gpgraph large pick N={va.shape[1]}: out_err {err:.3e}")
        assert err <= SN.TOL
        for m in range(3):
            e = np.abs(Z[f"{t}.out{m}"].transpose(2, 0, 1) - ref["passes"][m][0]).max() / np.abs(ref["passes"][m][0]).max()
            assert e <= SN.TOL, (m, e)
    assert und <= SN.CAP_SPLIT * total, (und, total)
    gen = net_state("gen.")
    assert SN.n_layers(GN.split_state(gen)[0]) == (3, 2) and SN.n_layers(GN.split_state(sd)[0]) == (7, 5)
    for i in range(2):
        t = str(Z[f"gen.pick{i}"])
        fig = GN.check_against(gen, Z[f"{t}.v_abs"][0, 0], Z[f"{t}.v_rel"][0], recorded(t, "gen.", i))
        assert fig["compared"] and fig["n_groups"] < fig["n"]


def test_decide_overrides_only_inside_the_bands():
    sd = net_state()
    t = next(t for t in PICKS if str(Z[f"{t}.split"]) == "hand" and str(Z[f"{t}.name"]) == "four")
    va, vr = Z[f"{t}.v_abs"][0, 0], Z[f"{t}.v_rel"][0]
    own = GN.forward(sd, va, vr)
    nobody = np.zeros((4, 4), bool)
    same = GN.forward(sd, va, vr, decide=(None, 0.0, nobody, 0.0))   # empty band: the given decisions are ignored
    assert np.array_equal(same["out"], own["out"]) and np.array_equal(same["indices"], own["indices"])
    other = GN.forward(sd, va, vr, decide=(None, 0.0, nobody, 10.0))  # a wide band: they are taken
    assert other["indices"].tolist() == [0, 1, 2, 3]
    assert np.abs(other["out"] - own["out"]).max() > 1e-4 * np.abs(own["out"]).max()


def test_row_form_of_the_merge_is_the_literal_loop():
    rng = np.random.default_rng(7)
    groups = 0
    for trial in range(400):
        n = int(rng.integers(1, 13))
        close = rng.random((n, n)) < rng.choice([0.1, 0.3, 0.6])
        close = close | close.T
        lit = GN.merge_literal(close)
        assert np.array_equal(GN.merge_rows(close), lit), (trial, close)
        groups += int(GN.compact(lit).max() != GN.compact(GN.merge_union_find(close)).max())
    assert groups > 20  # the loop is not connected components, and often so
    chain = np.zeros((3, 3), bool)
    chain[1, 0] = chain[2, 1] = chain[0, 1] = chain[1, 2] = True
    assert GN.compact(GN.merge_literal(chain)).tolist() == [0, 0, 1]
    assert GN.compact(GN.merge_union_find(chain)).tolist() == [0, 0, 0]


def test_synthetic_scenes_stay_within_the_bands_and_caps():
    """the ragged scenes and the synthetic split of the GPU tests: no undecided pair, each scene within the per-scene cap on
    undecided sigmoid entries, each of the two sets within the per-set one (as tests/test_sgcn_cpu.py counts them); the
    recorded group counts"""
    sd = net_state()
    th = GN.threshold(sd)
    ragged = [SN.synthetic_v(n) for n in SN.RAGGED]
    C_obs, nrm = SN.synthetic_split(SN.SPLIT_SIZES, SN.SPLIT_SEED)
    lo, split = 0, []
    for n in SN.SPLIT_SIZES:
        split.append(SN.scene_input(C_obs, nrm, lo, lo + n))
        lo += n
    at = differ = 0
    for scenes in (ragged, split):
        und_all = total_all = 0
        for v in scenes:
            res = GN.forward(sd, *GN.bridge_input(v))
            assert GN.pair_margin(res["dist"], th) > GN.BAND_D, v.shape
            assert res["n_groups"] == int(Z["synthetic.n_groups"][at]), (v.shape, res["n_groups"])
            differ += int(res["n_groups"] != int(GN.compact(GN.merge_union_find(res["close"])).max()) + 1)
            und = sum(SN.undecided(p[1], p[2])[0] for p in res["passes"])
            total = sum(SN.undecided(p[1], p[2])[1] for p in res["passes"])
            assert und <= SN.CAP_SCENE * total, (v.shape, und, total)
            und_all, total_all, at = und_all + und, total_all + total, at + 1
        assert und_all <= SN.CAP_SPLIT * total_all, (und_all, total_all)
    assert differ >= 1


def test_state_dict_names_and_shapes_are_the_references():
    for ref, net in ((net_state(), et_module()), (net_state("gen."), gen_module())):
        mine = net.state_dict()
        assert sorted(mine) == sorted(ref)
        assert all(tuple(mine[k].shape) == ref[k].shape for k in ref)
        net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in ref.items()}, strict=True)
        assert torch.equal(net.group_gen.th.detach(), torch.from_numpy(ref["group_gen.th"]))
    sd = et_module().state_dict()
    assert tuple(sd["group_gen.th"].shape) == (1,) and tuple(sd["group_gen.group_cnn.0.weight"].shape) == (8, 1, 3, 1)
    assert tuple(sd["group_mix.st_gcns_mix.1.weight"].shape) == (120, 360, 1, 1)
    assert tuple(sd["baseline_model.sparse_weighted_adjacency_matrices.temporal_attention.embedding.weight"].shape) == (64, 2)
    assert tuple(sd["baseline_model.sparse_weighted_adjacency_matrices.spatial_attention.embedding.weight"].shape) == (64, 1)
    from eigentrajectory_amd import GPGraphSGCN, get_GPGraph_SGCN_model
    assert type(get_GPGraph_SGCN_model(obs_len=8, pred_len=6, in_dims=1, out_dims=20)) is GPGraphSGCN
    get_GPGraph_SGCN_model()  # the reference's defaults construct


def test_sgcn_without_the_new_keyword_is_unchanged():
    from eigentrajectory_amd.sgcn import SGCN
    g20 = G.load("g20_sgcn_net.npz")
    plain = SGCN(number_asymmetric_conv_layer=7, obs_len=8, pred_len=6, n_tcn=5, in_dims=1, out_dims=20)
    ref = {k[4:]: g20[k] for k in g20.files if k.startswith("net.")}
    assert sorted(plain.state_dict()) == sorted(ref)
    assert all(tuple(v.shape) == ref[k].shape for k, v in plain.state_dict().items())
    assert plain.position_channel is False
    two = SGCN(number_asymmetric_conv_layer=7, obs_len=8, pred_len=6, n_tcn=5, in_dims=1, out_dims=20, position_channel=True)
    assert sorted(two.state_dict()) == sorted(ref)
    changed = [k for k, v in two.state_dict().items() if tuple(v.shape) != ref[k].shape]
    assert changed == ["sparse_weighted_adjacency_matrices.temporal_attention.embedding.weight"]


def test_reference_checkpoint_loads():
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    g2 = G.load("g2_fit_all_scenes.npz")
    hp = default_hyper_params(static_dist=G.static_dist("eth"))
    model = EigenTrajectory(et_module(), get_hook_func("gpgraphsgcn"), hp)
    ckpt = model.state_dict()
    for k, v in net_state().items():
        assert f"baseline_model.{k}" in ckpt, k
        ckpt[f"baseline_model.{k}"] = torch.from_numpy(np.array(v))
    for k in ckpt:
        if k.startswith("ET_"):
            ckpt[k] = torch.from_numpy(g2[f"eth.{k}"])
    model.load_state_dict(ckpt, strict=True)  # a reference ET-GPGraph-SGCN checkpoint's keys, unchanged
    assert torch.equal(model.baseline_model.group_gen.th.detach(), torch.from_numpy(Z["net.group_gen.th"]))
    assert any(k.startswith("baseline_model.baseline_model.") for k in ckpt)


def test_training_mode_dropout_and_unsupported_variants_raise():
    from eigentrajectory_amd.gpgraph import GPGraph
    from eigentrajectory_amd.sgcn import SGCN
    va, vr = torch.zeros((1, 1, 8, 3)), torch.zeros((1, 2, 8, 3))
    net = et_module()
    assert net.training
    with pytest.raises(RuntimeError, match="training"):
        net(va, vr)

    def base(**kw):
        args = dict(number_asymmetric_conv_layer=7, obs_len=8, pred_len=6, n_tcn=5, in_dims=1, out_dims=20, position_channel=True)
        args.update(kw)
        return SGCN(**args)

    with pytest.raises(RuntimeError, match="dropout"):
        GPGraph(base(dropout=0.1), in_channels=1, out_channels=20, obs_seq_len=8, pred_seq_len=6).eval()(va, vr)
    for kw in (dict(d_type="learned"), dict(d_type="euclidean"), dict(d_type="estimate_th"), dict(d_th=1.0),
               dict(mix_type="mean"), dict(mix_type="cnn"), dict(group_type=(True, False, True)), dict(weight_share=False)):
        bad = GPGraph(base(), in_channels=1, out_channels=20, obs_seq_len=8, pred_seq_len=6, **kw).eval()
        with pytest.raises(NotImplementedError, match="ET configuration"):
            bad(va, vr)
    with pytest.raises(NotImplementedError, match="ET configuration"):  # a one-channel base
        GPGraph(base(position_channel=False), in_channels=1, out_channels=20, obs_seq_len=8, pred_seq_len=6).eval()(va, vr)
    with pytest.raises(NotImplementedError, match="GPGraphSGCN"):       # the two-channel base on its own
        base().eval()(torch.zeros((1, 8, 3, 2)), [torch.eye(3)[None], torch.ones((3, 1, 1))])


def test_evaluate_split_refuses_other_pairings():
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    hp = default_hyper_params(static_dist=G.static_dist("eth"))
    obs, pred, sse = torch.zeros((3, 8, 2)), torch.zeros((3, 12, 2)), [[0, 3]]
    for predictor, hooks in ((et_module(), "sgcn"), (torch.nn.Linear(2, 2), "gpgraphsgcn"), (et_module(), "gpgraphstgcnn")):
        model = EigenTrajectory(predictor, get_hook_func(hooks), hp).eval()
        with pytest.raises(NotImplementedError, match="SocialSTGCNN.*SGCN.*GPGraph"):
            model.evaluate_split(obs, pred, sse)


def test_gpgraph_abi_names_declared_and_listed():
    from eigentrajectory_amd import _lib
    header = H.text()
    names = ("et_gpgraph_sgcn_workspace_bytes", "et_gpgraph_sgcn_forward_graph", "et_gpgraph_sgcn_forward_scenes")
    for name in names:
        assert re.search(rf"\b{name}\(", header) and name in _lib.SYMBOLS, name
    order = [n for n in H.functions() if n.startswith(("et_sgcn_", "et_gpgraph_"))]
    assert [n for n in _lib.SYMBOLS if n.startswith(("et_sgcn_", "et_gpgraph_"))] == order
    assert H.struct_fields("et_gpgraph_sgcn_params") == [f for f, _ in _lib.GPGraphSGCNParams._fields_]
    assert _lib.GPGraphSGCNParams._fields_[0] == ("base", _lib.SGCNParams)
    if os.path.exists(_lib.LIB_PATH):
        p = _lib.GPGraphSGCNParams()
        assert _lib.lib().et_gpgraph_sgcn_workspace_bytes(_lib.C.byref(p), _lib.i64(10), _lib.i64(100), 1) == 0  # not taken
        assert all(hasattr(_lib.lib(), name) for name in names)
