"""CPU checks of the native Graph-TERN predictor (eigentrajectory_amd/graphtern.py, csrc/et_graphtern.hip): the numpy
restatement (tests/_graphtern_np.py) against the reference's recorded network outputs (tests/golden/g27_graphtern.npz,
tools/make_golden_graphtern.py), what the fixture covers, the module's state_dict against the reference's, the
evaluate_split dispatch, the entry points' argument validation (host side, before any device work) and the refusal to run
in training mode."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from . import _abi_header as H
from . import _golden as G
from . import _graphtern_np as GN

Z = G.load("g27_graphtern.npz")
PICKS = sorted({k.split(".")[0] for k in Z.files if k.startswith("pick")}, key=lambda t: int(t[4:]))
HAND = ["grid", "single", "pair", "edge"]
TOL = 1e-5  # of the largest entry; the reference's own fp32 run against its fp64 run differs by 4.4e-7
GEN = dict(n_epgcn=2, n_epcnn=3, n_smpl=12)


def net_state(prefix="net."):
    return {k[len(prefix):]: Z[k] for k in Z.files if k.startswith(prefix) and not k[len(prefix):].startswith("net_out")}


def et_module(**kw):
    from eigentrajectory_amd.graphtern import GraphTERNLight
    args = dict(n_epgcn=1, n_epcnn=6, input_feat=1, seq_len=8, pred_seq_len=6, n_smpl=20)
    args.update(kw)
    return GraphTERNLight(**args)


def scale_err(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


def eth_scenes():
    """(u, rel, net_out) of every eth test scene"""
    lo = 0
    for n in Z["eth.scene_size"]:
        yield Z["eth.s_obs"][0][:, lo:lo + n], Z["eth.s_obs"][1][:, lo:lo + n], Z["eth.net_out"][:, lo:lo + n]
        lo += int(n)


def test_fixture_covers_the_cases_the_tests_need():
    obs, _, sse = G.dataset("eth", "test")
    assert Z["eth.scene_size"].tolist() == (sse[:, 1] - sse[:, 0]).tolist()  # EVERY eth test scene
    n_eth = int(Z["eth.scene_size"].sum())
    assert Z["eth.s_obs"].shape == (2, 8, n_eth) and Z["eth.net_out"].shape == (6, n_eth, 20)
    assert Z["eth.c_obs"].shape == (6, n_eth) and np.array_equal(Z["eth.c_obs"], Z["eth.s_obs"][0][:6])
    sizes = {str(Z[f"{t}.split"]): [] for t in PICKS}
    for t in PICKS:
        sizes[str(Z[f"{t}.split"])].append(Z[f"{t}.s_obs"].shape[3])
    assert set(sizes) == set(G.SCENES)
    for s in G.SCENES:  # the largest test scene of each split
        _, _, sse = G.dataset(s, "test")
        assert max(sizes[s]) == int((sse[:, 1] - sse[:, 0]).max()) == int(Z[f"{s}.scene_size"].max())
        assert Z[f"{s}.ade_spread"] > 0 and Z[f"{s}.fde_spread"] > 0 and 0 <= Z[f"{s}.moved_share"] <= 1
        assert 0.1 < Z[f"{s}.ade_mean"] < Z[f"{s}.fde_mean"] < 2
    tied = False  # an off-diagonal exact zero of A_abs between two non-zero values, in a small scene
    for t in PICKS:
        u = Z[f"{t}.s_obs"][0, 0, :, :, 0]
        if 2 <= u.shape[1] <= 30:
            for row in u:
                nz = row[row != 0]
                tied |= len(np.unique(nz)) < len(nz)
    assert tied
    for prefix, n_slopes in (("net.", 2 * 1 + 2 * 6), ("gen.", 2 * 2 + 2 * 3)):
        slopes = [float(v.reshape(-1)[0]) for k, v in net_state(prefix).items() if v.size == 1]
        assert len(slopes) == n_slopes and len(set(slopes)) == len(slopes) and 0.25 not in slopes  # every PReLU its own
    assert "tp_mrgcns.0.prelu.weight" in net_state()  # the slope the network never applies is there (and non-default)
    shapes = {t: Z[f"{t}.s_obs"].shape for t in HAND}
    assert shapes == {"grid": (1, 2, 8, 12, 1), "single": (1, 2, 8, 1, 1), "pair": (1, 2, 8, 2, 1), "edge": (1, 2, 8, 3, 1)}
    grid = Z["grid.s_obs"][0, 0, :, :, 0]
    assert np.array_equal(grid * 4, np.round(grid * 4)) and np.array_equal(grid[:, 2], grid[:, 5])
    zeros = (GN.distances(grid) == 0) & ~np.eye(12, dtype=bool)
    zeros[:, 2, 5] = zeros[:, 5, 2] = False
    assert zeros.any(axis=(1, 2)).sum() >= 4  # off-diagonal zeros beyond the identical pair, in at least half the time rows
    for t in PICKS + HAND:  # row 0 of rel is zero: its two graphs are the identity
        s_obs = Z[f"{t}.s_obs"]
        assert not s_obs[0, 1, 0].any() and np.array_equal(s_obs[0, 1, :, :, 0], GN.rel_of(s_obs[0, 0, :, :, 0])), t
    assert not Z["eth.s_obs"][1][0].any()
    assert [Z[f"gen.net_out{i}"].shape for i in range(2)] == [(1, 6, Z[f"{t}.s_obs"].shape[3], 12) for t in PICKS[:2]]


def test_numpy_restatement_reproduces_the_reference():
    sd = net_state()
    worst = 0.0
    for i, (u, rel, ref) in enumerate(eth_scenes()):
        err = scale_err(GN.forward(sd, u, rel), ref)
        worst = max(worst, err)
        assert err <= TOL, ("eth", i, err)
    for t in PICKS + HAND:
        s_obs = Z[f"{t}.s_obs"]
        u, rel = s_obs[0, 0, :, :, 0], s_obs[0, 1, :, :, 0]
        assert np.array_equal(GN.s_obs_of(u), s_obs), t  # the bridge's layout, bit for bit
        errs = (scale_err(GN.forward(sd, u, rel), Z[f"{t}.net_out"][0]), scale_err(GN.forward(sd, u), Z[f"{t}.net_out"][0]))
        worst = max(worst, *errs)
        assert max(errs) <= TOL, (t, errs)
    gen = net_state("gen.")
    assert GN.counts(gen) == (2, 3) and GN.counts(sd) == (1, 6)
    for i, t in enumerate(PICKS[:2]):
        err = scale_err(GN.forward(gen, Z[f"{t}.s_obs"][0, 0, :, :, 0]), Z[f"gen.net_out{i}"][0])
        worst = max(worst, err)
        assert err <= TOL, (t, err)
    print(f"restatement against the reference: {worst:.2e} of the largest entry")


def test_the_fixture_tells_the_variants_apart(monkeypatch):
    """zero padding instead of replication, the unused PReLU applied, a tolerance band around A == 0: each misses the bound"""
    sd = net_state()
    u = Z["grid.s_obs"][0, 0, :, :, 0]
    ref = Z["grid.net_out"][0]
    assert scale_err(GN.forward(sd, u), ref) <= TOL
    with monkeypatch.context() as m:
        m.setattr(GN, "PAD_MODE", "constant")
        assert scale_err(GN.forward(sd, u), ref) > TOL
    moved = dict(sd)
    moved["tpcnns.3.cpcns.0.1.weight"] = sd["tpcnns.2.cpcns.0.1.weight"]  # a swapped slope
    assert scale_err(GN.forward(moved, u), ref) > TOL
    nudged = u.copy()
    nudged[:, 5] = np.nextafter(nudged[:, 5], np.float32(np.inf))  # the identical pair an ulp apart: 1 / 2^-22 and more
    assert scale_err(GN.forward(sd, nudged), ref) > TOL


def test_state_dict_names_and_shapes_are_the_references():
    for prefix, kw in (("net.", {}), ("gen.", GEN)):
        ref = net_state(prefix)
        net = et_module(**kw)
        mine = net.state_dict()
        assert sorted(mine) == sorted(ref)
        assert all(tuple(mine[k].shape) == ref[k].shape for k in ref)
        net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in ref.items()}, strict=True)
        assert torch.equal(net.tpcnns[0].restconv[0].bias, torch.from_numpy(ref["tpcnns.0.restconv.0.bias"]))
    assert sorted(et_module(n_smpl=16).state_dict()) == sorted(str(k) for k in Z["keys.s16"])
    sd = et_module().state_dict()
    assert sd["tp_mrgcns.0.gcn.conv.weight"].shape == (64, 1, 1, 1) and sd["tp_mrgcns.0.residual.0.weight"].shape == (16, 1, 1, 1)
    assert sd["tpcnns.0.tpcns.0.0.weight"].shape == (6, 8, 3, 3) and sd["tpcnns.5.cpcns.0.0.weight"].shape == (20, 16, 3, 3)
    assert sd["tpcnns.5.rescconv.0.weight"].shape == (20, 16, 1, 1) and "tpcnns.4.rescconv.0.weight" not in sd
    assert "tpcnns.1.restconv.0.weight" not in sd and "tp_mrgcns.0.prelu.weight" in sd
    assert "tp_mrgcns.1.residual.0.weight" not in et_module(**GEN).state_dict()  # C_in = 16: identity
    assert not any("running" in k for k in sd)  # no BatchNorm anywhere
    import inspect
    from eigentrajectory_amd.graphtern import GraphTERNLight
    defaults = {k: v.default for k, v in inspect.signature(GraphTERNLight.__init__).parameters.items() if k != "self"}
    assert defaults == dict(n_epgcn=1, n_epcnn=6, input_feat=2, seq_len=8, pred_seq_len=12, n_smpl=20)  # model.py:221


def test_reference_checkpoint_loads_into_the_wrapper():
    from eigentrajectory_amd import EigenTrajectory, GraphTERNLight
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    assert GraphTERNLight is type(et_module())
    g2 = G.load("g2_fit_all_scenes.npz")
    hp = default_hyper_params(static_dist=G.static_dist("eth"))
    model = EigenTrajectory(et_module(), get_hook_func("graphtern"), hp)
    ckpt = model.state_dict()
    for k, v in net_state().items():
        ckpt[f"baseline_model.{k}"] = torch.from_numpy(np.array(v))
    for k in ckpt:
        if k.startswith("ET_"):
            ckpt[k] = torch.from_numpy(g2[f"eth.{k}"])
    model.load_state_dict(ckpt, strict=True)  # a reference ET-Graph-TERN checkpoint's keys, unchanged
    assert torch.equal(model.baseline_model.tp_mrgcns[0].prelu.weight, torch.from_numpy(Z["net.tp_mrgcns.0.prelu.weight"]))


def test_training_mode_forward_raises():
    net = et_module()
    assert net.training
    with pytest.raises(RuntimeError, match="training"):
        net(torch.zeros((1, 2, 8, 3, 1)))


def test_evaluate_split_dispatch():
    """the graphtern pairing gets past the dispatch (and stops at the missing device); under other hooks it does not"""
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd._lib import ETLibraryError
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    obs, pred = torch.zeros(3, 8, 2), torch.zeros(3, 12, 2)
    model = EigenTrajectory(et_module(), get_hook_func("graphtern"), default_hyper_params(static_dist=0.3)).eval()
    if not torch.cuda.is_available():
        with pytest.raises((ETLibraryError, RuntimeError, ValueError)) as exc:
            model.evaluate_split(obs, pred, [[0, 3]])
        assert not isinstance(exc.value, NotImplementedError)
    model.train()
    with pytest.raises(RuntimeError, match="training mode"):
        model.evaluate_split(obs, pred, [[0, 3]])
    for predictor, hooks in ((et_module(), "stgcnn"), (et_module(), "dmrgcn"), (torch.nn.Linear(2, 2), "graphtern")):
        model = EigenTrajectory(predictor, get_hook_func(hooks), default_hyper_params(static_dist=0.3)).eval()
        with pytest.raises(NotImplementedError, match="AgentFormerLight.*'agentformer'.*GraphTERNLight.*'graphtern'"):
            model.evaluate_split(obs, pred, [[0, 3]])


def _params(**kw):
    """et_graphtern_params of the ET configuration whose every pointer is a (never dereferenced) non-NULL host address"""
    from eigentrajectory_amd import _lib
    p = _lib.GraphTERNParams()
    p.n_epgcn, p.n_epcnn, p.input_feat, p.hidden_feat, p.seq_len, p.pred_seq_len, p.n_smpl = 1, 6, 1, 16, 8, 6, 20
    for k, v in kw.items():
        setattr(p, k, v)
    dummy = 8
    for i in range(_lib.GRAPHTERN_MAX_EPGCN):
        l = p.tp_mrgcns[i]
        l.gcn_w = l.gcn_b = l.tcn_prelu = l.tcn_w = l.tcn_b = l.prelu = dummy
        if i == 0:
            l.res_w = l.res_b = dummy
    for j in range(_lib.GRAPHTERN_MAX_EPCNN):
        e = p.tpcnns[j]
        e.tpcn_w = e.tpcn_b = e.tpcn_a = e.cpcn_w = e.cpcn_b = e.cpcn_a = dummy
        if j == 0:
            e.rest_w = e.rest_b = dummy
        if j == p.n_epcnn - 1 and p.n_smpl != 16:
            e.resc_w = e.resc_b = dummy
    return p


def test_arguments_are_validated_on_the_host():
    """Every refusal below is answered before a launch: the calls run without a device."""
    from eigentrajectory_amd import _lib
    lib = _lib.lib()
    UNSUPPORTED, INVALID = H.defines()["ET_ERR_UNSUPPORTED"], H.defines()["ET_ERR_INVALID_ARG"]

    def graph(p):
        return lib.et_graphtern_forward_graph(C.byref(p), 8, 3, 8, None, 0, None)

    def scenes(p):
        return lib.et_graphtern_forward_scenes(C.byref(p), 8, 8, 3, None, 0, 8, None, None, 0, None)

    for call in (graph, scenes):
        for bad in (dict(n_smpl=65), dict(n_smpl=0), dict(seq_len=9), dict(pred_seq_len=33, seq_len=35), dict(input_feat=2),
                    dict(hidden_feat=32), dict(n_epgcn=0), dict(n_epgcn=_lib.GRAPHTERN_MAX_EPGCN + 1), dict(n_epcnn=1),
                    dict(n_epcnn=_lib.GRAPHTERN_MAX_EPCNN + 1)):
            assert call(_params(**bad)) == UNSUPPORTED, bad
        p = _params()
        p.tp_mrgcns[0].gcn_b = None
        assert call(p) == INVALID
        p = _params()
        p.tpcnns[5].cpcn_a = None
        assert call(p) == INVALID
        p = _params()
        p.tpcnns[0].rest_w = None  # T != k in the first block: the residual is a convolution
        assert call(p) == INVALID
        p = _params()
        p.tpcnns[5].resc_w = None  # 16 != S in the last block
        assert call(p) == INVALID
        p = _params()
        p.tpcnns[2].resc_w = 8  # a middle block's residual is the identity
        assert call(p) == INVALID
    # N = 0 is nothing to do; a missing input is refused
    assert lib.et_graphtern_forward_graph(None, 8, 3, 8, None, 0, None) == INVALID
    assert lib.et_graphtern_forward_graph(C.byref(_params()), None, 0, None, None, 0, None) == 0
    assert lib.et_graphtern_forward_graph(C.byref(_params()), None, 3, 8, None, 0, None) == INVALID
    assert lib.et_graphtern_forward_scenes(C.byref(_params()), None, 8, 3, None, 0, 8, None, None, 0, None) == INVALID
    assert lib.et_graphtern_forward_scenes(C.byref(_params(n_smpl=16)), None, None, 0, None, 0, None, None, None, 0, None) == 0
    # workspace: none while the largest scene fits the LDS arena (S = 20, k = 6: 6 * 8 + 3 * 128 floats per pedestrian, 35)
    ws = lambda p, n, mx: int(lib.et_graphtern_workspace_bytes(C.byref(p), n, mx))
    assert ws(_params(), 5000, 35) == 0 and ws(_params(), 5000, 36) == 5000 * 432 * 4
    assert ws(_params(n_smpl=65), 5000, 100) == 0  # outside the family: not taken
    assert ws(_params(n_smpl=64), 100, 100) == 100 * (48 + 3 * 6 * 64) * 4  # the last block's (k, S) planes
    assert ws(_params(pred_seq_len=1, seq_len=3, n_epgcn=2), 100, 100) == 100 * (18 + 3 * 68) * 4  # C_in = 16: 4 * 17 rows


def test_graphtern_abi_names_declared_and_mirrored():
    from eigentrajectory_amd import _lib
    header = H.text()
    for name in ("et_graphtern_workspace_bytes", "et_graphtern_forward_graph", "et_graphtern_forward_scenes"):
        assert re.search(rf"\b{name}\(", header) and name in _lib.SYMBOLS, name
        assert hasattr(_lib.lib(), name)
    assert _lib.SYMBOLS.index("et_graphtern_workspace_bytes") == _lib.SYMBOLS.index("et_agentformer_forward_scenes") + 1
    for struct, mirror in (("et_graphtern_layer", _lib.GraphTERNLayer), ("et_graphtern_epcnn", _lib.GraphTERNEpcnn),
                           ("et_graphtern_params", _lib.GraphTERNParams)):
        assert H.struct_fields(struct) == [f for f, _ in mirror._fields_], struct
    d = H.defines()
    assert (d["ET_GRAPHTERN_MAX_EPGCN"], d["ET_GRAPHTERN_MAX_EPCNN"]) == (_lib.GRAPHTERN_MAX_EPGCN, _lib.GRAPHTERN_MAX_EPCNN)
    assert d["ET_GRAPHTERN_MAX_EPGCN"] >= 2 and d["ET_GRAPHTERN_MAX_EPCNN"] >= 6 and d["ET_ABI_VERSION"] == 3
    assert C.sizeof(_lib.GraphTERNLayer) == 8 * 8 and C.sizeof(_lib.GraphTERNEpcnn) == 10 * 8
    assert C.sizeof(_lib.GraphTERNParams) == 7 * 4 + 4 + 4 * 8 * 8 + 8 * 10 * 8  # ints, padding, pointer tables
