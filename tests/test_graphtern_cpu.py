"""CPU checks of the native Graph-TERN predictor (eigentrajectory_amd/graphtern.py, csrc/et_graphtern.hip): the numpy
restatement (tests/_graphtern_np.py) against the reference's recorded network outputs (tests/golden/g27_graphtern.npz,
tools/make_golden_graphtern.py), what the fixture covers, the module's state_dict against the reference's, the
evaluate_split dispatch, the entry points' argument validation (host side, before any device work) and the refusal to run
in training mode; and what tests/test_gpu_graphtern_shapes.py relies on: the path each configuration of GN.CONFIGS reaches
(the kernel's arena figures restated), its seeded weights, the restatement against the reference at those shapes
(tests/golden/g33_graphtern_family.npz), the restatement's own float32 mode on every input compared on the GPU, the exact
zeros of every layout, the NaN mask and the refusals one step outside every limit."""
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
                    dict(pred_seq_len=1, seq_len=4), dict(pred_seq_len=32, seq_len=33), dict(pred_seq_len=0, seq_len=2),
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


# ------------------------------------------------- the configurations of tests/test_gpu_graphtern_shapes.py (GN.CONFIGS)
G33 = G.load("g33_graphtern_family.npz")
# name: T, qpp, floats per pedestrian, the largest scene in LDS, the chunks of a later st_mrgcn block (None: one block)
FIGURES = {
    "k1": (3, 68, 222, 69, [1, 1, 1]),
    "k2s16": (4, 68, 228, 67, [1, 1, 1, 1]),
    "deep": (8, 128, 432, 35, [1] * 8),
    "wide": (8, 384, 1200, 12, [5, 3]),
    "kmax": (34, 2048, 6348, 2, [30, 4]),
    "tall": (34, 544, 1836, 8, [8, 8, 8, 8, 2]),
    "et": (8, 128, 432, 35, None),
}


def _cfg_params(name):
    c = GN.CONFIGS[name]
    return _params(n_epgcn=c["st"], n_epcnn=c["epcnn"], n_smpl=c["S"], seq_len=c["k"] + 2, pred_seq_len=c["k"])


def test_configs_reach_the_paths_they_are_for():
    """gt_dims_of / gt_arena_per_ped / the chunking of gt_run_scene restated (GN.dims) give the figures each configuration
    was chosen for, and the library sizes the workspace by the same rule on either side of every configuration's switch"""
    from eigentrajectory_amd import _lib
    assert {n: (c["k"], c["S"], c["st"], c["epcnn"]) for n, c in GN.CONFIGS.items()} == {
        "k1": (1, 1, 2, 2), "k2s16": (2, 16, 3, 2), "deep": (6, 9, 4, 8), "wide": (6, 64, 2, 3), "kmax": (32, 64, 2, 2),
        "tall": (32, 1, 3, 2), "et": (6, 20, 1, 6)}
    assert set(FIGURES) == set(GN.CONFIGS) and GN.LDS_BYTES // 4 == 15360
    ws = lambda name, n, mx: int(_lib.lib().et_graphtern_workspace_bytes(C.byref(_cfg_params(name)), n, mx))
    for name, (T, qpp, per, lim, later) in FIGURES.items():
        c = GN.CONFIGS[name]
        assert GN.config_dims(name) == (T, qpp, per, lim, later), name
        assert (later is None) == (c["st"] == 1) and (later is None or sum(later) == T), name
        assert per == 6 * T + 3 * qpp and per * lim * 4 <= GN.LDS_BYTES < per * (lim + 1) * 4
        assert GN.workspace_bytes(per, 1000, lim) == 0 and GN.workspace_bytes(per, 1000, lim + 1) == per * 1000 * 4
        assert GN.layout_sizes(name, "edge") == (1, 2, 3, 0, 63, 64, 65, lim, lim + 1)
        for n, mx in ((1000, lim), (1000, lim + 1), (lim, lim), (lim + 1, lim + 1), (7, 1), (16390, 16385)):
            assert ws(name, n, mx) == GN.workspace_bytes(per, n, mx), (name, n, mx)
        assert ws(name, sum(GN.layout_sizes(name, "edge")), lim + 1) == per * sum(GN.layout_sizes(name, "edge")) * 4
    floor = GN.REL * (GN.HIDDEN + 1)
    assert FIGURES["k1"][1] == FIGURES["k2s16"][1] == floor == 68 > 16 * 4 > 2 * 16          # the floor, above 16 T and k S
    assert FIGURES["wide"][1] == 6 * 64 > 16 * 8 and FIGURES["kmax"][1] == 32 * 64 > 16 * 34  # qpp from k S
    assert FIGURES["tall"][1] == 16 * 34 > 32 * 1 and FIGURES["deep"][1] == 16 * 8 > 6 * 9    # qpp from 16 T
    assert {n for n, f in FIGURES.items() if f[4] and max(f[4]) > 1} == {"wide", "kmax", "tall"}   # tq > 0 somewhere
    assert all(f[4][-1] < f[4][0] for n, f in FIGURES.items() if n in ("wide", "kmax", "tall"))     # a ragged last chunk
    assert GN.CONFIGS["k2s16"]["S"] == GN.HIDDEN                      # the last epcnn block's residual is the identity
    assert GN.CONFIGS["deep"]["st"] == _lib.GRAPHTERN_MAX_EPGCN and GN.CONFIGS["deep"]["epcnn"] == _lib.GRAPHTERN_MAX_EPCNN
    assert GN.CONFIGS["kmax"]["k"] == H.defines()["ET_MAX_K"] and FIGURES["kmax"][3] + 1 == 3  # the workspace from n = 3 on
    assert GN.BIG == (257, 512) and len(GN.MANY) == 300 and set(GN.MANY) == {0, 1, 2, 3, 4, 5}
    assert GN.NAN_SIZES == (4, 70, 40, 3, 9) and GN.FIXTURE_SIZES == (3, 13)
    assert {n for n, u in GN.USED.items() if "big" in u} == {"k1", "wide"}
    assert {n for n, u in GN.USED.items() if "many" in u} == {"k1", "et"}
    assert {n for n, u in GN.USED.items() if "nan" in u} == {"deep", "wide"}
    assert all({"edge", "g3", "g65"} <= set(u) for u in GN.USED.values()) and set(GN.USED) == set(GN.CONFIGS)
    assert set(GN.SEEDS) == {(n, l) for n, u in GN.USED.items() for l in u}


@pytest.mark.parametrize("name", list(GN.CONFIGS))
def test_config_loads_strictly_and_leaves_no_default(name):
    from eigentrajectory_amd.graphtern import GraphTERNLight
    sd = GN.random_state(name)
    net = GraphTERNLight(**GN.module_cfg(name))
    mine = net.state_dict()
    assert list(mine) == list(sd) == list(GN.state_shapes(name))
    assert all(tuple(mine[k].shape) == sd[k].shape == GN.state_shapes(name)[k] for k in sd)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    c = GN.CONFIGS[name]
    assert GN.counts(sd) == (c["st"], c["epcnn"]) and all(v.dtype == np.float32 for v in sd.values())
    slopes = [float(v[0]) for k, v in sd.items() if GN.is_slope(k)]
    assert all(sd[k].shape == (1,) for k in sd if GN.is_slope(k)) and len(slopes) == 2 * c["st"] + 2 * c["epcnn"]
    assert len(set(slopes)) == len(slopes) and all(abs(a - 0.25) > 0.02 and a > 0.04 for a in slopes)
    assert all(f"tp_mrgcns.{i}.prelu.weight" in sd for i in range(c["st"]))  # the slope the network never applies
    assert all(np.abs(v).min() > 0 for k, v in sd.items() if k.endswith("bias"))
    assert "tp_mrgcns.0.residual.0.weight" in sd and not any(f"tp_mrgcns.{i}.residual.0.weight" in sd for i in range(1, 4))
    last = c["epcnn"] - 1
    assert "tpcnns.0.restconv.0.weight" in sd and (f"tpcnns.{last}.rescconv.0.weight" in sd) == (c["S"] != 16)
    assert sum("rescconv" in k or "restconv" in k for k in sd) == (4 if c["S"] != 16 else 2)
    for other in GN.CONFIGS:  # no two configurations share a draw
        if other != name:
            assert not np.array_equal(GN.random_state(other)["tpcnns.0.cpcns.0.1.weight"], sd["tpcnns.0.cpcns.0.1.weight"])
    assert all(np.array_equal(v, GN.random_state(name)[k]) for k, v in sd.items())  # seeded


def test_the_split_generator_keeps_its_bits_and_the_float64_default_too():
    """GN.synthetic_split is tests/test_gpu_graphtern.py's former _synthetic (an int or the scene sizes, any k), and the
    restatement's default is fp64 as before the dtype argument"""
    a, b = GN.synthetic_split(65, 1), GN.synthetic_split((1, 0, 64), 1, 6)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].shape == (6, 65) and a[1].shape == (4, 65)
    assert np.array_equal(a[0][:, 21], a[0][:, 20]) and np.array_equal(a[1][:, 21], a[1][:, 20])  # the same pedestrian twice
    assert np.array_equal(a[0][:, 22], np.random.default_rng(1).normal(0, 1, (6, 65)).astype(np.float32)[:, 22])
    assert GN.synthetic_split((3, 4), 2, 1)[0].shape == (1, 7) and GN.synthetic_split((3, 4), 2, 32)[0].shape == (32, 7)
    sd = net_state()
    u = Z["grid.s_obs"][0, 0, :, :, 0]
    o = GN.forward(sd, u)
    assert o.dtype == np.float64 and np.array_equal(o, GN.forward(sd, u, dtype=np.float64))
    assert GN.graphs(u, GN.rel_of(u)).dtype == np.float64 and GN.graphs(u, GN.rel_of(u), np.float32).dtype == np.float32


def test_the_restatement_reproduces_the_reference_across_the_family():
    """g33: the reference's graph_tern_light at every configuration under GN.random_state, on the bridge's S_obs of the
    scenes of 3 and 13 (tools/make_golden_graphtern.py --family; no configuration was refused): the inputs are regenerated
    bit for bit, the fp64 restatement is within TOL of every output.  Measured: k1 2.0e-7, k2s16 1.8e-7, deep 3.2e-7, wide
    3.8e-7, kmax 3.1e-7, tall 6.8e-7, et 3.3e-7"""
    assert sorted(G33.files) == sorted(f"{name}.{what}{n}" for name in GN.CONFIGS for what in ("s_obs", "net_out")
                                       for n in GN.FIXTURE_SIZES)
    for name, c in GN.CONFIGS.items():
        sd = GN.random_state(name)
        sizes, C_obs, nrm = GN.fixture_inputs(name)
        worst = 0.0
        for _, lo, n, u in GN.scenes_of(sizes, C_obs, nrm):
            s_obs, ref = G33[f"{name}.s_obs{n}"], G33[f"{name}.net_out{n}"]
            assert s_obs.shape == (2, c["k"] + 2, n) and ref.shape == (c["k"], n, c["S"]) and ref.dtype == np.float32
            assert np.array_equal(GN.s_obs_of(u)[0, :, :, :, 0], s_obs), (name, n)
            errs = (scale_err(GN.forward(sd, s_obs[0], s_obs[1]), ref), scale_err(GN.forward(sd, u), ref))
            worst = max(worst, *errs)
            assert max(errs) <= TOL, (name, n, errs)
        print(f"graphtern {name}: restatement against the reference {worst:.2e} of the largest entry")


def _compared_inputs(name):
    """yields (label, u, rel or None) of every network input tests/test_gpu_graphtern_shapes.py compares at ``name``: the
    non-empty scenes of its layouts, the g33 scenes, and the graph-form scenes of 3 and 65 with GN.odd_rel"""
    for layout in GN.USED[name]:
        sizes, C_obs, nrm = GN.layout_inputs(name, layout)
        got = 0
        for s, _, n, u in GN.scenes_of(sizes, C_obs, nrm):
            got += 1
            yield layout, u, None
            if layout in ("g3", "g65"):
                yield layout + " odd rel", u, GN.odd_rel(u)
        assert got == sum(1 for n in sizes if n)  # no scene left out
    sizes, C_obs, nrm = GN.fixture_inputs(name)
    for _, _, n, u in GN.scenes_of(sizes, C_obs, nrm):
        yield "g33", u, None


@pytest.mark.parametrize("name", list(GN.CONFIGS))
def test_float32_mode_is_within_a_quarter_of_the_tolerance(name):
    """the restatement in numpy fp32 after the fp32 distances (the same statements, the arithmetic's own error) against
    itself in fp64 on every network input the GPU file compares: within TOL / 4 of the largest entry.  Measured (edge, g3,
    g65, then the others; the odd rel among g3 / g65): k1 8.3e-7, 8.7e-7, 3.6e-7, big 3.3e-7, many 1.3e-6; k2s16 1.9e-7,
    1.5e-7, 2.3e-7; deep 2.8e-7, 2.7e-7, 2.6e-7, nan 2.7e-7; wide 2.5e-7, 2.2e-7, 2.1e-7, big 2.3e-7, nan 2.2e-7; kmax
    2.5e-7, 1.9e-7, 1.8e-7; tall 3.8e-7, 3.6e-7, 2.9e-7; et 2.2e-7, 2.2e-7, 1.5e-7, many 3.6e-7"""
    sd, c = GN.random_state(name), GN.CONFIGS[name]
    worst = {}
    for label, u, rel in _compared_inputs(name):
        o64, o32 = GN.forward(sd, u, rel), GN.forward(sd, u, rel, dtype=np.float32)
        assert o32.dtype == np.float32 and o64.dtype == np.float64 and o64.shape == (c["k"], u.shape[1], c["S"])
        assert np.isfinite(o64).all()
        key = label.split()[0]
        worst[key] = max(worst.get(key, 0.0), scale_err(o32, o64))
    assert set(worst) == set(GN.USED[name]) | {"g33"}
    for key, err in worst.items():
        print(f"graphtern {name} {key}: float32 mode {err:.2e} of the largest entry (bound {GN.TOL / 4:.1e})")
        assert err <= GN.TOL / 4, (name, key, err)


def test_every_layout_has_exact_zeros_off_the_diagonal():
    """in both relations, in every time row (of rel: every row but the all-zero first), in some scene of every layout of
    every configuration -- coincident columns, rounded values, all-zero columns; and GN.odd_rel is what it says"""
    for name, used in GN.USED.items():
        k = GN.CONFIGS[name]["k"]
        for layout in used:
            sizes, C_obs, nrm = GN.layout_inputs(name, layout)
            both, tied_values = 0, False
            for _, lo, n, u in GN.scenes_of(sizes, C_obs, nrm):
                off = ~np.eye(n, dtype=bool)
                za, zr = (GN.distances(u) == 0) & off, (GN.distances(GN.rel_of(u)) == 0) & off
                both += bool(za.any(axis=(1, 2)).all() and zr.any(axis=(1, 2))[1:].all())
                pair = za.all(axis=0)  # the same pedestrian twice: zero in every row
                tied_values |= bool((za[:k] & ~pair).any())
            assert both >= 1, (name, layout)
            assert tied_values or max(sizes) < 8 or k > 6, (name, layout)  # equal rounded values beyond the repeated columns
            assert (C_obs == 0).all(axis=0).any() or C_obs.shape[1] <= 3
    for name, n in (("k1", 3), ("deep", 65), ("kmax", 13)):
        C_obs, nrm = GN.synthetic_split((n,), 1, GN.CONFIGS[name]["k"])
        u = GN.scene_input(C_obs, nrm, 0, n)
        rel = GN.odd_rel(u)
        assert rel.dtype == np.float32 and rel.shape == u.shape and rel[0].any()
        assert not np.array_equal(rel, GN.rel_of(u)) and np.abs(rel - GN.rel_of(u)).max() > 0.1
        if n >= 4:
            off = ~np.eye(n, dtype=bool)
            new = (GN.distances(rel) == 0) & off & ~((GN.distances(u) == 0) & off)
            assert new[:, 2, 3].all() and new[1::2, 0, n - 1].all() and not new[0::2, 0, n - 1].any()
        sd = GN.random_state(name)
        assert scale_err(GN.forward(sd, u, rel), GN.forward(sd, u)) > 1e-3  # rel is read as given


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("name", ["deep", "wide", "et"])
def test_a_nan_coefficient_poisons_the_whole_scene_in_the_restatement(name, value):
    """the reference's arithmetic, restated: a NaN (or inf: |inf - inf|) coefficient makes its pedestrian's row and column
    of A, every degree of that time row and so the whole time row NaN; the tcn carries it to the rows next to it and the
    first epcnn convolution, which sums over all rows, to the whole scene.  tests/test_gpu_graphtern_shapes.py and
    tests/test_gpu_graphtern.py hold the device to this mask"""
    sd = GN.random_state(name)
    C_obs, nrm = GN.synthetic_split((40,), 3, GN.CONFIGS[name]["k"])
    C_obs[3, 17] = value
    with np.errstate(invalid="ignore", divide="ignore"):
        out = GN.forward(sd, GN.scene_input(C_obs, nrm, 0, 40))
    assert np.isnan(out).all()


def test_one_step_outside_every_limit_is_refused_on_the_host():
    """the refusals test_arguments_are_validated_on_the_host leaves out, at ranks other than 6 too: k = 0 and 33, S = 0 and
    65, no st_mrgcn block and five, one epcnn block and nine, seq_len one off k + 2 on either side at k = 1, 2 and 32; the
    accepted side of each limit is a member of GN.CONFIGS.  Both entry points, before any launch (the calls run without a
    device); the workspace size of each is 0"""
    from eigentrajectory_amd import _lib
    lib = _lib.lib()
    UNSUPPORTED = H.defines()["ET_ERR_UNSUPPORTED"]
    bad = {"k = 0": dict(pred_seq_len=0, seq_len=2), "k = 33": dict(pred_seq_len=33, seq_len=35),
           "S = 0": dict(n_smpl=0), "S = 65": dict(n_smpl=65), "n_epgcn = 0": dict(n_epgcn=0),
           "n_epgcn = 5": dict(n_epgcn=_lib.GRAPHTERN_MAX_EPGCN + 1), "n_epcnn = 1": dict(n_epcnn=1),
           "n_epcnn = 9": dict(n_epcnn=_lib.GRAPHTERN_MAX_EPCNN + 1)}
    for k in (1, 2, 32):
        bad[f"seq_len = k + 1, k = {k}"] = dict(pred_seq_len=k, seq_len=k + 1)
        bad[f"seq_len = k + 3, k = {k}"] = dict(pred_seq_len=k, seq_len=k + 3)
    bad["k = 32 under seq_len 8"] = dict(pred_seq_len=32)
    for name, c in GN.CONFIGS.items():  # every configuration one step outside in S and in the block counts
        base = dict(n_epgcn=c["st"], n_epcnn=c["epcnn"], n_smpl=c["S"], seq_len=c["k"] + 2, pred_seq_len=c["k"])
        bad[f"{name} S = 65"] = dict(base, n_smpl=65)
        bad[f"{name} n_epgcn = 0"] = dict(base, n_epgcn=0)
        bad[f"{name} seq_len = k + 1"] = dict(base, seq_len=c["k"] + 1)
    for what, kw in bad.items():
        p = _params(**kw)
        assert lib.et_graphtern_forward_graph(C.byref(p), 8, 3, 8, None, 0, None) == UNSUPPORTED, what
        assert lib.et_graphtern_forward_scenes(C.byref(p), 8, 8, 3, None, 0, 8, None, None, 0, None) == UNSUPPORTED, what
        assert int(lib.et_graphtern_workspace_bytes(C.byref(p), 5000, 100)) == 0, what
    for name in GN.CONFIGS:  # the accepted side: N = 0 is answered ET_OK once the parameters have passed
        assert lib.et_graphtern_forward_graph(C.byref(_cfg_params(name)), None, 0, None, None, 0, None) == 0, name
        assert lib.et_graphtern_forward_scenes(C.byref(_cfg_params(name)), None, None, 0, None, 0, None, None, None, 0,
                                               None) == 0, name
