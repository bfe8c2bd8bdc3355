"""CPU checks of the native DMRGCN predictor (eigentrajectory_amd/dmrgcn.py, csrc/et_dmrgcn.hip): the numpy restatement
(tests/_dmrgcn_np.py) against the reference's recorded outputs (tests/golden/g23_dmrgcn.npz, tools/make_golden_dmrgcn.py),
that the fixture tells open from closed bins, the module's state_dict against the reference's, the entry points' argument
validation (host side, before any device work) and the refusal to run in training mode; and the pre-conditions of
tests/test_gpu_dmrgcn_shapes.py: the path each configuration of DN.CONFIGS reaches, its seeded weights, the restatement's
fp32 mode against its fp64 mode on every input the GPU file compares, the given-a path against a dense form."""
import ctypes as C
import os
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


# ------------------------------------------------- the configurations of tests/test_gpu_dmrgcn_shapes.py (DN.CONFIGS)
# name: K, qpp, floats per pedestrian, largest scene in LDS, chunks of the first block, chunks of a later block
FIGURES = {
    "k1": (3, 20, 96, 160, [1, 1, 1], None),
    "narrow": (9, 45, 243, 63, [2, 2, 2, 2, 1], None),
    "deep": (8, 100, 396, 38, [5, 3], [1] * 8),
    "wide3": (4, 650, 1998, 7, [4], [1] * 4),
    "kmax": (34, 2176, 6936, 2, [34], [3] * 11 + [1]),
    "et": (8, 160, 576, 26, [8], None),
}


def _cfg_params(name):
    c = DN.CONFIGS[name]
    p = _params(n_stgcn=c["st"], n_tpcnn=c["tp"], output_feat=c["S"], seq_len=c["k"] + 2, pred_seq_len=c["k"])
    if c["S"] == 1:  # input_feat = output_feat: the first block's residual is the identity
        p.st_dmrgcns[0].res_w = p.st_dmrgcns[0].res_b = None
    return p


def test_configs_reach_the_paths_they_are_for():
    """dm_dims_of / dm_arena_per_ped / the chunking restated (DN.dims) give the figures each configuration was chosen for,
    and the library sizes the workspace by the same rule on either side of every configuration's switch"""
    from eigentrajectory_amd import _lib
    assert {n: (c["k"], c["S"], c["st"], c["tp"]) for n, c in DN.CONFIGS.items()} == {
        "k1": (1, 1, 1, 1), "narrow": (7, 5, 1, 2), "deep": (6, 9, 4, 8), "wide3": (2, 64, 3, 2), "kmax": (32, 64, 2, 1),
        "et": (6, 20, 1, 4)}
    for name, (K, qpp, per, lim, first, later) in FIGURES.items():
        c = DN.CONFIGS[name]
        gK, gq, gper, glim, nt_first, nt_later = DN.config_dims(name)
        assert (gK, gq, gper, glim) == (K, qpp, per, lim), name
        assert DN.chunks(K, nt_first) == first and (nt_later is None) == (later is None) == (c["st"] == 1), name
        if later is not None:
            assert DN.chunks(K, nt_later) == later, name
        assert per * lim * 4 <= DN.LDS_BYTES < per * (lim + 1) * 4
        assert DN.workspace_bytes(per, 1000, lim) == 0 and DN.workspace_bytes(per, 1000, lim + 1) == per * 1000 * 4
        assert DN.layout_sizes(name, "edge") == (1, 2, 3, 0, 63, 64, 65, lim, lim + 1)
        if os.path.exists(_lib.LIB_PATH):
            ws = lambda n, mx: int(_lib.lib().et_dmrgcn_workspace_bytes(C.byref(_cfg_params(name)), n, mx))
            for n, mx in ((1000, lim), (1000, lim + 1), (lim, lim), (lim + 1, lim + 1), (7, 1), (16390, 16385)):
                assert ws(n, mx) == DN.workspace_bytes(per, n, mx), (name, n, mx)
    assert FIGURES["k1"][1] == 2 * DN.RB > 1 * 3                      # the floor of dm_dims_of, S K = 3 below it
    assert (DN.CONFIGS["deep"]["S"] + 1) % 2 == 0 and (DN.CONFIGS["wide3"]["S"] + 1) % 2 == 1  # J even: every lane pair full
    assert DN.CONFIGS["deep"]["st"] == _lib.DMRGCN_MAX_STGCN and DN.CONFIGS["deep"]["tp"] == _lib.DMRGCN_MAX_TPCNN
    assert FIGURES["kmax"][3] + 1 == 3                                # kmax: the workspace from n = 3 on
    assert DN.BIG == (257, 512) and len(DN.MANY) == 300 and set(DN.MANY) == {0, 1, 2, 3, 4, 5}
    assert {n for n, u in DN.USED.items() if "big" in u} == {"k1", "wide3"}
    assert {n for n, u in DN.USED.items() if "many" in u} == {"k1", "et"}
    assert all({"edge", "g3", "g65"} <= set(u) for u in DN.USED.values()) and {n for n, u in DN.USED.items() if "nan" in u} == {"narrow", "deep"}
    assert set(DN.SEEDS) == {(n, l) for n, u in DN.USED.items() for l in u}


@pytest.mark.parametrize("name", list(DN.CONFIGS))
def test_config_loads_strictly_and_leaves_no_default(name):
    from eigentrajectory_amd.dmrgcn import SocialDMRGCN
    sd = DN.random_state(name)
    net = SocialDMRGCN(**DN.module_cfg(name))
    assert list(net.state_dict()) == list(sd) == list(DN.state_shapes(name))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    c = DN.CONFIGS[name]
    assert all(v.dtype == np.float32 for v in sd.values())
    slopes = [float(v[0]) for k, v in sd.items() if DN.is_slope(k)]
    assert all(sd[k].shape == (1,) for k in sd if DN.is_slope(k)) and len(slopes) == 2 * c["st"] + 3 * c["tp"]
    assert len(set(slopes)) == len(slopes) and all(abs(a - 0.25) > 0.02 and a > 0.04 for a in slopes)
    assert all(np.abs(v).min() > 0 for k, v in sd.items() if k.endswith("bias"))
    for i in range(c["st"]):  # the two relations' weights differ
        assert np.abs(sd[f"st_dmrgcns.{i}.gcns.0.conv.weight"] - sd[f"st_dmrgcns.{i}.gcns.1.conv.weight"]).max() > 0.05
        assert np.abs(sd[f"st_dmrgcns.{i}.gcns.0.conv.bias"] - sd[f"st_dmrgcns.{i}.gcns.1.conv.bias"]).max() > 0.01
    assert ("st_dmrgcns.0.residual.0.weight" in sd) == (c["S"] != 1) and "tpcnns.0.residual.0.weight" in sd
    for other in DN.CONFIGS:  # no two configurations share a draw
        if other != name:
            assert not np.array_equal(DN.random_state(other)["tpcnns.0.gtacn.0.1.weight"], sd["tpcnns.0.gtacn.0.1.weight"])
    assert all(np.array_equal(v, DN.random_state(name)[k]) for k, v in sd.items())  # seeded


@pytest.mark.parametrize("name", list(DN.CONFIGS))
def test_float32_mode_is_within_a_quarter_of_the_tolerance(name):
    """the restatement in fp32 after the bin decision (dtype=np.float32: the same statements, the arithmetic's own error)
    against itself in fp64 on every scene of every layout the GPU file compares: within TOL / 4 of the largest entry.
    Measured: k1 edge 3.0e-7, g3 3.3e-7, g65 1.0e-7, big 1.8e-7, many 6.7e-7; narrow 1.9e-7, 1.3e-7, 1.5e-7, nan 1.6e-7;
    deep 2.5e-7, 1.3e-7, 2.1e-7, nan 2.1e-7; wide3 4.2e-7, 2.2e-7, 3.1e-7, big 3.9e-7; kmax 1.5e-6, 7.7e-7, 8.5e-7; et 3.7e-7, 2.0e-7,
    2.3e-7, many 4.1e-7"""
    sd, c = DN.random_state(name), DN.CONFIGS[name]
    kw = dict(n_stgcn=c["st"], n_tpcnn=c["tp"])
    for layout in DN.USED[name]:
        sizes, C_obs, nrm = DN.layout_inputs(name, layout)
        worst, scenes = 0.0, 0
        for _, _, n, v in DN.scenes_of(sizes, C_obs, nrm):
            o64, o32 = DN.forward(sd, v, **kw), DN.forward(sd, v, dtype=np.float32, **kw)
            assert o32.dtype == np.float32 and o64.dtype == np.float64 and o64.shape == (c["S"], c["k"], n)  # nothing promoted
            worst, scenes = max(worst, scale_err(o32, o64)), scenes + 1
        assert scenes == sum(1 for n in sizes if n)  # no scene left out
        print(f"dmrgcn {name} {layout}: float32 mode {worst:.2e} of the largest entry (bound {DN.TOL / 4:.1e})")
        assert worst <= DN.TOL / 4, (name, layout, worst)


def _dense_gcn(sd, pre, x, a, split=DN.SPLIT):
    """dmrgcn.py:66-68 and normalizer.py restated densely in fp64: all ten Laplacians I - D^-1/2 (A_b + I) D^-1/2 with
    row-sum degrees, the 1x1 convolution viewed as (bins, S), einsum('rbtwv,rbctv->ctw')"""
    Cin, K, n = x.shape
    eye = np.eye(n)
    Ls, xs = [], []
    for r in range(2):
        A = np.asarray(a[r], np.float64)                                   # (K, n, n)
        edges = [float(s) for s in split[r]] + [DN.LAST]
        Ab = np.stack([((A > edges[b]) & (A < edges[b + 1])).astype(np.float64) for b in range(len(split[r]))])
        At = Ab + eye
        dm = At.sum(-1) ** -0.5                                            # (5, K, n): row sums
        Ls.append(eye - dm[..., :, None] * At * dm[..., None, :])
        W = np.asarray(sd[f"{pre}.gcns.{r}.conv.weight"], np.float64)[:, :, 0, 0]
        xc = np.einsum("oc,ctv->otv", W, x) + np.asarray(sd[f"{pre}.gcns.{r}.conv.bias"], np.float64)[:, None, None]
        xs.append(xc.reshape(len(split[r]), -1, K, n))
    return np.einsum("rbtwv,rbctv->ctw", np.stack(Ls), np.stack(xs))


@pytest.mark.parametrize("name,n", [("deep", 12), ("narrow", 7), ("k1", 5)])
def test_a_given_a_is_read_as_it_is(name, n):
    """the restatement's given-a path (masked sums, never a Laplacian) against the dense form on an a no bridge builds:
    asymmetric, diagonal entries inside a bin, entries exactly on split values, a row with no neighbour -- in the first
    block (C_in = 1) and, at deep, a later one (C_in = S); to 1e-12.  Each property moves the result."""
    sd, c = DN.random_state(name), DN.CONFIGS[name]
    sd64 = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    C_obs, nrm = DN.synthetic_split((n,), 4, c["k"])
    v = DN.scene_input(C_obs, nrm, 0, n)
    K = c["k"] + 2
    a = DN.odd_adjacency(v)
    assert a.dtype == np.float32 and a.shape == (2, K, n, n)
    eye = np.eye(n, dtype=bool)
    for r in range(2):
        inbin = DN.bins(a[r], DN.SPLIT[r]).any(axis=0)                      # (K, n, n)
        assert (inbin != np.swapaxes(inbin, 1, 2)).any() and not np.array_equal(a[r], np.swapaxes(a[r], 1, 2))  # asymmetric
        assert inbin[:, eye].any() and not inbin[:, eye].all()             # some diagonal entries inside a bin
        assert any(((a[r] == np.float32(s)) & ~eye).any() for s in DN.SPLIT[r][1:])  # entries exactly on a split value ...
        assert not inbin[a[r] == np.float32(DN.SPLIT[r][1])].any()         # ... which are in no bin
        assert not inbin[:, 1, :].any() and inbin[:, 0, :].any()           # row 1 has no neighbour in any bin
    x0 = v.astype(np.float64)[None]
    blocks = [("st_dmrgcns.0", x0)]
    if c["st"] > 1:
        blocks.append(("st_dmrgcns.1", np.random.default_rng(5).normal(0, 1, (c["S"], K, n))))
    for pre, x in blocks:
        got = DN.gcn(sd64, pre, x, DN.v_rel(v), v, a)
        ref = _dense_gcn(sd, pre, x, a)
        assert got.shape == ref.shape == (c["S"], K, n)
        err = scale_err(got, ref)
        print(f"dmrgcn {name} {pre} given a, n = {n}: {err:.2e} from the dense form")
        assert err <= 1e-12, (name, pre, err)
        nodiag = a.copy()
        nodiag[:, :, eye] = 0
        assert scale_err(_dense_gcn(sd, pre, x, nodiag), ref) > 1e-3       # the diagonal is counted
        assert scale_err(_dense_gcn(sd, pre, x, np.swapaxes(a, 2, 3)), ref) > 1e-3  # rows are w, columns v
        assert scale_err(_dense_gcn(sd, pre, x, DN.adjacency(v)), ref) > 1e-3
        own = DN.gcn(sd64, pre, x, DN.v_rel(v), v)                          # the bridge's a, formed or given: the same bits
        assert np.array_equal(own, DN.gcn(sd64, pre, x, DN.v_rel(v), v, DN.adjacency(v)))
    kw = dict(n_stgcn=c["st"], n_tpcnn=c["tp"])
    assert scale_err(DN.forward(sd, v, a, **kw), DN.forward(sd, v, **kw)) > 1e-3


def test_one_step_outside_every_limit_is_refused_on_the_host():
    """the refusals test_arguments_are_validated_on_the_host leaves out: k = 0 and 33, S = 0, no and nine tpcnn blocks, no
    st block, seq_len one short, kernel_size 5, a split value that is negative, NaN or >= 1e10; the accepted side of each
    limit is a member of DN.CONFIGS.  Both entry points, before any launch; the workspace size of each is 0"""
    from eigentrajectory_amd import _lib
    lib = _lib.lib()
    UNSUPPORTED = H.defines()["ET_ERR_UNSUPPORTED"]

    def split_with(r, b, val):
        p = _params()
        p.split[r][b] = val
        return p

    bad = {"k = 0": _params(pred_seq_len=0, seq_len=2), "k = 33": _params(pred_seq_len=33, seq_len=35),
           "S = 0": _params(output_feat=0), "n_stgcn = 0": _params(n_stgcn=0), "n_tpcnn = 0": _params(n_tpcnn=0),
           "n_tpcnn = 9": _params(n_tpcnn=_lib.DMRGCN_MAX_TPCNN + 1), "seq_len = k + 1": _params(seq_len=7),
           "kernel_size = 5": _params(kernel_size=5), "negative split": split_with(0, 0, -0.125),
           "NaN split": split_with(1, 2, float("nan")), "NaN first split": split_with(0, 0, float("nan")),
           "split at 1e10": split_with(1, 4, 1e10), "split above 1e10": split_with(0, 4, 2e10)}
    for what, p in bad.items():
        assert lib.et_dmrgcn_forward_graph(C.byref(p), 8, 8, 3, 8, None, 0, None) == UNSUPPORTED, what
        assert lib.et_dmrgcn_forward_scenes(C.byref(p), 8, 8, 3, None, 0, 8, None, None, 0, None) == UNSUPPORTED, what
        assert int(lib.et_dmrgcn_workspace_bytes(C.byref(p), 5000, 100)) == 0, what
    for name in DN.CONFIGS:  # the accepted side: N = 0 is answered ET_OK once the parameters have passed
        assert lib.et_dmrgcn_forward_graph(C.byref(_cfg_params(name)), None, None, 0, None, None, 0, None) == 0, name
    assert lib.et_dmrgcn_forward_graph(C.byref(split_with(1, 4, 9.99e9)), None, None, 0, None, None, 0, None) == 0
