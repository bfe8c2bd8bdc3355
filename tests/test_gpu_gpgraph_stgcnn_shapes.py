"""csrc/et_gpgraph_stgcnn.hip (with the per-time-row branch of csrc/et_stgcnn_core.inl and the CH = 1 instantiation of
csrc/et_gpgraph_core.inl) away from the two members of its family tests/test_gpu_gpgraph_stgcnn.py runs (1 st_gcn / 5 tpcnns /
S 20 / k 6 and 2 / 3 / 12 / 6, both T = 8, no scene above 130, v_rel always v_abs itself): the configurations of
tests/_gpgraph_stgcnn_np.py: CONFIGS, each chosen for a path -- et (the ET shape with seeded weights, as control), tp1 (tpcnns[0]
straight into tpcnn_ouput, q stays 2 K), s1 (S = 1: the first block's residual is the identity, read from u; T = 3; one output
number per pedestrian; no scene ever leaves LDS), j17 (a second st_gcn contracting J = 17 rows: the second group of 16 holds
the ones row alone; one pass of the tpcnn residual loop), deep (eight st_gcns and eight tpcnns, the limits; J = 8), wide (S =
64: J = 65, five groups) and max (T = 34, S k = 2048: the largest mix product and its 49152 bytes of LDS; scenes of at most
17) -- on the scene layouts edge (1, 2, 3, an empty scene, L - 1, L, L + 1, 2 around the configuration's own LDS limit L),
257 and 512 pedestrians (the strided per-pedestrian loops of the grouping, the limit), 300 scenes in one call (the strided
scene_sq_before, the binary search of the mix, a grid of 900), graph-form scenes of 3, 13 and L + 1 with the bridge's v_rel
and with a v_rel that no bridge builds, plus the two extreme thresholds, a NaN coefficient, bit-equalities, the workspace
(its size restated, nothing written outside it or outside the outputs, no dependence on what it held), the C entry's "does
not fit the stacks" case and the refusals one step outside every limit.

Every comparison goes through tests/test_gpu_gpgraph_stgcnn.check: distances within TOL_D = 1e-6 of the largest, indices
equal (no pair is undecided: tests/test_gpgraph_stgcnn_cpu.py), the fp32 bounds on the inputs of passes 1 and 2 (ratios <= 1),
the output within TOL = 1e-5 of the largest entry of the restatement fed the device's own fp32 inputs of passes 1 and 2; no
scene is left out.  The scenes form returns the v it formed as pass 0's input: its C_obs rows are checked bit for bit and its
obs_ori rows within 2 ulp of the numpy fp32 value, and the restatement is fed THAT v.  A threshold belongs to its case and
is written into the module in place before the launch.  The recorded outputs of the reference's own GPGraph (fixture G34)
are compared with directly where its fp32 run is within 1e-6 of its fp64 run, the ties are robust and the device's tie pattern
is the reference's.

Measured on the MI355X (DESIGN section 4 "GP-Graph-STGCNN", "Across the family"), per configuration over its layouts: largest
distance error; largest ratios error / bound of v' and of the means; largest output error against the restatement; against
G34's recorded output directly; and, from the CPU (tests/test_gpgraph_stgcnn_cpu.py), the restatement's own fp32 mode against
its fp64 mode on the same scenes:
  et    1.5e-7   0.26  0.32   4.2e-7   4.5e-7   3.1e-7
  tp1   8.3e-8   0.20  0.28   4.4e-7   4.8e-7   4.5e-7
  s1    1.4e-7   0.23  0.32   1.8e-7   8.4e-8   1.6e-7
  j17   1.2e-7   0.18  0.24   3.1e-7   2.5e-7   2.1e-7
  deep  1.2e-7   0.14  0.21   2.9e-7   3.5e-7   3.0e-7
  wide  9.7e-8   0.18  0.28   9.2e-7   8.0e-7   4.6e-7
  max   1.6e-7   0.26  0.34   2.4e-6   2.1e-6   5.1e-7
All 26 recorded cases are compared with the reference's output directly; every bit-equality holds and every guard band is
intact; the slowest test takes 0.76 s (300 scenes at et).  The output error is within 2 x of the CPU's fp32 figure except at max,
4.7 x: the mix kernel adds the 3 S k = 6144 products of an output in sequence in one lane, numpy blockwise; that sequential
fp32 sum alone, on the CPU with everything else in fp64, gives 1.7e-6 on the scene of 3 (device 2.1e-6).

What notices a kernel that is wrong in numbers only (four in-bounds variants of et_stgcnn_core.inl / et_gpgraph_core.inl, each
run once on the MI355X with this file and tests/test_gpu_gpgraph_stgcnn.py):
  (a) pass 0 of the graph form reads v_abs where g_rel belongs -- test_graph_form_at_every_config fails at all seven
      configurations (the odd v_rel); the older file passes;
  (c) the column sums of sig run over the first 256 rows only -- test_large_scenes[s1-limit], [deep-limit] and
      test_threshold_extremes[s1] (G = n at 300) fail, through the bound on v' (ratios 37 to 2252); the three scenes of 257 do
      NOT notice the one missing row (v' = (v - s) + s hides s up to rounding); the older file passes;
  (d) block 0's identity residual reads time row 0 (xin[w]) instead of xin[it] -- the scene form, the graph form, both large
      scenes, the 300 scenes and the extremes fail at s1; the older file passes;
  (b) the second-stage product of the per-row branch reads q with the first layer's row stride (t 2 n for t J n) -- the scene
      and graph forms at j17, deep, wide and max, test_large_scenes[j17-big] and [deep-limit], test_threshold_extremes[j17] and
      the NaN test fail; the older file's two-layer case (test_generic_loop_counts) sees this one as well.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from . import _golden as G
from . import _gpgraph_stgcnn_np as GS
from ._gpu_common import *  # noqa: F401,F403 -- fixtures (dev, ops) and helpers
from .test_gpu_gpgraph_stgcnn import check, run_graph, same_ties
from .test_gpu_sgcn_shapes import guarded, guards_intact, reversed_rows

pytestmark = pytest.mark.gpu
Z34 = G.load("g34_gpgraph_stgcnn_family.npz")
_NETS = {}
FIGS = {}  # configuration -> the largest figures over everything this session compared (printed by every test that adds to them)


def net(dev, name):
    """CONFIGS[name] with its seeded weights on the device, built once per session; only th is ever edited, in place"""
    if name not in _NETS:
        _NETS[name] = GS.module(name, dev).eval()
    return _NETS[name]


def note(name, fig, direct=None):
    f = FIGS.setdefault(name, {"dist_err": 0.0, "vprime": 0.0, "means": 0.0, "out_err": 0.0, "direct": 0.0, "scenes": 0})
    if fig is not None:
        for key in ("dist_err", "vprime", "means", "out_err"):
            f[key] = max(f[key], fig[key])
        f["scenes"] += 1
    if direct is not None:
        f["direct"] = max(f["direct"], direct)


def report(name, t0):
    print(f"gpgraph-stgcnn shapes {name}: " + ", ".join(f"{k} {v:.2e}" if isinstance(v, float) else f"{k} {v}"
                                                         for k, v in FIGS.get(name, {}).items()) + f"; {time.time() - t0:.2f} s")


def check_scene(name, th, v_abs, got, v_rel=None):
    fig = check(GS.with_threshold(name, th), v_abs, got, th=float(th), v_rel=v_rel)
    assert fig["margin"] > GS.BAND_D, fig  # no pair is undecided, so check() did compare the indices
    note(name, fig)
    return fig


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def run_scenes(ops, m, name, sizes, C_obs, nrm, th):
    """one launch of the scenes form under the case's threshold, with the details -> (C_pred_refine (k, N, S), {scene: dict(out
    (S, k, n), indices, dist, gin)}); the call without the details gives the same bits"""
    dev = next(m.parameters()).device
    n_st, n_tp, S, k = GS.CONFIGS[name]
    GS.set_threshold(m, th)
    Cd, nd = T(C_obs, dev), T(nrm, dev)
    out, det = ops.gpgraph_stgcnn_forward_scenes(m, Cd, nd, scene_sizes=list(sizes), want_details=True)
    plain = ops.gpgraph_stgcnn_forward_scenes(m, Cd, nd, scene_sizes=list(sizes))
    out = N_(out)
    assert out.shape == (k, sum(sizes), S) and np.array_equal(bits(N_(plain)), bits(out))  # (as bits: a NaN equals itself)
    scenes = GS.unpack(sizes, k + 2, N_(det["dist"]), N_(det["graph_inputs"]), N_(det["group_index"]), N_(det["n_groups"]))
    lo = 0
    for s, n in enumerate(sizes):
        if n:
            scenes[s]["out"] = out[:, lo:lo + n].transpose(2, 0, 1)
            scenes[s]["lo"] = lo
        lo += n
    return out, scenes


def check_launch(name, sizes, C_obs, nrm, th, scenes):
    """every non-empty scene of one launch: the v the kernels formed against tests/_sgcn_np.scene_input (the C_obs rows bit for
    bit, the obs_ori rows within 2 ulp at the scale of the scene's positions: both are a fp32 mean in their own summation
    order, subtracted once), then check() with THAT v"""
    k = C_obs.shape[0]
    for s, lo, n, v in GS.scenes_of(sizes, C_obs, nrm):
        got = scenes[s]
        dv = got["gin"][0]
        assert np.array_equal(dv[:k], v[:k]), (name, s)
        ulp = np.spacing(np.abs(nrm[:2, lo:lo + n]).max().astype(np.float32))
        assert np.abs(dv[k:].astype(np.float64) - v[k:]).max() <= 2 * ulp, (name, s)
        assert np.isfinite(got["out"]).all()
        check_scene(name, th, dv, got)
    assert set(scenes) == {s for s, n in enumerate(sizes) if n}


@pytest.mark.parametrize("name", list(GS.CONFIGS))
def test_scene_form_at_every_config(dev, ops, name):
    """one launch on the edge layout with the details: every scene against the restatement, the packed details unpacked with
    the configuration's own T; the workspace size is the restated one with sum_n2 on either side of the LDS switch"""
    from eigentrajectory_amd import _lib as L
    t0 = time.time()
    m, cfg = net(dev, name), GS.CONFIGS[name]
    sizes, C_obs, nrm, th = GS.layout_case(name, "edge")
    out, scenes = run_scenes(ops, m, name, sizes, C_obs, nrm, th)
    check_launch(name, sizes, C_obs, nrm, th, scenes)
    params, _ = m.et_params()
    lim = GS.lds_max_n(*cfg)
    for N, n2, S in ((1, 1, 1), (lim, lim * lim, 1), (lim + 1, (lim + 1) ** 2, 1), (lim + 1, (lim + 1) ** 2 - 1, 1),
                     (1000, 12345, 300), (sum(sizes), sum(n * n for n in sizes), len(sizes))):
        assert L.lib().et_gpgraph_stgcnn_workspace_bytes(C.byref(params), N, n2, S) == 4 * GS.workspace_floats(cfg, N, n2, S), \
            (name, N, n2, S)
    report(name, t0)


@pytest.mark.parametrize("name", list(GS.CONFIGS))
def test_graph_form_at_every_config(dev, ops, name):
    """scenes of 3, 13 and L + 1 through m(v_abs, v_rel) with the bridge's v_rel = v_abs; on 3 and 13 also a seeded v_rel that
    no bridge builds, which must change the output; the recorded outputs of fixture G34 compared with directly"""
    t0 = time.time()
    m = net(dev, name)
    outs, direct = {}, []
    for which, odd in GS.graph_cases(name):
        va, vr, th = GS.graph_case(name, which, odd)
        GS.set_threshold(m, th)
        got = run_graph(ops, m, dev, va, vr if odd else None)
        assert got["out"].shape == (GS.CONFIGS[name][2], GS.CONFIGS[name][3], va.shape[1])
        fig = check_scene(name, th, va, got, vr if odd else None)
        if which == "gL1" or (name == "max" and which == "g3"):
            assert fig["n_groups"] <= GS.lds_max_n(*GS.CONFIGS[name]) < va.shape[1]  # pass 1 in LDS, passes 0 and 2 not
        outs[which, odd] = got["out"]
        tag = f"{name}.{which}{'odd' if odd else ''}"
        if f"{tag}.out" in Z34.files:
            assert np.array_equal(got["indices"], Z34[f"{tag}.indices"]) and GS.rel_err(got["dist"], Z34[f"{tag}.dist"]) <= GS.TOL_D
            if float(Z34[f"{tag}.cond"]) <= GS.COND and bool(Z34[f"{tag}.ties_robust"]) and \
                    same_ties(got["gin"], [Z34[f"{tag}.v_rel"], Z34[f"{tag}.v_group"], Z34[f"{tag}.v_intra"]]):
                err = GS.rel_err(got["out"], Z34[f"{tag}.out"])
                print(f"{tag}: against the reference's output directly {err:.3e}")
                assert err <= GS.TOL, (tag, err)
                note(name, None, err)
                direct.append(tag)
    for which in GS.ODD:
        if (which, True) in outs:
            assert GS.rel_err(outs[which, True], outs[which, False]) > 1e-3, (name, which)
    assert f"{name}.g3" in direct, direct
    print(f"gpgraph-stgcnn shapes {name}: compared with the reference's output directly: {direct}")
    report(name, t0)


@pytest.mark.parametrize("name,layout", [(n, l) for n, used in GS.USED.items() for l in used if l in ("big", "limit")])
def test_large_scenes(dev, ops, name, layout):
    """one scene of 257 and one of 512 = ET_SGCN_MAX_N pedestrians, in both forms: the labels, hit, cnt, the column sums and
    the ranks stride by the workgroup; the graph form is fed the v the scenes form made and gives the same bits.  At 512 the
    scene also runs between two small ones, (3, 512, 4): bit-equal to the scene alone, the small ones against the restatement"""
    t0 = time.time()
    m = net(dev, name)
    sizes, C_obs, nrm, th = GS.layout_case(name, layout)
    out, scenes = run_scenes(ops, m, name, sizes, C_obs, nrm, th)
    check_launch(name, sizes, C_obs, nrm, th, scenes)
    one = ops.gpgraph_stgcnn_forward_scenes(m, T(C_obs, dev), T(nrm, dev))  # no scene list: one scene of N rows
    assert np.array_equal(N_(one), out)
    got = run_graph(ops, m, dev, scenes[0]["gin"][0])
    for key in ("out", "indices", "dist"):
        assert np.array_equal(got[key], scenes[0][key]), key
    assert all(np.array_equal(a, b) for a, b in zip(got["gin"], scenes[0]["gin"]))
    if layout == "limit":
        sizes3, C3, n3, th3 = GS.around_case(name)
        out3, scenes3 = run_scenes(ops, m, name, sizes3, C3, n3, th3)
        assert np.array_equal(out3[:, 3:3 + sizes[0]], out)
        for key in ("indices", "dist"):
            assert np.array_equal(scenes3[1][key], scenes[0][key])
        small = {s: scenes3[s] for s in (0, 2)}
        keep = np.r_[0:3, 3 + sizes[0]:sum(sizes3)]
        check_launch(name, (3, 4), np.ascontiguousarray(C3[:, keep]), np.ascontiguousarray(n3[:, keep]), th3,
                     {0: small[0], 1: small[2]})
    report(name, t0)


@pytest.mark.parametrize("name", [n for n, used in GS.USED.items() if "many" in used])
def test_many_scenes(dev, ops, name):
    """300 scenes of 1, 2, 3, ... in one call: more than the 256 lanes that sum the squared sizes of the scenes before a scene,
    a binary search over 300 offsets in the mix, 900 virtual scenes.  Every scene against the restatement; the last scene
    alone gives the same bits"""
    t0 = time.time()
    m = net(dev, name)
    sizes, C_obs, nrm, th = GS.layout_case(name, "many")
    assert len(sizes) > 256
    out, scenes = run_scenes(ops, m, name, sizes, C_obs, nrm, th)
    check_launch(name, sizes, C_obs, nrm, th, scenes)
    lo, n = scenes[299]["lo"], sizes[299]
    alone, sa = run_scenes(ops, m, name, (n,), np.ascontiguousarray(C_obs[:, lo:]), np.ascontiguousarray(nrm[:, lo:]), th)
    assert np.array_equal(alone, out[:, lo:]) and np.array_equal(sa[0]["dist"], scenes[299]["dist"])
    assert all(np.array_equal(a, b) for a, b in zip(sa[0]["gin"], scenes[299]["gin"]))
    report(name, t0)


@pytest.mark.parametrize("name", list(GS.EXTREMES))
def test_threshold_extremes(dev, ops, name):
    """th below every pair distance: G = n, the same-group matrix is I and the intra-group Laplacian I - I = 0 (the
    restatement's, which the output is compared with); th above every one: G = 1, pass 1 runs on a single node"""
    t0 = time.time()
    m = net(dev, name)
    T_ = GS.CONFIGS[name][3] + 2
    outs = []
    for above in (False, True):
        sizes, C_obs, nrm, th = GS.extreme_case(name, above)
        (n,) = sizes
        out, scenes = run_scenes(ops, m, name, sizes, C_obs, nrm, th)
        assert scenes[0]["indices"].tolist() == ([0] * n if above else list(range(n)))
        assert scenes[0]["gin"][1].shape == ((T_, 1) if above else (T_, n))
        check_launch(name, sizes, C_obs, nrm, th, scenes)
        outs.append(out)
    assert GS.rel_err(outs[0], outs[1]) > 1e-3
    report(name, t0)


@pytest.mark.parametrize("name", ["j17", "s1"])
def test_bit_equalities(dev, ops, name):
    """on the edge layout: a second run, the scenes in reversed order, every scene alone in the graph form fed the v the
    scenes form made (identical inputs, so identical tie patterns), and -- inside run_scenes -- the plain call against the call
    with details, all give the same bits"""
    m = net(dev, name)
    sizes, C_obs, nrm, th = GS.layout_case(name, "edge")
    out, scenes = run_scenes(ops, m, name, sizes, C_obs, nrm, th)
    again, scenes2 = run_scenes(ops, m, name, sizes, C_obs, nrm, th)
    assert np.array_equal(again, out)
    order = reversed_rows(sizes)
    rout, rscenes = run_scenes(ops, m, name, sizes[::-1], np.ascontiguousarray(C_obs[:, order]),
                               np.ascontiguousarray(nrm[:, order]), th)
    assert np.array_equal(rout, out[:, order])
    last = len(sizes) - 1
    for s, got in scenes.items():
        for other in (scenes2[s], rscenes[last - s]):
            assert np.array_equal(other["dist"], got["dist"]) and np.array_equal(other["indices"], got["indices"])
            assert all(np.array_equal(a, b) for a, b in zip(other["gin"], got["gin"]))
        graph = run_graph(ops, m, dev, got["gin"][0])
        for key in ("out", "indices", "dist"):
            assert np.array_equal(graph[key], got[key]), (s, key)
        assert all(np.array_equal(a, b) for a, b in zip(graph["gin"], got["gin"]))


def c_entry(dev, m, name, sizes, C_obs, nrm, th, sum_n2=None, fill=None):
    """et_gpgraph_stgcnn_forward_scenes called directly, with the workspace (exactly et_gpgraph_stgcnn_workspace_bytes of the
    honest sum of squares), C_pred_refine, group_index, dist and graph_inputs each inside a larger tensor of ``fill`` bytes
    (None: plain zero-filled buffers).  ``sum_n2``: what the call is told (default: the honest value)
    -> dict(out (k, N, S), gi, dist, gin, ws: views on the device, intact: the guards are as they were)"""
    from eigentrajectory_amd import _lib as L
    n_st, n_tp, S, k = GS.CONFIGS[name]
    GS.set_threshold(m, th)
    params, _ = m.et_params()
    N, honest = int(sum(sizes)), int(sum(n * n for n in sizes))
    nbytes = L.lib().et_gpgraph_stgcnn_workspace_bytes(C.byref(params), N, honest, len(sizes))
    assert nbytes == 4 * GS.workspace_floats(GS.CONFIGS[name], N, honest, len(sizes))
    want = dict(ws=nbytes, out=4 * k * N * S, gi=4 * N, dist=4 * honest, gin=4 * 3 * (k + 2) * N)
    whole, part = {}, {}
    for key, nb in want.items():
        if fill is None:
            part[key] = torch.zeros((nb,), device=dev, dtype=torch.uint8)
        else:
            whole[key], part[key] = guarded(nb, fill, dev)
        assert part[key].data_ptr() % 16 == 0
    Cd, nd = T(C_obs, dev), T(nrm, dev)
    off = T(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), dev)
    L.call("et_gpgraph_stgcnn_forward_scenes", C.byref(params), L.ptr(Cd), L.ptr(nd), N, L.ptr(off), len(sizes),
           honest if sum_n2 is None else sum_n2, int(max(sizes)), L.ptr(part["out"]), L.ptr(part["gi"]), L.ptr(part["dist"]),
           L.ptr(part["gin"]), L.ptr(part["ws"]), nbytes, L.stream(dev))
    torch.cuda.synchronize(dev)
    res = {key: part[key].view(torch.int32 if key == "gi" else torch.float32) for key in part}
    res["out"] = res["out"].view(k, N, S)
    res["intact"] = all(guards_intact(whole[key], want[key], fill) for key in whole)
    return res


@pytest.mark.parametrize("name,layout", [("et", "edge"), ("wide", "edge"), ("s1", "big")])
def test_only_the_workspace_and_the_outputs_are_written(dev, ops, name, layout):
    """the C entry with the workspace and every output each inside a larger tensor: the guard bands stay as they were, and
    buffers of 0xFF bytes (NaN bit patterns) and of zeros give the bits ops.gpgraph_stgcnn_forward_scenes gives; no entry of
    the output keeps the fill"""
    m = net(dev, name)
    sizes, C_obs, nrm, th = GS.layout_case(name, layout)
    out, scenes = run_scenes(ops, m, name, sizes, C_obs, nrm, th)
    assert np.isfinite(out).all() and (out != 0).all()
    for fill in (0xFF, 0x00):
        got = c_entry(dev, m, name, sizes, C_obs, nrm, th, fill=fill)
        assert got["intact"], (name, fill)
        assert np.array_equal(N_(got["out"]), out), (name, fill)
        assert not bool((got["out"].view(torch.int32) == (-1 if fill else 0)).any())
        mine = GS.unpack(sizes, GS.CONFIGS[name][3] + 2, N_(got["dist"]), N_(got["gin"]), N_(got["gi"]),
                         [int(scenes[s]["indices"].max()) + 1 if s in scenes else 0 for s in range(len(sizes))])
        for s, ref in scenes.items():
            assert np.array_equal(mine[s]["dist"], ref["dist"]) and np.array_equal(mine[s]["indices"], ref["indices"])
            assert all(np.array_equal(a, b) for a, b in zip(mine[s]["gin"], ref["gin"]))


def test_scenes_that_do_not_fit_the_stacks(dev, ops):
    """et on the edge layout with sum_n2 one short of the scenes' squared sizes (the buffers sized for the honest value): the
    last scene's stack would pass the end, so its rows come back NaN; every scene before it is bit-equal to the full call and
    nothing outside the buffers is written"""
    m = net(dev, "et")
    sizes, C_obs, nrm, th = GS.layout_case("et", "edge")
    out, _ = run_scenes(ops, m, "et", sizes, C_obs, nrm, th)
    assert np.isfinite(out).all()
    honest = sum(n * n for n in sizes)
    got = c_entry(dev, m, "et", sizes, C_obs, nrm, th, sum_n2=honest - 1, fill=0xA5)
    z = N_(got["out"])
    last = sizes[-1]
    assert got["intact"] and last > 0
    assert np.isnan(z[:, -last:]).all() and np.array_equal(z[:, :-last], out[:, :-last])


def test_one_step_outside_every_limit_is_refused(dev, ops):
    """S = 65, k = 33, nine st_gcns, nine tpcnns: each constructs, its workspace size is 0 and the C entry answers
    ET_ERR_UNSUPPORTED (status 3) before any launch; the device answers a good call bit for bit afterwards"""
    from eigentrajectory_amd import _lib as L
    from eigentrajectory_amd.gpgraph import GPGraph
    from eigentrajectory_amd.stgcnn import SocialSTGCNN
    from . import _stgcnn_np as ST
    m = net(dev, "j17")
    va, vr, th = GS.graph_case("j17", "g3")
    GS.set_threshold(m, th)
    a = T(va[None, None], dev)
    good, _ = m(a, a)
    assert torch.isfinite(good).all()
    n_st, n_tp, S, k = GS.CONFIGS["j17"]
    for cfg in ((n_st, n_tp, 65, k), (n_st, n_tp, S, 33), (9, n_tp, S, k), (n_st, 9, S, k)):
        base = SocialSTGCNN(graph_per_time_row=True, **ST.module_kw(*cfg))
        bad = GPGraph(base, in_channels=1, out_channels=cfg[2], obs_seq_len=cfg[3] + 2, pred_seq_len=cfg[3]).to(dev).eval()
        params, _ = bad.et_params()
        assert L.lib().et_gpgraph_stgcnn_workspace_bytes(C.byref(params), 3, 9, 1) == 0, cfg
        v = torch.zeros((1, 1, cfg[3] + 2, 3), device=dev)
        out = torch.zeros((1, cfg[2], cfg[3], 3), device=dev)
        ws = torch.zeros((1 << 20,), device=dev, dtype=torch.uint8)
        with pytest.raises(L.ETLibraryError, match="status 3"):
            L.call("et_gpgraph_stgcnn_forward_graph", C.byref(params), L.ptr(v), L.ptr(v), 3, L.ptr(out), None, None, None,
                   L.ptr(ws), ws.numel(), L.stream(dev))
        with pytest.raises(L.ETLibraryError, match="status 3"):
            bad(v, v)
    assert torch.equal(m(a, a)[0], good)


def test_a_nan_stays_in_its_scene(dev, ops):
    """j17 on (9, 20, 5): a NaN coefficient of one pedestrian of the middle scene makes every output row of that scene NaN
    (its distances to everybody are NaN, so is every column sum of sig and with it v') and leaves the other scenes bit-equal"""
    t0 = time.time()
    m = net(dev, "j17")
    sizes, C_obs, nrm, th = GS.layout_case("j17", "nan")
    clean, scenes = run_scenes(ops, m, "j17", sizes, C_obs, nrm, th)
    check_launch("j17", sizes, C_obs, nrm, th, scenes)
    bad = C_obs.copy()
    bad[2, 9 + 11] = np.nan
    got, _ = run_scenes(ops, m, "j17", sizes, bad, nrm, th)
    assert np.isnan(got[:, 9:29]).all()
    keep = np.r_[0:9, 29:34]
    assert np.array_equal(got[:, keep], clean[:, keep]) and np.isfinite(clean).all()
    report("j17", t0)
