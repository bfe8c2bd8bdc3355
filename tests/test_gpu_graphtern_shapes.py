"""csrc/et_graphtern.hip away from the two members of its family tests/test_gpu_graphtern.py runs (k 6 / S 20 / 1 st_mrgcn / 6
epcnn and 6 / 12 / 2 / 3, both T = 8): the configurations of tests/_graphtern_np.py: CONFIGS, each chosen for a path (the
figures are asserted on the CPU, tests/test_graphtern_cpu.py) -- k1 (qpp at the floor of gt_dims_of, one row in the cpcn
plane so all three row taps of conv33_replicate clamp to it, S = 1, the first epcnn block straight into the last), k2s16
(S = 16: the identity residual of the last epcnn block; three st_mrgcn blocks), deep (four st_mrgcn and eight epcnn blocks,
the limits: four rotations of x / y / q), wide (qpp = k S = 384, a later block in chunks of 5 and 3 time rows: tq > 0 and a
ragged last chunk), kmax (k = 32, T = 34, chunks 30 and 4, the workspace from n = 3 on), tall (k = 32, S = 1: chunks
8,8,8,8,2) and et (the ET shape with seeded weights, as control) -- on the layouts edge (1, 2, 3, an empty scene, 63, 64, 65,
the configuration's own lds_max_n and lds_max_n + 1), big (257 and 512), many (300 scenes of 0 .. 5), graph-form scenes of
3, 13 and 65 with the bridge's rel and with a rel no bridge builds, plus bit-equalities, a NaN and an inf coefficient, guard
bands and the "fits nowhere" branch of graphtern_kernel.

Every comparison with the restatement goes through test_gpu_graphtern.py's _check_scenes (C_obs rows bit for bit, obs_ori
within 2 ulp, the output within TOL = 1e-5 of the largest entry of the fp64 restatement fed the device's graph_inputs, no
scene left out) or, in the graph form, the same bound against GN.forward(sd, u, rel) and against the reference's own
recorded output (tests/golden/g33_graphtern_family.npz).  The seeded weights and inputs meet one condition on the CPU: the
restatement's own float32 mode is within TOL / 4 of its fp64 mode on every network input compared here.

Measured on the MI355X (DESIGN §4 "Graph-TERN", "Across the family"), largest error over a configuration's layouts, of the
largest entry: k1 2.2e-6 (many: one output number per pedestrian; 7.4e-7 on big, 5.4e-7 on edge), k2s16 3.1e-7, deep 6.8e-7
(g3), wide 3.9e-7 (big), kmax 4.6e-7 (edge), tall 7.2e-7 (g3, the odd rel), et 6.8e-7 (many); against the reference's own
output on the g33 scenes at most 6.4e-7 (tall).  The restatement's float32 mode against its fp64 mode on the same inputs
(CPU): 1.3e-6 (many; 8.7e-7 elsewhere), 2.3e-7, 2.8e-7, 2.5e-7, 2.5e-7, 3.8e-7, 3.6e-7 -- the kernel is within 2.5 times what
numpy's fp32 is from fp64.  Every bit-equality holds, every guard band is intact, the NaN masks are the restatement's (all
40 columns of the scene, for a NaN and for an inf); the slowest test takes 0.32 s (many at et; the restatement, not the
launch).  No test here found the kernel wrong: et_graphtern.hip is unchanged.

What notices a kernel that is wrong in numbers only (three variants of et_graphtern.hip, each built once and run once on
the MI355X with both Graph-TERN files; none moves a write, changes a loop bound, an arena size or nt, and each reads only
entries the unchanged kernel has written by then):
  1 the 1x1 convolution reads q with the time-row stride of the first block, row `tq 8 + r J` instead of `(tq 4 + r) J` (no
    larger an offset, rows of the same chunk): equal wherever tq == 0 or J == 2.  Fails the scene and graph forms at wide,
    kmax and tall, big and both NaN cases at wide (nine tests); tests/test_gpu_graphtern.py passes.
  2 the last epcnn block's identity residual reads x transposed within its (k, 16) plane (`x[(o k + t) n + w]`): only S = 16
    takes that branch.  Fails the scene and graph forms at k2s16; tests/test_gpu_graphtern.py passes.
  3 GraphSrc forms rel from u (`u[t] - u[t-1]`, row 0 zero) instead of reading S_obs[:, 1]: equal for every S_obs a bridge
    builds.  Fails the graph form at all seven configurations, each at the odd rel of the scene of 3;
    tests/test_gpu_graphtern.py passes.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from . import _golden as G
from . import _graphtern_np as GN
from ._gpu_common import *  # noqa: F401,F403 -- fixtures (dev, ops) and helpers
from .test_gpu_graphtern import TOL, _check_scenes, scale_err
from .test_gpu_sgcn_shapes import guarded, guards_intact, reversed_rows

pytestmark = pytest.mark.gpu
G33 = G.load("g33_graphtern_family.npz")
_NETS, _SD = {}, {}
assert TOL == GN.TOL


def state(name):
    if name not in _SD:
        _SD[name] = GN.random_state(name)
    return _SD[name]


def net(dev, name):
    """CONFIGS[name] with its seeded weights on the device, built once per session; nothing edits it"""
    if name not in _NETS:
        from eigentrajectory_amd.graphtern import GraphTERNLight
        m = GraphTERNLight(**GN.module_cfg(name))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in state(name).items()}, strict=True)
        _NETS[name] = m.to(dev).eval()
    return _NETS[name]


def run_scenes(ops, m, C_obs, nrm, sizes):
    """-> the device's (C_pred_refine, graph_inputs) as numpy; the call without the details gives the same bits"""
    dev = next(m.parameters()).device
    Cd, nd = T(C_obs, dev), T(nrm, dev)
    out, det = ops.graphtern_forward_scenes(m, Cd, nd, scene_sizes=list(sizes), want_details=True)
    plain = ops.graphtern_forward_scenes(m, Cd, nd, scene_sizes=list(sizes))
    assert np.array_equal(N_(plain).view(np.int32), N_(out).view(np.int32))  # (as bits: a NaN equals itself)
    return N_(out), N_(det["graph_inputs"])


def check(ops, dev, name, layout):
    sizes, C_obs, nrm = GN.layout_inputs(name, layout)
    print(f"graphtern shapes {name} {layout}:", end=" ")
    out = _check_scenes(ops, net(dev, name), state(name), C_obs, nrm, list(sizes))
    c = GN.CONFIGS[name]
    assert out.shape == (c["k"], sum(sizes), c["S"]) and np.isfinite(out).all()
    return sizes, out


def ws_bytes(m, N, max_n):
    from eigentrajectory_amd import _lib as L
    p, _ = m.et_params()
    return int(L.lib().et_graphtern_workspace_bytes(C.byref(p), N, max_n))


@pytest.mark.parametrize("name", list(GN.CONFIGS))
def test_scene_form_at_every_config(dev, ops, name):
    """one launch on the edge layout: every non-empty scene within TOL, arenas in LDS and in the workspace in one call; the
    workspace size is the restated one on either side of the configuration's switch"""
    sizes, _ = check(ops, dev, name, "edge")
    m = net(dev, name)
    _, _, per, lim, _ = GN.config_dims(name)
    N = sum(sizes)
    assert min(n for n in sizes if n) <= lim < max(sizes)
    assert ws_bytes(m, N, lim) == GN.workspace_bytes(per, N, lim) == 0
    assert ws_bytes(m, N, lim + 1) == GN.workspace_bytes(per, N, lim + 1) == per * N * 4 > 0


def run_graph(ops, m, dev, u, rel):
    s_obs = T(np.stack([u, rel])[None, :, :, :, None], dev)
    out = m(s_obs)
    assert torch.equal(ops.graphtern_forward_graph(m, s_obs), out)
    return N_(out)[0]


@pytest.mark.parametrize("name", list(GN.CONFIGS))
def test_graph_form_at_every_config(dev, ops, name):
    """(1) the g33 scenes of 3 and 13 against the reference's own output; (2) scenes of 3 and 65 with the bridge's S_obs of
    the u the scene form reports, against the restatement; (3) the same u with GN.odd_rel (a non-zero first row, not the
    difference of u, ties u does not have), against the restatement given that rel: a kernel that formed rel from u would
    pass (2) and miss this; (4) the scene form on that one scene equals (2) bit for bit, as include/eigentraj.h promises.
    The scene of 65 runs from the workspace at every configuration but k1 and k2s16"""
    m, sd, c = net(dev, name), state(name), GN.CONFIGS[name]
    for n in GN.FIXTURE_SIZES:
        s_obs, ref = G33[f"{name}.s_obs{n}"], G33[f"{name}.net_out{n}"]
        out = run_graph(ops, m, dev, s_obs[0], s_obs[1])
        assert out.shape == ref.shape == (c["k"], n, c["S"])
        err = scale_err(out, ref)
        print(f"graphtern shapes {name} g33 n={n} against the reference: {err:.2e}")
        assert err <= TOL, (name, n, err)
    for layout in ("g3", "g65"):
        (n,), C_obs, nrm = GN.layout_inputs(name, layout)
        scene_out, u = run_scenes(ops, m, C_obs, nrm, (n,))
        assert u.shape == (c["k"] + 2, n) and np.array_equal(u[:c["k"]], C_obs)
        if layout == "g65":
            assert (ws_bytes(m, n, n) > 0) == (name not in ("k1", "k2s16"))
        outs = []
        for what, rel in (("bridge rel", GN.rel_of(u)), ("odd rel", GN.odd_rel(u))):
            out = run_graph(ops, m, dev, u, rel)
            assert out.shape == (c["k"], n, c["S"]) and np.isfinite(out).all()
            err = scale_err(out, GN.forward(sd, u, rel))
            print(f"graphtern shapes {name} {layout} {what}: {err:.2e}")
            assert err <= TOL, (name, layout, what, err)
            outs.append(out)
        assert np.array_equal(outs[0], scene_out), (name, layout)
        assert scale_err(outs[1], outs[0]) > 1e-3


@pytest.mark.parametrize("name", ["k1", "wide"])
def test_large_scenes(dev, ops, name):
    """scenes of 257 and 512 pedestrians in one call: scene_v's mean and every loop stride by the workgroup more than
    once, both arenas in the workspace, the second at an offset (kmax and tall are deliberately not run here: the
    O(T n^2) loops of one workgroup at T = 34)"""
    check(ops, dev, name, "big")


@pytest.mark.parametrize("name", ["k1", "et"])
def test_many_scenes_in_one_call(dev, ops, name):
    """300 scenes of 0 .. 5 pedestrians: more workgroups than the device runs at once, every sixth scene empty"""
    sizes, _ = check(ops, dev, name, "many")
    assert len(sizes) == 300 and sizes.count(0) == 50


@pytest.mark.parametrize("name", ["deep", "wide", "kmax"])
def test_bit_equalities(dev, ops, name):
    """at both block limits, with a chunked later block and at T = 34, on the edge layout (arenas in LDS and in the
    workspace): a scene alone equals the same scene inside the launch, a second run and the reversed scene order give the
    same bits"""
    m = net(dev, name)
    sizes, C_obs, nrm = GN.layout_inputs(name, "edge")
    lim = GN.config_dims(name)[3]
    assert min(n for n in sizes if n) <= lim < max(sizes)
    out, gin = run_scenes(ops, m, C_obs, nrm, sizes)
    again = run_scenes(ops, m, C_obs, nrm, sizes)
    assert np.isfinite(out).all() and np.array_equal(again[0], out) and np.array_equal(again[1], gin)
    lo = 0
    for n in sizes:
        if n:
            o1, g1 = run_scenes(ops, m, np.ascontiguousarray(C_obs[:, lo:lo + n]), np.ascontiguousarray(nrm[:, lo:lo + n]), [n])
            assert np.array_equal(o1, out[:, lo:lo + n]) and np.array_equal(g1, gin[:, lo:lo + n]), (lo, n)
        lo += n
    order = reversed_rows(sizes)
    rout, rgin = run_scenes(ops, m, np.ascontiguousarray(C_obs[:, order]), np.ascontiguousarray(nrm[:, order]), sizes[::-1])
    assert np.array_equal(rout, out[:, order]) and np.array_equal(rgin, gin[:, order])


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("name", ["deep", "wide"])
def test_a_nan_coefficient(dev, ops, name, value):
    """one NaN -- or inf -- coefficient of pedestrian 17 of the scene of 40 (the middle one of 4, 70, 40, 3, 9).  Every
    other scene is bit-equal to the run without it; inside the scene the device's output is NaN exactly where the fp64
    restatement's is, which is the whole scene (the poisoned distance is in every degree of its time row; asserted on the
    CPU too, tests/test_graphtern_cpu.py), and no entry is infinite"""
    m, sd = net(dev, name), state(name)
    sizes, clean = check(ops, dev, name, "nan")
    _, C_obs, nrm = GN.layout_inputs(name, "nan")
    s = sizes.index(40)
    lo = sum(sizes[:s])
    bad = C_obs.copy()
    bad[3, lo + 17] = value
    out, gin = run_scenes(ops, m, bad, nrm, sizes)
    keep = np.r_[0:lo, lo + 40:sum(sizes)]
    assert np.array_equal(out[:, keep], clean[:, keep])
    assert np.array_equal(gin[:, lo:lo + 40].view(np.int32)[:bad.shape[0]], bad[:, lo:lo + 40].view(np.int32))
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = GN.forward(sd, gin[:, lo:lo + 40])
    mine = out[:, lo:lo + 40]
    print(f"graphtern shapes {name} {value}: NaN in {int(np.isnan(mine).any(axis=(0, 2)).sum())} columns of the device's "
          f"output, {int(np.isnan(ref).any(axis=(0, 2)).sum())} of the restatement's")
    assert np.isnan(ref).all() and not np.isinf(mine).any()
    assert np.array_equal(np.isnan(mine), np.isnan(ref))


def c_entry(dev, m, C_obs, nrm, sizes, fill, ws_nbytes=None):
    """et_graphtern_forward_scenes called directly, with the workspace, C_pred_refine and graph_inputs each inside a larger
    tensor of ``fill`` bytes.  ``ws_nbytes``: the workspace handed over (default: et_graphtern_workspace_bytes, which is
    checked against the restated size; 0: a NULL workspace)
    -> dict(out (k, N, S), gin (T, N): float32 views on the device, intact: the guards are as they were)"""
    from eigentrajectory_amd import _lib as L
    params, _ = m.et_params()
    T_, k, S = params.seq_len, params.pred_seq_len, params.n_smpl
    N = int(sum(sizes))
    nbytes = int(L.lib().et_graphtern_workspace_bytes(C.byref(params), N, int(max(sizes))))
    assert nbytes == GN.workspace_bytes(GN.dims(k, S, params.n_epgcn)[2], N, int(max(sizes)))
    nbytes = nbytes if ws_nbytes is None else ws_nbytes
    want = dict(ws=nbytes, out=4 * k * N * S, gin=4 * T_ * N)
    whole, part = {}, {}
    for key, nb in want.items():
        whole[key], part[key] = guarded(nb, fill, dev)
        assert part[key].data_ptr() % 16 == 0
    Cd, nd = T(C_obs, dev), T(nrm, dev)
    off = T(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), dev)
    L.call("et_graphtern_forward_scenes", C.byref(params), L.ptr(Cd), L.ptr(nd), N, L.ptr(off), len(sizes),
           L.ptr(part["out"]), L.ptr(part["gin"]), L.ptr(part["ws"]) if nbytes else None, nbytes, L.stream(dev))
    torch.cuda.synchronize(dev)
    res = {"out": part["out"].view(torch.float32).view(k, N, S), "gin": part["gin"].view(torch.float32).view(T_, N)}
    res["intact"] = all(guards_intact(whole[key], want[key], fill) for key in whole)
    return res


@pytest.mark.parametrize("name", ["wide", "kmax"])
def test_only_the_outputs_and_the_workspace_are_written(dev, ops, name):
    """the C entry on the edge layout with the workspace (exactly et_graphtern_workspace_bytes), C_pred_refine and
    graph_inputs each inside a larger tensor: the guard bands stay as they were; buffers of 0xFF bytes (NaN) and of zeros
    give the bits ops.graphtern_forward_scenes gives -- nothing depends on what the workspace held -- and no output entry
    keeps the fill"""
    m = net(dev, name)
    sizes, C_obs, nrm = GN.layout_inputs(name, "edge")
    out, gin = run_scenes(ops, m, C_obs, nrm, sizes)
    assert np.isfinite(out).all() and (out != 0).all() and np.isfinite(gin).all()
    for fill in (0xFF, 0x00):
        got = c_entry(dev, m, C_obs, nrm, sizes, fill)
        assert got["intact"], (name, fill)
        assert np.array_equal(N_(got["out"]), out) and np.array_equal(N_(got["gin"]), gin), (name, fill)
        assert not bool((got["out"].view(torch.int32) == (-1 if fill else 0)).any()), (name, fill)


@pytest.mark.parametrize("case", ["short", "null"])
def test_scenes_the_c_entry_does_not_compute(dev, ops, case):
    """the "fits nowhere" branch of graphtern_kernel at k1 (69 pedestrians fit LDS), ET_OK from the launch.  short: scenes
    of 3, 80, 5, 90, 2 and a workspace that holds every row before the scene of 90 and all of its rows but one float: the
    scenes of 3, 5, 2 (LDS) and of 80 (its rows end inside the workspace) equal the full run bit for bit, the scene of 90 is
    NaN in the output and in graph_inputs.  null: scenes of 2, 70, 3 and no workspace at all: the scene of 70 is NaN, the
    others are computed.  Written over zero-filled buffers whose guard bands stay intact; the next call on the device
    gives the full run's bits again"""
    m = net(dev, "k1")
    _, _, per, lim, _ = GN.config_dims("k1")
    assert lim == 69
    sizes, left, ws_nbytes = ((3, 80, 5, 90, 2), 3, 4 * (per * 178 - 1)) if case == "short" else ((2, 70, 3), 1, 0)
    C_obs, nrm = GN.synthetic_split(sizes, 5, 1)
    full, full_gin = run_scenes(ops, m, C_obs, nrm, sizes)
    assert np.isfinite(full).all()
    got = c_entry(dev, m, C_obs, nrm, sizes, 0x00, ws_nbytes=ws_nbytes)
    out, gin = N_(got["out"]), N_(got["gin"])
    assert got["intact"]
    lo = sum(sizes[:left])
    nan_cols = np.r_[lo:lo + sizes[left]]
    done = np.setdiff1d(np.arange(sum(sizes)), nan_cols)
    assert np.array_equal(out[:, done], full[:, done]) and np.array_equal(gin[:, done], full_gin[:, done])
    assert np.isnan(out[:, nan_cols]).all() and np.isnan(gin[:, nan_cols]).all()
    again = run_scenes(ops, m, C_obs, nrm, sizes)
    assert np.array_equal(again[0], full) and np.array_equal(again[1], full_gin)
