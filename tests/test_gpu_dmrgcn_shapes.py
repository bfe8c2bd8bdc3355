"""csrc/et_dmrgcn.hip away from the two members of its family tests/test_gpu_dmrgcn.py runs (k 6 / S 20 / 1 st / 4 tpcnn and
6 / 12 / 2 / 2, both K = 8): the configurations of tests/_dmrgcn_np.py: CONFIGS, each chosen for a path (the figures are
asserted on the CPU, tests/test_dmrgcn_cpu.py) -- k1 (S K = 3 below the floor of dm_dims_of, three chunks of one time row in
the first block, S = 1 in conv33, an identity residual in the FIRST block, the single tpcnn block has the residual
convolution and stores), narrow (first block in chunks 2,2,2,2,1; the LDS / workspace switch at 63 / 64), deep (four st and
eight tpcnn blocks, the limits; J = 10 even; first block 5,3), wide3 (S = 64, J = 65, three st blocks, K = 4), kmax (K = 34;
a later block in chunks of 3 x 11 and 1; the workspace from n = 3 on) and et (the ET shape with seeded weights, as control)
-- on the layouts edge (1, 2, 3, an empty scene, 63, 64, 65, the configuration's own lds_max_n and lds_max_n + 1), big (257
and 512), many (300 scenes of 0 .. 5), graph-form scenes of 3 and 65 with the bridge's a and with an a no bridge builds, plus
bit-equalities, moved split values, a NaN and an inf coefficient, guard bands, the "not computed" branches of dmrgcn_kernel and the
graph form's refusals.

Every comparison with the restatement goes through test_gpu_dmrgcn.py's _check_scenes (C_obs rows bit for bit, obs_ori
within 2 ulp, the output within TOL = 1e-5 of the largest entry of the fp64 restatement fed the device's graph_inputs, no
scene left out) or, in the graph form, the same bound against DN.forward(sd, v, a).  The seeded weights and inputs meet one
condition on the CPU: the restatement's own float32 mode is within TOL / 4 of its fp64 mode on every scene compared here.

Measured on the MI355X (DESIGN §4 "DMRGCN", "Across the family"), largest error over a configuration's layouts, of the
largest entry: k1 5.6e-7 (big), narrow 2.0e-7, deep 2.7e-7 (moved splits, the nan layout), wide3 7.7e-7 (big), kmax 1.4e-6 (edge; 1.1e-6 with
the odd a), et 4.5e-7; the restatement's float32 mode against its fp64 mode on the same inputs (CPU): 6.7e-7, 1.9e-7, 2.5e-7,
4.2e-7, 1.5e-6, 4.1e-7 -- the kernel is no further from fp64 than numpy's fp32 is.  Every bit-equality holds, every guard
band is intact, each test takes under 1.5 s.

What the NaN test found: the contraction skips a pair that is in no bin of a graph, where the reference's dense einsum
adds 0 x[v]; a NaN coefficient therefore stayed within 9 columns of its scene of 40 (the reach of four 3x3 convolutions)
and the other 31 pedestrians got finite numbers, while the restatement -- and the reference -- answer NaN for the whole
scene.  The kernel now keeps that product once per contracted row (one fmaf per pair and row into a sum that is +0 for
finite rows: finite results keep their bits).

What notices a kernel that is wrong in numbers only (four variants of et_dmrgcn.hip, each built once and run once on the
MI355X with both DMRGCN files; none moves a write, and each reads only entries the unchanged kernel has written by then):
  1 the 1x1 convolution reads q with the time-row stride of J = 2, `tq 20 + rb J` instead of `(tq 10 + rb) J` (no larger an
    offset, rows of the same chunk): equal in every first block and wherever a later block has nt = 1.  Fails the scene and
    graph forms at kmax (later block nt = 3); tests/test_gpu_dmrgcn.py passes.
  2 the contraction takes time row `tq` instead of `t0 + tq` (a row below K): equal while a block is one chunk.  Fails every
    comparison with the restatement here but et's and two of test_gpu_dmrgcn.py (the 6 / 12 / 2 / 2 weights: chunks 6,2).
  3 `Cin = k` in a tpcnn block that is the first AND the last (fewer channels, smaller offsets into the same tensors):
    equal for n_tpcnn >= 2.  Fails every comparison at k1 and kmax (six tests); test_gpu_dmrgcn.py passes.
  4 the diagonal of a given a is left out of L (`1 - d_w d_w`; the degree still counts it; no index changes): equal for
    every a a bridge builds.  Fails the graph form at deep and kmax (the odd a); test_gpu_dmrgcn.py passes.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from . import _dmrgcn_np as DN
from ._gpu_common import *  # noqa: F401,F403 -- fixtures (dev, ops) and helpers
from .test_gpu_dmrgcn import TOL, _check_scenes, _quarter_grid, scale_err
from .test_gpu_sgcn_shapes import guarded, guards_intact, reversed_rows

pytestmark = pytest.mark.gpu
_NETS, _SD = {}, {}
assert TOL == DN.TOL


def state(name):
    if name not in _SD:
        _SD[name] = DN.random_state(name)
    return _SD[name]


def fresh_net(dev, name):
    from eigentrajectory_amd.dmrgcn import SocialDMRGCN
    m = SocialDMRGCN(**DN.module_cfg(name))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state(name).items()}, strict=True)
    return m.to(dev).eval()


def net(dev, name):
    """CONFIGS[name] with its seeded weights on the device, built once per session; nothing edits it"""
    if name not in _NETS:
        _NETS[name] = fresh_net(dev, name)
    return _NETS[name]


def counts(name):
    return dict(n_stgcn=DN.CONFIGS[name]["st"], n_tpcnn=DN.CONFIGS[name]["tp"])


def run_scenes(ops, m, C_obs, nrm, sizes):
    """-> the device's (C_pred_refine, graph_inputs) as numpy; the call without the details gives the same bits"""
    dev = next(m.parameters()).device
    Cd, nd = T(C_obs, dev), T(nrm, dev)
    out, det = ops.dmrgcn_forward_scenes(m, Cd, nd, scene_sizes=list(sizes), want_details=True)
    plain = ops.dmrgcn_forward_scenes(m, Cd, nd, scene_sizes=list(sizes))
    assert np.array_equal(N_(plain).view(np.int32), N_(out).view(np.int32))  # (as bits: a NaN equals itself)
    return N_(out), N_(det["graph_inputs"])


def ws_bytes(m, N, max_n):
    from eigentrajectory_amd import _lib as L
    p, _ = m.et_params()
    return int(L.lib().et_dmrgcn_workspace_bytes(C.byref(p), N, max_n))


@pytest.mark.parametrize("name", list(DN.CONFIGS))
def test_scene_form_at_every_config(dev, ops, name):
    """one launch on the edge layout: every non-empty scene within TOL, arenas in LDS and in the workspace in one call; the
    workspace size is the restated one on either side of the configuration's switch"""
    m = net(dev, name)
    sizes, C_obs, nrm = DN.layout_inputs(name, "edge")
    out = _check_scenes(ops, m, C_obs, nrm, list(sizes), sd=state(name), label=f"dmrgcn shapes {name} edge", **counts(name))
    assert out.shape == (DN.CONFIGS[name]["k"], sum(sizes), DN.CONFIGS[name]["S"]) and np.isfinite(out).all()
    _, _, per, lim, _, _ = DN.config_dims(name)
    N = sum(sizes)
    assert ws_bytes(m, N, lim) == DN.workspace_bytes(per, N, lim) == 0
    assert ws_bytes(m, N, lim + 1) == DN.workspace_bytes(per, N, lim + 1) == per * N * 4 > 0


def run_graph(ops, m, dev, v, a):
    vd, ad = T(v[None, None], dev), T(a[None], dev)
    out, a_back = m(vd, ad)
    assert a_back is ad and torch.equal(ops.dmrgcn_forward_graph(m, vd, ad), out)
    return N_(out)[0]


@pytest.mark.parametrize("name", list(DN.CONFIGS))
def test_graph_form_at_every_config(dev, ops, name):
    """a scene of 3 and one of 65 with the bridge's a, read as given; at deep and kmax the scene of 65 also with
    DN.odd_adjacency (asymmetric, diagonal entries inside a bin, entries on split values, a row without neighbours), which
    the kernel reads by rows with row-sum degrees and the diagonal counted: each within TOL of the restatement given the
    same a, and the two outputs differ.  The scene of 65 runs from the workspace at every configuration but k1."""
    m, sd, c = net(dev, name), state(name), DN.CONFIGS[name]
    for layout in ("g3", "g65"):
        (n,), C_obs, nrm = DN.layout_inputs(name, layout)
        v = DN.scene_input(C_obs, nrm, 0, n)
        assert v.shape == (c["k"] + 2, n)
        cases = [DN.adjacency(v)]
        if name in ("deep", "kmax") and layout == "g65":
            cases.append(DN.odd_adjacency(v))
        if layout == "g65":
            assert (ws_bytes(m, n, n) > 0) == (name != "k1")
        outs = []
        for a in cases:
            out = run_graph(ops, m, dev, v, a)
            assert out.shape == (c["S"], c["k"], n) and np.isfinite(out).all()
            err = scale_err(out, DN.forward(sd, v, a, **counts(name)))
            print(f"dmrgcn shapes {name} {layout} {'odd a' if len(outs) else 'bridge a'}: {err:.2e}")
            assert err <= TOL, (name, layout, len(outs), err)
            outs.append(out)
        if len(outs) == 2:
            assert scale_err(outs[1], outs[0]) > 1e-3


@pytest.mark.parametrize("name", ["k1", "wide3"])
def test_large_scenes(dev, ops, name):
    """scenes of 257 and 512 pedestrians in one call: scene_v's mean and every loop stride by the workgroup more than
    once, both arenas in the workspace (kmax is deliberately not run here: 6936 floats per pedestrian)"""
    sizes, C_obs, nrm = DN.layout_inputs(name, "big")
    _check_scenes(ops, net(dev, name), C_obs, nrm, list(sizes), sd=state(name), label=f"dmrgcn shapes {name} big", **counts(name))


@pytest.mark.parametrize("name", ["k1", "et"])
def test_many_scenes_in_one_call(dev, ops, name):
    """300 scenes of 0 .. 5 pedestrians: more workgroups than the device runs at once, every sixth scene empty"""
    sizes, C_obs, nrm = DN.layout_inputs(name, "many")
    assert len(sizes) == 300 and sizes.count(0) == 50
    _check_scenes(ops, net(dev, name), C_obs, nrm, list(sizes), sd=state(name), label=f"dmrgcn shapes {name} many", **counts(name))


@pytest.mark.parametrize("name", ["deep", "kmax"])
def test_bit_equalities(dev, ops, name):
    """at both block limits and at K = 34, on the edge layout (arenas in LDS and in the workspace): a scene alone equals the
    same scene inside the launch, a second run and the reversed scene order give the same bits, empty scenes among the
    others change nothing"""
    m = net(dev, name)
    sizes, C_obs, nrm = DN.layout_inputs(name, "edge")
    lim = DN.config_dims(name)[3]
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
    padded = [0]
    for n in sizes:
        padded += [n, 0] if n else [0]
    assert sum(padded) == sum(sizes) and padded.count(0) > len(sizes)
    pout, pgin = run_scenes(ops, m, C_obs, nrm, padded)
    assert np.array_equal(pout, out) and np.array_equal(pgin, gin)


@pytest.mark.parametrize("splits", [[[0.25, 0.75, 1.25, 2.5, 3.0], [0.5, 1.5, 1.75, 3.25, 5.0]],
                                    [[0.125, 0.375, 0.875, 1.625, 2.875], [0.125, 0.625, 1.125, 2.375, 4.125]]],
                         ids=["on-values", "in-gaps"])
def test_moved_splits_at_deep(dev, ops, splits):
    """test_moved_splits with four st blocks: every block decides the bins again, on the same u"""
    m = fresh_net(dev, "deep")
    m.split = splits
    C_obs, nrm = _quarter_grid(32, 3)
    sizes = [16, 16]
    out = _check_scenes(ops, m, C_obs, nrm, sizes, sd=state("deep"), label="dmrgcn shapes deep splits", split=splits,
                        **counts("deep"))
    usual = N_(ops.dmrgcn_forward_scenes(net(dev, "deep"), T(C_obs, dev), T(nrm, dev), scene_sizes=sizes))
    assert not np.array_equal(out, usual)
    a = DN.adjacency(DN.scene_input(C_obs, nrm, 0, 16))
    on = [bool((a[r] == np.float32(s)).any()) for r in range(2) for s in splits[r]]
    assert all(on) if splits[0][0] == 0.25 else not any(on)


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("name", ["narrow", "deep"])
def test_a_nan_coefficient(dev, ops, name, value):
    """narrow (and deep: later blocks, C_in = S): one NaN -- or inf -- coefficient of pedestrian 17 of the scene of 40 (the
    middle one of 4, 70, 40, 3, 9).  Every other scene is bit-equal to the run without it; inside the scene the device's
    output is NaN exactly where the fp64 restatement's is (the restatement decides how far it spreads), and finite
    entries are within TOL.  The restatement, like the reference's dense einsum, multiplies the poisoned column by the zero
    entries of every other pedestrian's Laplacian row: the whole time row, and after the first 3x3 convolution the whole
    scene, is NaN.  (Before the contraction kept that product the device skipped it with the pair and answered finite
    numbers outside 9 of the 40 columns.)"""
    m, sd = net(dev, name), state(name)
    sizes, C_obs, nrm = DN.layout_inputs(name, "nan")
    clean = _check_scenes(ops, m, C_obs, nrm, list(sizes), sd=sd, label=f"dmrgcn shapes {name} nan", **counts(name))
    assert np.isfinite(clean).all()
    s = sizes.index(40)
    lo = sum(sizes[:s])
    bad = C_obs.copy()
    bad[3, lo + 17] = value
    out, gin = run_scenes(ops, m, bad, nrm, sizes)
    keep = np.r_[0:lo, lo + 40:sum(sizes)]
    assert np.array_equal(out[:, keep], clean[:, keep])
    assert np.array_equal(gin[:, lo:lo + 40].view(np.int32)[:bad.shape[0]], bad[:, lo:lo + 40].view(np.int32))
    with np.errstate(invalid="ignore"):
        ref = DN.c_pred_refine(DN.forward(sd, gin[:, lo:lo + 40], **counts(name)))
    mine = out[:, lo:lo + 40]
    assert np.isnan(ref).any() and not np.isinf(ref).any() and not np.isinf(mine).any()
    print(f"dmrgcn shapes {name} {value}: NaN in {int(np.isnan(mine).any(axis=(0, 2)).sum())} columns of the device's output, "
          f"{int(np.isnan(ref).any(axis=(0, 2)).sum())} of the restatement's")
    assert np.array_equal(np.isnan(mine), np.isnan(ref))
    fin = np.isfinite(ref)
    if fin.any():
        assert np.abs(mine[fin] - ref[fin]).max() <= TOL * np.abs(ref[fin]).max()


def c_entry(dev, m, C_obs, nrm, sizes, fill=None, ws_nbytes=None):
    """et_dmrgcn_forward_scenes called directly, with the workspace, C_pred_refine and graph_inputs each inside a larger
    tensor of ``fill`` bytes (None: plain torch.empty buffers, no guards).  ``ws_nbytes``: the workspace handed over
    (default: et_dmrgcn_workspace_bytes, which is checked against the restated size)
    -> dict(out (k, N, S), gin (K, N): float32 views on the device, intact: the guards are as they were)"""
    from eigentrajectory_amd import _lib as L
    params, _ = m.et_params()
    K, k, S = params.seq_len, params.pred_seq_len, params.output_feat
    N = int(sum(sizes))
    nbytes = int(L.lib().et_dmrgcn_workspace_bytes(C.byref(params), N, int(max(sizes))))
    assert nbytes == DN.workspace_bytes(DN.dims(k, S, params.n_stgcn)[2], N, int(max(sizes)))
    nbytes = nbytes if ws_nbytes is None else ws_nbytes
    want = dict(ws=nbytes, out=4 * k * N * S, gin=4 * K * N)
    whole, part = {}, {}
    for key, nb in want.items():
        if fill is None:
            part[key] = torch.empty((nb,), device=dev, dtype=torch.uint8)
        else:
            whole[key], part[key] = guarded(nb, fill, dev)
        assert part[key].data_ptr() % 16 == 0
    Cd, nd = T(C_obs, dev), T(nrm, dev)
    off = T(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), dev)
    L.call("et_dmrgcn_forward_scenes", C.byref(params), L.ptr(Cd), L.ptr(nd), N, L.ptr(off), len(sizes), L.ptr(part["out"]),
           L.ptr(part["gin"]), L.ptr(part["ws"]) if nbytes else None, nbytes, L.stream(dev))
    torch.cuda.synchronize(dev)
    res = {"out": part["out"].view(torch.float32).view(k, N, S), "gin": part["gin"].view(torch.float32).view(K, N)}
    res["intact"] = all(guards_intact(whole[key], want[key], fill) for key in whole)
    return res


@pytest.mark.parametrize("name", ["k1", "wide3", "kmax"])
def test_only_the_workspace_and_the_outputs_are_written(dev, ops, name):
    """the C entry on the edge layout with the workspace (exactly et_dmrgcn_workspace_bytes), C_pred_refine and graph_inputs
    each inside a larger tensor: the guard bands stay as they were; buffers of 0xFF bytes (NaN) and of zeros give the bits
    ops.dmrgcn_forward_scenes gives -- nothing depends on what the workspace held -- and no output entry keeps the fill"""
    m = net(dev, name)
    sizes, C_obs, nrm = DN.layout_inputs(name, "edge")
    out, gin = run_scenes(ops, m, C_obs, nrm, sizes)
    assert np.isfinite(out).all() and (out != 0).all() and np.isfinite(gin).all()
    for fill in (0xFF, 0x00):
        got = c_entry(dev, m, C_obs, nrm, sizes, fill=fill)
        assert got["intact"], (name, fill)
        assert np.array_equal(N_(got["out"]), out) and np.array_equal(N_(got["gin"]), gin), (name, fill)
        assert not bool((got["out"].view(torch.int32) == (-1 if fill else 0)).any()), (name, fill)


def test_scenes_the_c_entry_does_not_compute(dev, ops):
    """the two branches of dmrgcn_kernel that answer NaN rows, ET_OK from the launch in both.  (1) wide3 (7 pedestrians fit
    LDS), scenes of 3, 10, 5, 12, 9, 2 and a workspace that ends with the scene of 10's rows: the scenes of 3, 5 and 2 (LDS)
    and of 10 (its rows end inside the workspace) equal the full run bit for bit, the scenes of 12 and 9 are NaN in the
    output and in graph_inputs, written over zero-filled buffers whose guard bands stay intact.  (2) k1, a scene of
    ET_SCENE_MAX_N + 1 = 16385 between scenes of 2 and 3: NaN, the small ones are computed as if alone"""
    from eigentrajectory_amd._lib import SCENE_MAX_N
    m = net(dev, "wide3")
    sizes = (3, 10, 5, 12, 9, 2)
    _, _, per, lim, _, _ = DN.config_dims("wide3")
    assert lim == 7
    C_obs, nrm = DN.synthetic_split(sizes, 5, DN.CONFIGS["wide3"]["k"])
    full, full_gin = run_scenes(ops, m, C_obs, nrm, sizes)
    assert np.isfinite(full).all()
    got = c_entry(dev, m, C_obs, nrm, sizes, fill=0x00, ws_nbytes=4 * per * 13)
    out, gin = N_(got["out"]), N_(got["gin"])
    assert got["intact"]
    done, left = np.r_[0:18, 39:41], np.r_[18:39]
    assert np.array_equal(out[:, done], full[:, done]) and np.array_equal(gin[:, done], full_gin[:, done])
    assert np.isnan(out[:, left]).all() and np.isnan(gin[:, left]).all()
    # (2)
    m = net(dev, "k1")
    big = SCENE_MAX_N + 1
    sizes = (2, big, 3)
    C_obs, nrm = DN.synthetic_split(sizes, 6, 1)
    small = np.r_[0:2, 2 + big:2 + big + 3]
    ref, ref_gin = run_scenes(ops, m, np.ascontiguousarray(C_obs[:, small]), np.ascontiguousarray(nrm[:, small]), (2, 3))
    assert np.isfinite(ref).all()
    got = c_entry(dev, m, C_obs, nrm, sizes, fill=0x00)
    out, gin = N_(got["out"]), N_(got["gin"])
    assert got["intact"]
    assert np.isnan(out[:, 2:2 + big]).all() and np.isnan(gin[:, 2:2 + big]).all()
    assert np.array_equal(out[:, small], ref) and np.array_equal(gin[:, small], ref_gin)


def test_graph_form_refusals(dev, ops):
    """wide3: a scene of 8 needs the workspace -- none, or one four bytes short, is ET_ERR_WORKSPACE (4); a scene of
    ET_SCENE_MAX_N + 1 is ET_ERR_INVALID_ARG (1); nothing is launched: the output keeps what it held"""
    from eigentrajectory_amd import _lib as L
    m = net(dev, "wide3")
    p, _ = m.et_params()
    _, _, per, lim, _, _ = DN.config_dims("wide3")
    n = lim + 1
    v, a = torch.zeros((1, 1, 4, n), device=dev), torch.zeros((1, 2, 4, n, n), device=dev)
    out = torch.full((1, 64, 2, n), 7.0, device=dev)
    short = torch.empty((4 * per * n - 4,), device=dev, dtype=torch.uint8)
    for ws in (None, short):
        rc = L.lib().et_dmrgcn_forward_graph(C.byref(p), L.ptr(v), L.ptr(a), n, L.ptr(out), L.ptr(ws),
                                             0 if ws is None else ws.numel(), L.stream(dev))
        assert rc == 4
    exact = torch.empty((4 * per * n,), device=dev, dtype=torch.uint8)
    rc = L.lib().et_dmrgcn_forward_graph(C.byref(p), L.ptr(v), L.ptr(a), L.SCENE_MAX_N + 1, L.ptr(out), L.ptr(exact),
                                         exact.numel(), L.stream(dev))
    assert rc == 1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert L.lib().et_dmrgcn_forward_graph(C.byref(p), L.ptr(v), L.ptr(a), n, L.ptr(out), L.ptr(exact), exact.numel(),
                                           L.stream(dev)) == 0  # the exact size is taken
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == 7.0).any())
