"""csrc/et_sgcn_core.inl away from the two members of its family tests/test_gpu_sgcn.py runs (7 asym / 5 tcn / k 6 / S 20 and
3 / 2 / 6 / 12, both T = 8, no scene above 130): the configurations of tests/_sgcn_np.py: CONFIGS, each chosen for a path --
k1 (one asym layer: the logits are the only layer's output, written straight into the caller's buffers; tcns[0] only; one
output lane; T = 3), k2_wide (an even layer count: the ping-pong ends in the other buffer; S = 64, every lane of the tail's
output block), deep (eight asym and eight tcn layers, the limits), k12 (T = 14, S = 33), kmax (T = 34 = kSnMaxT: full
register arrays in sgcn_fuse, the largest tail LDS) and et (the ET shape with the seeded weights, as control) -- on the scene
layouts EDGE_SIZES (1, 2, 3, an empty scene, 63, 64, 65), 257 and 512 pedestrians (scene_v's strided mean and copies, the
limit), 300 scenes in one call (the strided scene_sq_before, the 65536 / n_scenes cap of the chunks), plus a NaN coefficient,
bit-equalities, the workspace (its size restated, nothing written outside it or outside the outputs, no dependence on what it
held), the two "not computed" cases of the C entry and the refusals one step outside every limit.

Every comparison with the fp64 restatement goes through SN.check_against unchanged: logits within DELTA = 1e-5, no decision
differs outside the band, the band within 0.5 % of a scene and 1e-4 of a launch, the output within TOL = 1e-5 of the largest
entry of the restatement run with the device's in-band decisions; no scene is left out.  The seeded weights and inputs meet
two conditions on the CPU (tests/test_sgcn_cpu.py): the restatement's own float32 mode is within DELTA / 2 (logits) and
TOL / 4 (output) of fp64, and the fp64 logits alone keep the band within the caps.

Measured on the MI355X (DESIGN §4 "SGCN", "Across the family"), largest logit error / output error over a configuration's
layouts: k1 2.1e-6 / 1.9e-6, k2_wide 1.1e-6 / 8.6e-7, deep 2.9e-6 / 4.2e-7, k12 8.9e-7 / 4.9e-7, kmax 5.9e-7 / 4.0e-7, et
1.8e-6 / 5.4e-7; at most 5.3e-5 of a launch undecided (kmax).  Every bit-equality holds and every guard band is intact.

What notices a kernel that is wrong in numbers only (four in-bounds variants of et_sgcn_core.inl / et_scene_helpers.inl, run
once on the MI355X; tests/test_gpu_sgcn.py passes all four): Cin = j ? k : min(T, 8) in sgcn_tail -- the scene and graph forms
at k12 and kmax and the NaN test fail; the tcn residual applied at j = 0 when n_tcn = 1 -- every comparison at k1 fails;
scene_v's mean over the first 256 pedestrians only -- the four large-scene tests fail; ident_t read with strides of 8 where
T >= 8 -- the graph form at k12 fails."""
import ctypes as C

import numpy as np
import pytest
import torch

from . import _sgcn_np as SN
from ._gpu_common import *  # noqa: F401,F403 -- fixtures (dev, ops) and helpers
from .test_gpu_sgcn import scale_err

pytestmark = pytest.mark.gpu
GUARD = 4096  # bytes on either side of every buffer the kernels may write
_NETS, _SD = {}, {}


def state(name):
    if name not in _SD:
        _SD[name] = SN.random_state(name)
    return _SD[name]


def net(dev, name):
    """CONFIGS[name] with its seeded weights on the device, built once per session; nothing edits it"""
    if name not in _NETS:
        from eigentrajectory_amd.sgcn import SGCN
        m = SGCN(**SN.module_cfg(name))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in state(name).items()}, strict=True)
        _NETS[name] = m.to(dev).eval()
    return _NETS[name]


def run_scenes(ops, m, C_obs, nrm, sizes):
    """-> the device's (C_pred_refine, packed logit_s, packed logit_t) as numpy; the call without the logits gives the
    same bits"""
    dev = next(m.parameters()).device
    Cd, nd = T(C_obs, dev), T(nrm, dev)
    out, ls, lt = ops.sgcn_forward_scenes(m, Cd, nd, scene_sizes=list(sizes), want_logits=True)
    plain = ops.sgcn_forward_scenes(m, Cd, nd, scene_sizes=list(sizes))
    assert np.array_equal(N_(plain).view(np.int32), N_(out).view(np.int32))  # (as bits: a NaN equals itself)
    return N_(out), N_(ls), N_(lt)


def blocks(sizes, T_, ls, lt):
    """the documented packing: scene s's (T, 4, n, n) block at 4 T (n_0^2 + ... + n_{s-1}^2) of logit_s, its (n, 4, T, T)
    block at 4 T T (n_0 + ... + n_{s-1}) of logit_t -> [(lo, n, block_s, block_t)]"""
    res, lo, sq = [], 0, 0
    for n in sizes:
        res.append((lo, n, ls[4 * T_ * sq:4 * T_ * (sq + n * n)].reshape(T_, 4, n, n),
                    lt[4 * T_ * T_ * lo:4 * T_ * T_ * (lo + n)].reshape(n, 4, T_, T_)))
        lo, sq = lo + n, sq + n * n
    assert ls.size == 4 * T_ * sq and lt.size == 4 * T_ * T_ * lo
    return res


def check_launch(name, label, sizes, C_obs, nrm, out, ls, lt):
    """every non-empty scene of one launch through check_against, the launch's undecided entries within CAP_SPLIT"""
    c = SN.CONFIGS[name]
    T_ = c["k"] + 2
    assert out.shape == (c["k"], sum(sizes), c["S"])
    und = total = 0
    worst_l = worst_o = 0.0
    for lo, n, bs, bt in blocks(sizes, T_, ls, lt):
        if n == 0:
            continue
        ids, idt = SN.bridge_identities(T_, n)
        fig = SN.check_against(state(name), SN.scene_input(C_obs, nrm, lo, lo + n), ids, idt, out[:, lo:lo + n], bs, bt)
        und, total = und + fig["undecided"], total + fig["entries"]
        worst_l, worst_o = max(worst_l, fig["logit_err"]), max(worst_o, fig["out_err"])
    print(f"sgcn shapes {name} {label}: logit error {worst_l:.2e}, output error {worst_o:.2e}, undecided {und} of {total}")
    assert und <= SN.CAP_SPLIT * total, (name, label, und, total)


def reversed_rows(sizes):
    off = np.concatenate([[0], np.cumsum(sizes)])
    return np.concatenate([np.arange(off[i], off[i + 1]) for i in reversed(range(len(sizes)))]).astype(np.int64)


@pytest.mark.parametrize("name", list(SN.CONFIGS))
def test_scene_form_at_every_config(dev, ops, name):
    """one launch on EDGE_SIZES with the logits: every scene against the restatement, its logit blocks unpacked with the
    configuration's own T"""
    sizes, C_obs, nrm = SN.layout_inputs(name, "edge")
    out, ls, lt = run_scenes(ops, net(dev, name), C_obs, nrm, sizes)
    assert np.isfinite(out).all() and np.isfinite(ls).all() and np.isfinite(lt).all()
    check_launch(name, "edge", sizes, C_obs, nrm, out, ls, lt)


def run_graph(ops, m, dev, v, ids, idt):
    vd, ident = T(v[None, :, :, None], dev), [T(ids, dev), T(idt, dev)]
    out, ls, lt = ops.sgcn_forward_graph(m, vd, ident, want_logits=True)
    assert torch.equal(ops.sgcn_forward_graph(m, vd, ident), out) and torch.equal(m(vd, ident), out)
    return N_(out), N_(ls), N_(lt)


@pytest.mark.parametrize("name", list(SN.CONFIGS))
def test_graph_form_at_every_config(dev, ops, name):
    """a scene of 3 and one of 65 with the bridge's identities; at k12 (T = 14) also a spatial identity that changes with t
    and has an entry off the diagonal, and a per-pedestrian temporal one that is neither all ones nor eye(T): read with the
    configuration's T strides, and each changes the output"""
    m, sd = net(dev, name), state(name)
    T_ = SN.CONFIGS[name]["k"] + 2
    for layout in ("g3", "g65"):
        (n,), C_obs, nrm = SN.layout_inputs(name, layout)
        v = SN.scene_input(C_obs, nrm, 0, n)
        assert v.shape == (T_, n)
        ids, idt = SN.bridge_identities(T_, n)
        cases = [(ids, idt)]
        if name == "k12" and layout == "g65":
            i, t, u = np.arange(n), np.arange(T_), np.arange(T_)
            idt_full = (0.25 + 0.25 * ((i[:, None, None] + 2 * t[None, :, None] + u[None, None, :]) % 4)).astype(np.float32)
            assert idt_full.shape == (n, T_, T_) and not (idt_full == 1).all() and idt_full[0, 0, 1] != 0
            ids_t = np.eye(n, dtype=np.float32)[None] * (1 + 0.25 * t.astype(np.float32))[:, None, None]
            ids_t[t[:, None], i[None, :], (i[None, :] + t[:, None] + 1) % n] += 0.5
            cases += [(ids, idt_full), (np.ascontiguousarray(ids_t), idt)]
        outs = []
        for a, b in cases:
            out, ls, lt = run_graph(ops, m, dev, v, a, b)
            assert out.shape == (T_ - 2, n, SN.CONFIGS[name]["S"]) and ls.shape == (T_, 4, n, n) and lt.shape == (n, 4, T_, T_)
            fig = SN.check_against(sd, v, a, b, out, ls, lt)
            print(f"sgcn shapes {name} {layout}: logit error {fig['logit_err']:.2e}, output error {fig['out_err']:.2e}, "
                  f"undecided {fig['undecided']} of {fig['entries']}")
            outs.append(out)
        for p in range(len(outs)):
            for q in range(p):
                assert scale_err(outs[p], outs[q]) > 1e-3, (p, q)


def lay_restated(T_, N, n2, S):
    """the workspace of et_sgcn_core.inl: lay_of, in floats, every block rounded up to 4: a header of 64, the scenes' stack
    offsets (int64 [S + 1]), v (T, N), the spatial and the temporal softmax rows' (max, sum), two spatial stacks (T, 4, n2),
    three temporal ones (N, 4, T, T), three feature arrays (N, 4, T, 16) -> ({block: offset}, total)"""
    sizes = [("hdr", 64), ("sq", 2 * (S + 1)), ("v", T_ * N), ("rs_s", 2 * T_ * 4 * N), ("rs_t", 2 * T_ * 4 * N),
             ("xa", T_ * 4 * n2), ("xb", T_ * 4 * n2), ("ta", N * 4 * T_ * T_), ("tb", N * 4 * T_ * T_), ("at", N * 4 * T_ * T_),
             ("f2", N * 4 * T_ * 16), ("f1", N * 4 * T_ * 16), ("ts", N * 4 * T_ * 16)]
    at, where = 0, {}
    for block, size in sizes:
        where[block] = at
        at = (at + size + 3) // 4 * 4
    return where, at


def guarded(nbytes, fill, dev):
    """-> (the whole tensor, its middle ``nbytes``): GUARD bytes on either side, every byte ``fill``"""
    whole = torch.full((GUARD + nbytes + GUARD,), fill, device=dev, dtype=torch.uint8)
    return whole, whole[GUARD:GUARD + nbytes]


def guards_intact(whole, nbytes, fill):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[GUARD + nbytes:] == fill).all())


def c_entry(dev, m, C_obs, nrm, sizes, sum_n2=None, fill=None, n2_buffers=None):
    """et_sgcn_forward_scenes called directly, with the workspace, C_pred_refine and both logit buffers each inside a larger
    tensor of ``fill`` bytes (None: plain torch.empty buffers, no guards).  ``sum_n2``: what the call is told (default: the
    scenes' squared sizes); ``n2_buffers``: what the workspace and logit_s are sized for (default: the same)
    -> dict(out, ls, lt, ws: float32 views on the device, intact: the guards are as they were)"""
    from eigentrajectory_amd import _lib as L
    params, _ = m.et_params()
    T_, k, S = params.obs_len, params.pred_len, params.out_dims
    N = int(sum(sizes))
    honest = int(sum(n * n for n in sizes))
    sum_n2 = honest if sum_n2 is None else sum_n2
    n2_buffers = sum_n2 if n2_buffers is None else n2_buffers
    nbytes = L.lib().et_sgcn_workspace_bytes(C.byref(params), N, n2_buffers, len(sizes))
    assert nbytes == 4 * lay_restated(T_, N, n2_buffers, len(sizes))[1]  # exactly what the header of lay_of says
    want = dict(ws=nbytes, out=4 * k * N * S, ls=4 * 4 * T_ * n2_buffers, lt=4 * N * 4 * T_ * T_)
    whole, part = {}, {}
    for key, nb in want.items():
        if fill is None:
            part[key] = torch.empty((nb,), device=dev, dtype=torch.uint8)
        else:
            whole[key], part[key] = guarded(nb, fill, dev)
        assert part[key].data_ptr() % 16 == 0
    Cd, nd = T(C_obs, dev), T(nrm, dev)
    off = T(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), dev)
    L.call("et_sgcn_forward_scenes", C.byref(params), L.ptr(Cd), L.ptr(nd), N, L.ptr(off), len(sizes), sum_n2,
           int(max(sizes)), L.ptr(part["out"]), L.ptr(part["ls"]), L.ptr(part["lt"]), L.ptr(part["ws"]), nbytes, L.stream(dev))
    torch.cuda.synchronize(dev)
    res = {key: t.view(torch.float32) for key, t in part.items()}
    res["out"] = res["out"].view(k, N, S)
    res["intact"] = all(guards_intact(whole[key], want[key], fill) for key in whole)
    return res


@pytest.mark.parametrize("layout", ["big", "limit"])
@pytest.mark.parametrize("name", ["k1", "k2_wide"])
def test_large_scenes(dev, ops, name, layout):
    """one scene of 257 and one of 512 = ET_SGCN_MAX_N pedestrians: scene_v's mean and its copy loops stride by the workgroup.
    The scene form returns no v, so the restatement is fed SN.scene_input; the v the kernels did form is read from the
    workspace of a direct call: the C_obs rows bit for bit, the obs_ori rows within 2 ulp (at the scale of the scene's
    positions: both sides are a fp32 mean in their own summation order, subtracted once) of the numpy fp32 value"""
    m = net(dev, name)
    sizes, C_obs, nrm = SN.layout_inputs(name, layout)
    (n,), k = sizes, SN.CONFIGS[name]["k"]
    out, ls, lt = run_scenes(ops, m, C_obs, nrm, sizes)
    check_launch(name, layout, sizes, C_obs, nrm, out, ls, lt)
    direct = c_entry(dev, m, C_obs, nrm, sizes)
    assert np.array_equal(N_(direct["out"]), out) and np.array_equal(N_(direct["ls"]), ls) and np.array_equal(N_(direct["lt"]), lt)
    at = lay_restated(k + 2, n, n * n, 1)[0]["v"]
    v = N_(direct["ws"][at:at + (k + 2) * n]).reshape(k + 2, n)
    assert np.array_equal(v[:k], C_obs)
    ulp = np.spacing(np.abs(nrm[:2]).max().astype(np.float32))
    assert np.abs(v[k:].astype(np.float64) - SN.scene_input(C_obs, nrm, 0, n)[k:]).max() <= 2 * ulp
    one = ops.sgcn_forward_scenes(m, T(C_obs, dev), T(nrm, dev))  # no scene list: one scene of N rows
    assert np.array_equal(N_(one), out)


@pytest.mark.parametrize("name", ["k1", "et"])
def test_many_scenes_in_one_call(dev, ops, name):
    """300 scenes of 1, 2, 3, ...: more than the 256 lanes that sum the squared sizes of the scenes before a scene, and
    65536 / 300 caps the chunks per scene.  Every scene against the restatement; the same scenes in reversed order give the
    same bits, scene by scene"""
    m = net(dev, name)
    T_ = SN.CONFIGS[name]["k"] + 2
    sizes, C_obs, nrm = SN.layout_inputs(name, "many")
    assert len(sizes) > 256
    out, ls, lt = run_scenes(ops, m, C_obs, nrm, sizes)
    check_launch(name, "many", sizes, C_obs, nrm, out, ls, lt)
    order = reversed_rows(sizes)
    rout, rls, rlt = run_scenes(ops, m, np.ascontiguousarray(C_obs[:, order]), np.ascontiguousarray(nrm[:, order]), sizes[::-1])
    assert np.array_equal(rout, out[:, order])
    fwd, rev = blocks(sizes, T_, ls, lt), blocks(sizes[::-1], T_, rls, rlt)[::-1]
    for (_, n, bs, bt), (_, rn, rbs, rbt) in zip(fwd, rev):
        assert n == rn and np.array_equal(bs, rbs) and np.array_equal(bt, rbt)


@pytest.mark.parametrize("name", ["deep", "kmax"])
def test_bit_equalities(dev, ops, name):
    """at both layer limits and at T = 34: a scene alone equals the same scene inside EDGE_SIZES, reversed scene order and
    a second run give the same bits, empty scenes among the others change nothing"""
    m = net(dev, name)
    T_ = SN.CONFIGS[name]["k"] + 2
    sizes, C_obs, nrm = SN.layout_inputs(name, "edge")
    out, ls, lt = run_scenes(ops, m, C_obs, nrm, sizes)
    again = run_scenes(ops, m, C_obs, nrm, sizes)
    assert all(np.array_equal(a, b) for a, b in zip(again, (out, ls, lt)))
    for lo, n, bs, bt in blocks(sizes, T_, ls, lt):
        if n == 0:
            continue
        o1, s1, t1 = run_scenes(ops, m, np.ascontiguousarray(C_obs[:, lo:lo + n]), np.ascontiguousarray(nrm[:, lo:lo + n]), [n])
        assert np.array_equal(o1, out[:, lo:lo + n]) and np.array_equal(s1, bs.ravel()) and np.array_equal(t1, bt.ravel()), n
    order = reversed_rows(sizes)
    rout, _, _ = run_scenes(ops, m, np.ascontiguousarray(C_obs[:, order]), np.ascontiguousarray(nrm[:, order]), sizes[::-1])
    assert np.array_equal(rout, out[:, order])
    padded = [0]
    for n in sizes:
        padded += [n, 0] if n else [0]
    assert sum(padded) == sum(sizes) and padded.count(0) > len(sizes)
    pout, pls, plt_ = run_scenes(ops, m, C_obs, nrm, padded)
    assert np.array_equal(pout, out) and np.array_equal(pls, ls) and np.array_equal(plt_, lt)


def test_a_nan_stays_in_its_scene(dev, ops):
    """k12: a NaN coefficient of one pedestrian of the scene of 40 makes every output row of that scene NaN (its softmax
    rows at that t are NaN for every pedestrian, and every pedestrian's temporal product reads them) and leaves every other
    scene bit-equal, logits included"""
    m = net(dev, "k12")
    T_ = SN.CONFIGS["k12"]["k"] + 2
    sizes, C_obs, nrm = SN.layout_inputs("k12", "nan")
    clean = run_scenes(ops, m, C_obs, nrm, sizes)
    assert np.isfinite(clean[0]).all()
    check_launch("k12", "nan", sizes, C_obs, nrm, *clean)
    s = sizes.index(40)
    lo = sum(sizes[:s])
    bad = C_obs.copy()
    bad[5, lo + 17] = np.nan
    got = run_scenes(ops, m, bad, nrm, sizes)
    assert np.isnan(got[0][:, lo:lo + 40]).all()
    keep = np.r_[0:lo, lo + 40:sum(sizes)]
    assert np.array_equal(got[0][:, keep], clean[0][:, keep])
    for q, (a, b) in enumerate(zip(blocks(sizes, T_, got[1], got[2]), blocks(sizes, T_, clean[1], clean[2]))):
        if q != s:
            assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), q


@pytest.mark.parametrize("name", ["k1", "k2_wide", "kmax"])
def test_only_the_workspace_and_the_outputs_are_written(dev, ops, name):
    """the C entry on EDGE_SIZES with the workspace (exactly et_sgcn_workspace_bytes), C_pred_refine and both logit buffers
    each inside a larger tensor: the guard bands stay as they were, buffers of 0xFF bytes (NaN) and of zeros give the bits
    ops.sgcn_forward_scenes gives, and no entry of the output or the logits keeps the fill"""
    from eigentrajectory_amd import _lib as L
    m = net(dev, name)
    c = SN.CONFIGS[name]
    params, _ = m.et_params()
    for N, n2, S in ((1, 1, 1), (3, 5, 2), (130, 16900, 1), (1000, 12345, 300)):
        assert L.lib().et_sgcn_workspace_bytes(C.byref(params), N, n2, S) == 4 * lay_restated(c["k"] + 2, N, n2, S)[1]
    sizes, C_obs, nrm = SN.layout_inputs(name, "edge")
    want = run_scenes(ops, m, C_obs, nrm, sizes)
    assert all(np.isfinite(a).all() and (a != 0).all() for a in want)
    for fill in (0xFF, 0x00):
        got = c_entry(dev, m, C_obs, nrm, sizes, fill=fill)
        assert got["intact"], (name, fill)
        pattern = -1 if fill else 0
        for key, ref in zip(("out", "ls", "lt"), want):
            assert np.array_equal(N_(got[key]).reshape(ref.shape), ref), (name, fill, key)
            assert not bool((got[key].view(torch.int32) == pattern).any()), (name, fill, key)


def test_scenes_the_c_entry_does_not_compute(dev, ops):
    """k1, the two cases sgcn_input answers by leaving a scene out (its stack offset is -1, every later kernel skips it, the
    tail writes NaN: nothing is read or written for it).  (1) a scene of ET_SGCN_MAX_N + 1 between two small ones, sum_n2
    the sum of all three squared sizes as include/eigentraj.h documents: its rows are NaN, the small scenes equal a run
    without it bit for bit.  (2) sum_n2 one short of what the scenes need, workspace and logit buffers sized for the honest
    value: the last scene does not fit the stacks and is NaN, the others are unchanged."""
    from eigentrajectory_amd._lib import SGCN_MAX_N
    m = net(dev, "k1")
    T_ = 3
    big = SGCN_MAX_N + 1
    sizes = (2, big, 3)
    C_obs, nrm = SN.synthetic_split(sizes, 5, 1)
    small = np.r_[0:2, 2 + big:2 + big + 3]
    ref = run_scenes(ops, m, np.ascontiguousarray(C_obs[:, small]), np.ascontiguousarray(nrm[:, small]), (2, 3))
    assert np.isfinite(ref[0]).all()
    got = c_entry(dev, m, C_obs, nrm, sizes)
    out = N_(got["out"])
    assert np.isnan(out[:, 2:2 + big]).all() and np.array_equal(out[:, small], ref[0])
    mine, theirs = blocks(sizes, T_, N_(got["ls"]), N_(got["lt"])), blocks((2, 3), T_, ref[1], ref[2])
    for a, b in ((mine[0], theirs[0]), (mine[2], theirs[1])):
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    # (2)
    sizes = (3, 2, 4)
    C_obs, nrm = SN.synthetic_split(sizes, 6, 1)
    honest = run_scenes(ops, m, C_obs, nrm, sizes)
    assert np.isfinite(honest[0]).all()
    got = c_entry(dev, m, C_obs, nrm, sizes, sum_n2=29 - 1, n2_buffers=29)
    out = N_(got["out"])
    assert np.isnan(out[:, 5:]).all() and np.array_equal(out[:, :5], honest[0][:, :5])
    mine, theirs = blocks(sizes, T_, N_(got["ls"]), N_(got["lt"])), blocks(sizes, T_, honest[1], honest[2])
    for q in (0, 1):
        assert np.array_equal(mine[q][2], theirs[q][2]) and np.array_equal(mine[q][3], theirs[q][3])


def test_one_step_outside_every_limit_is_refused(dev, ops):
    """pred_len 33, obs_len != pred_len + 2, out_dims 0 and 65, 0 and 9 asym layers, 0 and 9 tcn layers: every one of them
    constructs, its workspace size is 0 and its forward answers ET_ERR_UNSUPPORTED (status 3) before any launch; the
    device answers a good call bit for bit afterwards"""
    from eigentrajectory_amd import _lib as L
    from eigentrajectory_amd.sgcn import SGCN
    m = net(dev, "k12")
    (n,), C_obs, nrm = SN.layout_inputs("k12", "g3")
    v = T(SN.scene_input(C_obs, nrm, 0, n)[None, :, :, None], dev)
    ident = [T(a, dev) for a in SN.bridge_identities(14, n)]
    good = m(v, ident)
    assert torch.isfinite(good).all()
    base = SN.module_cfg("k12")
    for kw in (dict(pred_len=33, obs_len=35), dict(obs_len=15), dict(obs_len=13), dict(out_dims=0), dict(out_dims=65),
               dict(number_asymmetric_conv_layer=0), dict(number_asymmetric_conv_layer=9), dict(n_tcn=0), dict(n_tcn=9)):
        bad = SGCN(**{**base, **kw}).to(dev).eval()
        params, _ = bad.et_params()
        assert L.lib().et_sgcn_workspace_bytes(C.byref(params), n, n * n, 1) == 0, kw
        vv = torch.zeros((1, bad.obs_len, n, 1), device=dev)
        with pytest.raises(L.ETLibraryError, match="status 3"):
            bad(vv, ident)
        with pytest.raises(L.ETLibraryError, match="status 3"):
            ops.sgcn_forward_scenes(bad, torch.zeros((bad.pred_len, n), device=dev), torch.zeros((4, n), device=dev))
    assert torch.equal(m(v, ident), good)
