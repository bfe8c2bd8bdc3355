"""csrc/et_agentformer.hip away from the two configurations tests/test_gpu_agentformer.py runs (model 256 / 8 heads of 32 /
ff 512 and model 64 / 4 heads of 16 / ff 96): the members of the supported family in tests/_agentformer_np.py: CONFIGS, each
chosen for a path it opens -- idle wavefronts of the attention kernel (1, 3, 6 heads), head_dim 4, 20 (off the 16 grid),
128 and 256 (two and four rounds of 64 P V columns), the partial last k-step of a Linear (ff 1, 30, 97, 511), 1, 3, 5 and 6
column blocks, LayerNorm narrower than a wavefront, out_fc with 1, 17, 33 and 64 columns, four layers a side with T = 16,
k = 1 (16 scenes in one decoder tile), past_frames != future_frames + 2 in the module form -- plus scores beyond exp's fp32
range, and the workspace: its size restated, nothing written outside it or outside the outputs, no dependence on what it
held.

Every comparison is against the fp64 restatement fed the fp32 input the kernels report; TOL = 1e-5 of the largest entry,
no scene, row or configuration left out.  The restatement's own float32 mode is 1.2e-7 .. 6.1e-7 from fp64 on these
configurations (CPU, tests/test_agentformer_cpu.py), so TOL leaves more than ten times the arithmetic's own error.

Measured on the MI355X (DESIGN §4 "AgentFormer"), largest error per configuration, scene form (both layouts) / module form
(n = 1, 16, 17):
  min 6.7e-7 / 1.8e-7, h3 5.3e-7 / 3.6e-7, h6 6.4e-7 / 5.0e-7, hd4 5.6e-7 / 3.7e-7, hd20 4.6e-7 / 3.9e-7,
  hd128 6.7e-7 / 5.9e-7, hd256 8.3e-7 / 5.5e-7, deep 5.3e-7 / 5.5e-7; module form only: long_dec 4.5e-7, long_enc 2.4e-7.
Every bit-equality below holds (a scene alone through the hooks, reversed scene order, repeated calls, a 0xFF against a
zero workspace) and every guard band is intact.

Large logits (in_proj weights x 8; the restatement's largest score about 136 at h3 and 318 at hd20, exp overflows fp32 above
88.7): near-argmax attention is ill-conditioned in fp32 itself, so the bound is max(TOL, 10 x the float32 restatement's
error against fp64 at the same inputs), never a figure of the kernels.
Measured: h3 float32 restatement 1.49e-5, bound 1.49e-4, kernels 3.1e-5 (scenes of 1 / 2 / 17: 6.4e-7, 4.7e-6, 3.1e-5); hd20
float32 restatement 3.58e-5, bound 3.58e-4, kernels 2.7e-5 (1.9e-6, 1.5e-6, 2.7e-5).

What notices a kernel that is wrong in numbers only (three one-line variants of et_agentformer.hip, run once on the MI355X;
tests/test_gpu_agentformer.py passes all three): the partial k-step of af_linear dropped -- min, h3, h6, hd128 fail in both
forms; the row sum carried from one round of 64 P V columns into the next -- hd128 and hd256 fail in both forms; exp
without the row maximum -- both large-logit tests fail."""
import ctypes as C

import numpy as np
import pytest
import torch

from . import _agentformer_np as AN
from ._gpu_common import *  # noqa: F401,F403 -- fixtures (dev, ops) and helpers
from .test_gpu_agentformer import check_scenes, scale_err, state_np

pytestmark = pytest.mark.gpu
TOL = 1e-5
# a run of one-pedestrian scenes (up to 16 scenes in one 16-token tile), then boundaries inside tiles, an empty scene, 16, 17
BASE = [1] * 18 + [2, 17, 3, 0, 16, 1]
GUARD = 4096  # bytes on either side of every buffer the kernels may write
_NETS = {}


def net(dev, name):
    """CONFIGS[name] with seed-11 weights on the device, built once per session; nothing edits it"""
    if name not in _NETS:
        _NETS[name] = AN.config_module(name)[0].to(dev).eval()
    return _NETS[name]


def layouts(name):
    """the two scene layouts of configuration ``name``: BASE (+ a tail that fills the last decoder tile where k divides
    16), and the same with one more scene of 1"""
    tail = [7] if name in ("min", "hd4") else []
    return BASE + tail, BASE + tail + [1]


def run_scenes(ops, m, C_obs, nrm, sizes):
    dev = next(m.parameters()).device
    return N_(ops.agentformer_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=sizes))


@pytest.mark.parametrize("name", AN.SCENE_CONFIGS)
def test_scene_form_at_every_config(dev, ops, name):
    """every scene of both layouts against the restatement, graph_inputs, the scene alone through the hooks bit for bit
    (check_scenes); reversed scene order and a second call bit for bit.  deep and hd128 are the accept side of the limits
    (4 + 4 layers, T = 16, model 256, ff 511, S = 64)."""
    c = AN.CONFIGS[name]
    m = net(dev, name)
    k = c["k"]
    first, second = layouts(name)
    if name in ("min", "hd4"):  # the last decoder tile exactly full, then one more pedestrian (k tokens: 1 at min, 2 at hd4)
        assert (sum(first) * k) % 16 == 0 and sum(second) * k == sum(first) * k + k
        assert (sum(first) * c["T"]) % 16 == 0  # ... and the last encoder tile
    for sizes in (first, second):
        C_obs, nrm = AN.random_scenes(sizes, 3, k)
        whole = check_scenes(ops, m, name, C_obs, nrm, sizes)
        assert np.isfinite(whole).all() and whole.shape == (k, sum(sizes), c["S"])
        assert np.array_equal(whole, run_scenes(ops, m, C_obs, nrm, sizes))
        off = np.concatenate([[0], np.cumsum(sizes)])
        order = np.concatenate([np.arange(off[i], off[i + 1]) for i in reversed(range(len(sizes)))])
        rev = run_scenes(ops, m, np.ascontiguousarray(C_obs[:, order]), np.ascontiguousarray(nrm[:, order]), sizes[::-1])
        assert np.array_equal(rev, whole[:, order])


@pytest.mark.parametrize("name", list(AN.CONFIGS))
def test_module_form_at_every_config(dev, ops, name):
    """agentformer_forward_graph on scenes of 1, 16 and 17 against forward(..., frames=k); long_dec (T 3, k 16) and
    long_enc (T 16, k 1) exist in this form only"""
    c = AN.CONFIGS[name]
    m = net(dev, name)
    sd = state_np(m)
    worst = 0.0
    for n in (1, 16, 17):
        C_obs, nrm = AN.random_scenes([n], 20 + n, c["T"] - 2)
        u = AN.scene_input(C_obs, nrm, 0, n)
        assert u.shape == (c["T"], n)
        out = ops.agentformer_forward_graph(m, T(u, dev)[:, :, None])
        assert out.shape == (c["k"], n, c["S"])
        err = scale_err(N_(out), AN.forward(sd, u, c["nhead"], frames=c["k"]))
        worst = max(worst, err)
        assert err <= TOL, (name, n, err)
        assert torch.equal(out, ops.agentformer_forward_graph(m, T(u, dev)))
    print(f"{name} module form: {worst:.2e}")


@pytest.mark.parametrize("name", ["h3", "hd128"])
def test_a_nan_stays_in_its_scene(dev, ops, name):
    """with an idle wavefront walking head 0 (h3) and with two rounds of P V columns (hd128): a NaN in one pedestrian of
    the scene of 17 makes that scene NaN and leaves every other row bit-equal"""
    m = net(dev, name)
    C_obs, nrm = AN.random_scenes(BASE, 7, AN.CONFIGS[name]["k"])
    whole = run_scenes(ops, m, C_obs, nrm, BASE)
    assert np.isfinite(whole).all()
    off = np.concatenate([[0], np.cumsum(BASE)])
    s17 = BASE.index(17)
    bad = C_obs.copy()
    bad[1, off[s17] + 4] = np.nan
    got = run_scenes(ops, m, bad, nrm, BASE)
    assert np.isnan(got[:, off[s17]:off[s17 + 1]]).all()
    keep = np.r_[0:off[s17], off[s17 + 1]:off[-1]]
    assert np.array_equal(got[:, keep], whole[:, keep])


def workspace_bytes_restated(c, N):
    """the header comment of af_workspace: u (T N), the encoder's rows, projections (5 D a row) and attention output, the
    decoder's the same, the cross-attention's q | q_self (2 D a row); every block rounded up to 4 floats"""
    ME, MD, D = N * c["T"], N * c["k"], c["D"]
    blocks = [ME, ME * D, ME * 5 * D, ME * D, MD * D, MD * 5 * D, MD * D, MD * 2 * D]
    assert len(blocks) == 8
    return 4 * sum((b + 3) // 4 * 4 for b in blocks)


def guarded(nbytes, fill, dev):
    """-> (the whole tensor, its middle ``nbytes``): GUARD bytes on either side, every byte ``fill``"""
    whole = torch.full((GUARD + nbytes + GUARD,), fill, device=dev, dtype=torch.uint8)
    return whole, whole[GUARD:GUARD + nbytes]


def guards_intact(whole, nbytes, fill):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[GUARD + nbytes:] == fill).all())


@pytest.mark.parametrize("name", ["min", "hd20", "hd128"])
def test_only_the_workspace_and_the_outputs_are_written(dev, ops, name):
    """the C entry point with the workspace, C_pred_refine and graph_inputs each inside a larger tensor: the guard bands
    stay as they were, a workspace of 0xFF bytes (NaN) and one of zeros give the bits ops.agentformer_forward_scenes gives"""
    from eigentrajectory_amd import _lib as L
    c = AN.CONFIGS[name]
    m = net(dev, name)
    params, _ = m.et_params()
    k, S = c["k"], c["S"]
    n = sum(BASE)
    for N in (1, 3, n, 1000):
        assert L.lib().et_agentformer_workspace_bytes(C.byref(params), N, N) == workspace_bytes_restated(c, N), N
    nbytes = workspace_bytes_restated(c, n)
    C_obs, nrm = AN.random_scenes(BASE, 13, k)
    want, det = ops.agentformer_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=BASE, want_details=True)
    assert bool(torch.isfinite(want).all())
    c_dev, r_dev = T(C_obs, dev), T(nrm, dev)
    off = ops.scene_offsets(BASE, n, dev)
    for fill in (0xFF, 0x00):
        ws_all, ws = guarded(nbytes, fill, dev)
        out_all, out = guarded(4 * k * n * S, fill, dev)
        gin_all, gin = guarded(4 * (k + 2) * n, fill, dev)
        assert ws.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and gin.data_ptr() % 16 == 0
        L.call("et_agentformer_forward_scenes", C.byref(params), L.ptr(c_dev), L.ptr(r_dev), n, L.ptr(off), len(BASE),
               L.ptr(out), L.ptr(gin), L.ptr(ws), nbytes, L.stream(dev))
        torch.cuda.synchronize(dev)
        assert guards_intact(ws_all, nbytes, fill), (name, fill, "workspace")
        assert guards_intact(out_all, out.numel(), fill), (name, fill, "C_pred_refine")
        assert guards_intact(gin_all, gin.numel(), fill), (name, fill, "graph_inputs")
        assert torch.equal(out.view(torch.float32).view(k, n, S), want), (name, fill)
        assert torch.equal(gin.view(torch.float32).view(k + 2, n), det["graph_inputs"]), (name, fill)


@pytest.mark.parametrize("name", AN.LARGE_LOGITS["configs"])
def test_large_logits(dev, ops, name):
    """in_proj weights x 8 on scenes of 1, 2 and 17: the restatement's scores pass 88.7, where exp without the row maximum
    overflows fp32 -- the reason for the attention's first pass.  Outputs finite and within max(TOL, 10 x the float32
    restatement's error against fp64 at these inputs) of the fp64 restatement.
    Measured on the MI355X: h3 largest score 135.7, float32 restatement 1.49e-5, bound 1.49e-4, kernels 3.1e-5; hd20 317.7,
    3.58e-5, 3.58e-4, 2.7e-5."""
    c = AN.CONFIGS[name]
    sizes = AN.LARGE_LOGITS["sizes"]
    m = AN.config_module(name, in_proj_scale=AN.LARGE_LOGITS["scale"])[0].to(dev).eval()
    sd = state_np(m)
    C_obs, nrm = AN.random_scenes(sizes, AN.LARGE_LOGITS["seed"], c["k"])
    out, det = ops.agentformer_forward_scenes(m, T(C_obs, dev), T(nrm, dev), scene_sizes=sizes, want_details=True)
    out, gin = N_(out), N_(det["graph_inputs"])
    assert np.isfinite(out).all()
    stats, lo, e32, errs = {}, 0, 0.0, []
    for n in sizes:
        u = gin[:, lo:lo + n]
        ref = AN.forward(sd, u, c["nhead"], stats=stats)
        e32 = max(e32, scale_err(AN.forward(sd, u, c["nhead"], dtype=np.float32), ref))
        errs.append(scale_err(out[:, lo:lo + n], AN.c_pred_refine(ref)))
        lo += n
    assert stats["max_score"] > 88.7, stats  # the precondition: these inputs do need the row maximum
    bound = max(TOL, 10 * e32)
    print(f"{name} large logits: max score {stats['max_score']:.1f}, fp32 restatement {e32:.2e}, bound {bound:.2e}, "
          f"kernels {max(errs):.2e} {['%.2e' % e for e in errs]}")
    assert max(errs) <= bound, (name, errs, bound)
