"""Native ET-GPGraph-SGCN training on the GPU (csrc/et_gpgraph_train.inl on csrc/et_sgcn_train.inl; eigentrajectory_amd/
gpgraph.py): the training forward against the eval forward, every kept value and every gradient against the float64
restatement's derived bounds (tests/_gpgraph_train_np.py: both passes step by step on the device's own kept inputs of each
step), the scenes form, determinism, zero and sparse upstream gradients and a wrapped model under ETTrainer.  No tolerance is
fixed in advance: every comparison with the restatement is |device - value| <= bound.

The fixture G30 (the reference's float64 gradients; tests/test_gpgraph_train_cpu.py holds the restatement against it to 1e-9)
is compared with the device under the restatement's whole-chain bound (``run(..., propagate=True)``), the distance to the
exact gradient.  That bound is a worst case carried through three passes and back through the input gradient: sharp for the
small configuration (k1: below half the largest entry for 14 to 26 of its 41 tensors), very loose for the ET shape (median
bound / largest entry 170 to 870 at n <= 5, mostly infinite at n = 17), so the test also prints, and DESIGN records, the
plain measured distance |device - reference| / largest entry per group.

Measured on the MI355X ("GP-Graph-SGCN training"): every comparison within its bound; largest error / bound
of the gradients 0.43 (group_mix), 0.23 (group_gen), 0.072 (output), below 0.065 for the other groups; of a kept forward value
1.000 (one rounding against a half-ulp bound), of a kept backward value 0.98 (d dense_s); scenes form 0.006 (edge) and 0.001
(many); undecided decisions at most 511 of 10.2 million (kmax, n = 65), none in the exact cases, no undecided pair.  Against
G30: error / whole-chain bound at most 0.26 (group_mix), 0.037 (output), below 0.01 elsewhere; |device - reference| / largest
entry at most 1.6e-4 (interaction_mask, et at n = 17), 4.9e-5 (stsgcn), below 4e-6 for the other groups."""
import numpy as np
import pytest
import torch

from eigentrajectory_amd import _lib as L_

from . import _golden as G
from . import _gpgraph_np as GN
from . import _gpgraph_train_cases as CS
from . import _gpgraph_train_np as GT
from . import _sgcn_np as SN
from . import _sgcn_train_np as TN
from ._gpu_common import *  # noqa: F401,F403 -- fixtures (dev, ops) and helpers

pytestmark = pytest.mark.gpu
_MODULES = {}


def net(dev, name, sd=None):
    if name not in _MODULES:
        _MODULES[name] = CS.module(name, dev).eval()
    return _MODULES[name] if sd is None else CS.set_threshold(_MODULES[name], sd)


def to_np(x):
    if isinstance(x, dict):
        return {k: to_np(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [to_np(v) for v in x]
    return N_(x) if torch.is_tensor(x) else x


def native(ops, dev, name, sd, va, vr, d_out, want_views=True):
    """training forward + backward, graph form -> (out (S, k, n), indices, {name: gradient}, kept values) as numpy, the flat
    buffer"""
    m = net(dev, name, sd)
    n = va.shape[1]
    a, r = T(va[None, None], dev), T(vr[None], dev)
    ws = ops.gpgraph_sgcn_train_workspace(m, n)
    out, idx = ops.gpgraph_sgcn_train_forward_graph(m, a, r, ws)
    flat = ops.gpgraph_sgcn_backward_graph(m, ws, T(d_out[None], dev))
    grads = {k: N_(g) for k, g in ops.gpgraph_sgcn_grad_views(m, flat).items()}
    kept = None
    if want_views:
        kept = to_np(ops.gpgraph_sgcn_train_views(m, ws, n))
        kept["out"] = N_(out)[0]
    return N_(out)[0], N_(idx), grads, kept, flat


def check(tag, sd, va, vr, d_out, out, idx, grads, kept, exact=False):
    """every kept value, the output and every gradient within the restatement's bound; the decisions' bookkeeping"""
    n = va.shape[1]
    R = GT.run(sd, va, vr, d_out, device=kept)
    worst = {g: 0.0 for g in GT.GROUPS}
    for k, ref in R["grads"].items():
        if "key.bias" in k:
            assert not grads[k].any(), (tag, k)   # an exact zero
            continue
        worst[GT.group_of(k)] = max(worst[GT.group_of(k)], TN.compare(grads[k], ref))
    kr = R["kept_ratio"]
    back = {k: r for k, r in kr.items() if k.split(".")[-1].startswith(("d_", "g_", "dir_", "dd_", "dx", "srec", "trec"))}
    print(f"{tag}: G = {R['n_groups']}, pairs {R['pairs']}, kept error / bound {max(kr.values()):.3f} ({max(kr, key=kr.get)}), of "
          f"the backward's {max(back.values()):.3f} ({max(back, key=back.get)}), gradients "
          + ", ".join(f"{g} {w:.2e}" for g, w in worst.items()) + f"; decisions {R['decisions']}")
    assert R["pairs"]["undecided"] == 0, (tag, R["pairs"])
    assert np.array_equal(idx, R["own_indices"]), (tag, idx, R["own_indices"])   # no undecided pair: the restatement's own index
    for fig in R["decisions"]:
        for kind in ("mask", "prelu"):
            assert fig[kind]["flips_outside_band"] == 0, (tag, fig)
            assert fig[kind]["undecided"] <= SN.CAP_SCENE * fig[kind]["entries"], (tag, fig)
            if exact:
                assert fig[kind]["undecided"] == 0, (tag, fig)
    assert not GT.vacuous(R["grads"], n, R["n_groups"]), (tag, GT.vacuous(R["grads"], n, R["n_groups"]))
    # group_cnn's bias is left out of that condition: its exact gradient is 0 (the distance reads f_i - f_j), and the device's
    # value lies around 0 within the bound of its own sum plus d f's step bounds (tests/test_gpgraph_train_cpu.py: the
    # restatement's own value is float64 noise, below 1e-9 of the weight's gradient)
    assert (np.abs(grads["group_gen.group_cnn.0.bias"]) <= R["bias_zero_bound"]).all(), (tag, grads["group_gen.group_cnn.0.bias"], R["bias_zero_bound"])
    if n > 1:
        assert R["bias_zero_bound"].max() < 0.5 * np.abs(grads["group_gen.group_cnn.0.weight"]).max(), (tag, R["bias_zero_bound"])
    assert all(r <= 1.0 for r in kr.values()), (tag, {k: r for k, r in kr.items() if r > 1.0})
    assert all(w <= 1.0 for w in worst.values()), (tag, worst)
    return R


def eval_forward(ops, dev, name, sd, va, vr):
    out, idx = ops.gpgraph_sgcn_forward_graph(net(dev, name, sd), T(va[None, None], dev), T(vr[None], dev))
    return N_(out)[0], N_(idx)


def case(name, n):
    va, vr = CS.scene(name, n)
    return CS.case_state(name, [va]), va, vr, CS.d_out(name, n)


@pytest.mark.parametrize("name", CS.EXACT_CONFIGS)
def test_exact_cases(dev, ops, name):
    """scenes of 1, 2, 3, 5: bit-equal to the eval forward, everything within bound with an EMPTY band, a second run bit-equal;
    one pedestrian: P = [[1]], exact zeros for group_cnn and th"""
    for n in CS.EXACT_N:
        sd, va, vr, d_out = case(name, n)
        out, idx, grads, kept, flat = native(ops, dev, name, sd, va, vr, d_out)
        ref_out, ref_idx = eval_forward(ops, dev, name, sd, va, vr)
        assert np.array_equal(out, ref_out) and np.array_equal(idx, ref_idx) and idx.dtype == np.int64
        R = check(f"exact {name} n={n}", sd, va, vr, d_out, out, idx, grads, kept, exact=True)
        assert torch.equal(flat, native(ops, dev, name, sd, va, vr, d_out, want_views=False)[4])   # determinism
        if n == 1:
            assert not any(grads[k].any() for k in grads if k.startswith("group_gen")), {k: grads[k] for k in grads if k.startswith("group_gen")}
        if n >= 3:
            assert 1 < R["n_groups"] < n


@pytest.mark.parametrize("name,n", CS.RAGGED)
def test_ragged_and_deep(dev, ops, name, n):
    sd, va, vr, d_out = case(name, n)
    out, idx, grads, kept, flat = native(ops, dev, name, sd, va, vr, d_out)
    ref_out, ref_idx = eval_forward(ops, dev, name, sd, va, vr)
    assert np.array_equal(out, ref_out) and np.array_equal(idx, ref_idx)
    R = check(f"ragged {name} n={n}", sd, va, vr, d_out, out, idx, grads, kept)
    assert 1 < R["n_groups"] < n
    assert torch.equal(flat, native(ops, dev, name, sd, va, vr, d_out, want_views=False)[4])


@pytest.mark.parametrize("which", sorted(CS.LAYOUTS))
def test_scenes_form(dev, ops, which):
    """a scene's kept values are bit for bit what the scene gives alone; the batch's gradients equal the ascending fixed-order
    sum of the single-scene device gradients within the fp32 bound of that sum (tests/test_gpu_sgcn_train.py: the batch adds
    the same per-workgroup partials in one chain over all scenes' chunks, so per element the two differ by at most
    gamma(chunks + scenes) x the sum of the partials' magnitudes, bounded through the restatement's ``tm``; the attention
    tensors follow through the linear prep backward); an empty scene contributes nothing"""
    name, sizes, C_obs, nrm = CS.layout(which)
    scenes = list(SN.scenes_of(sizes, C_obs, nrm))
    sd = CS.case_state(name, [GN.bridge_input(v)[0] for _, _, _, v in scenes])
    m = net(dev, name, sd)
    N = int(sum(sizes))
    k, S = SN.CONFIGS[name]["k"], SN.CONFIGS[name]["S"]
    d_all = np.random.default_rng([7, N]).normal(0, 1, (k, N, S)).astype(np.float32)
    out, ws = ops.gpgraph_sgcn_train_forward_scenes(m, T(C_obs, dev), T(nrm, dev), list(sizes))
    assert np.array_equal(N_(out), N_(ops.gpgraph_sgcn_forward_scenes(m, T(C_obs, dev), T(nrm, dev), list(sizes))))
    flat = ops.gpgraph_sgcn_backward_scenes(m, ws, T(d_all, dev), list(sizes))
    assert torch.equal(flat, ops.gpgraph_sgcn_backward_scenes(m, ws, T(d_all, dev), list(sizes)))
    batch = {key: N_(g).astype(np.float64) for key, g in ops.gpgraph_sgcn_grad_views(m, flat).items()}
    total = {key: np.zeros(np.asarray(w).shape, np.float32) for key, w in sd.items()}
    mags = {key: np.zeros(np.asarray(w).shape) for key, w in sd.items()}
    sum_n2, sq, n_chunks = sum(s * s for s in sizes), 0, 0
    dab_mag = [np.zeros(4), np.zeros(4)] + [np.zeros(4) for _ in range(6)]
    pr = None
    for s, lo, n, _ in scenes:
        mine = to_np(ops.gpgraph_sgcn_train_views(m, ws, N, sum_n2, len(sizes), lo=lo, sq=sq, scene_n=n, scene=s))
        va, vr = np.ascontiguousarray(mine["v_abs"]), np.ascontiguousarray(np.stack([mine["passes"][0]["vp"], mine["passes"][0]["v"]]))
        d_out = np.ascontiguousarray(d_all[:, lo:lo + n].transpose(2, 0, 1))                 # (S, k, n)
        _, idx, grads, kept, _ = native(ops, dev, name, sd, va, vr, d_out)
        for key in ("f", "dist", "sig", "sn", "colsum", "group_index", "d_vp", "d_P", "d_sig", "d_d", "d_f"):
            assert np.array_equal(kept[key], mine[key]), (which, s, key)
        for p_ in range(3):
            assert np.array_equal(kept["d_o"][p_], mine["d_o"][p_]), (which, s, p_)
            for key, val in kept["passes"][p_].items():
                if key == "dx" and p_ == 0:
                    continue   # pass 0's input is detached: its input gradient is not formed
                pairs = zip(val, mine["passes"][p_][key]) if isinstance(val, list) else [(val, mine["passes"][p_][key])]
                assert all(np.array_equal(a, b) for a, b in pairs), (which, s, p_, key)
        sq += n * n
        kept["out"] = N_(out)[:, lo:lo + n].transpose(2, 0, 1)
        R = GT.run(sd, va, vr, d_out, device=kept)
        pr = R["passes"][0]["prep"]
        n_chunks += sum(GT.slots_of(va.shape[0], m_) for m_ in (n, R["n_groups"], n)) + 3
        for key in total:
            total[key] = total[key] + grads[key]          # ascending, in fp32
            g = R["grads"][key]
            tm = np.abs(g.val) if g.tm is None or np.size(g.tm) != g.val.size else np.asarray(g.tm).reshape(g.val.shape)
            mags[key] += g.err + tm
        for p_ in range(3):
            for q in range(2):
                dab_mag[q] += R["passes"][p_]["dab"][q].tm + R["passes"][p_]["dab"][q].err
            for q in range(6):
                dab_mag[2 + q] += R["passes"][p_]["dh"][q].tm + R["passes"][p_]["dh"][q].err
    g = TN.gamma(n_chunks + len(sizes) + -(-N // L_.GPGRAPH_BWD_ROWS) + 2)
    z4 = np.zeros(4)
    lin = TN.prep_bwd(pr[0], TN.V(z4, g * dab_mag[0]), TN.V(z4, g * dab_mag[1]), CS.BASE + SN.SWA + "spatial_attention.")
    lin.update(GT.prep_t_bwd(pr[1], [TN.V(z4, g * dab_mag[2 + q]) for q in range(6)], CS.BASE + SN.SWA + "temporal_attention."))
    worst = 0.0
    for key in total:
        if "key.bias" in key:
            assert not batch[key].any()
            continue
        b = lin[key].err.reshape(mags[key].shape) + 2 * len(sizes) * TN.U * np.abs(total[key]) if key in lin else g * mags[key]
        err = np.abs(batch[key] - total[key].astype(np.float64))
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = float(np.where(err == 0, 0.0, err / b).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (which, key, ratio)
    print(f"scenes form {which}: batch against the fixed-order sum of {len(scenes)} scenes, error / bound {worst:.3f}")


def test_a_scene_beyond_the_limit_contributes_nothing(dev, ops):
    """a listed scene larger than ET_SGCN_MAX_N is not computed: NaN rows, and the gradients are the other scenes'"""
    name = "k1"
    sizes = [3, L_.SGCN_MAX_N + 1, 2]
    C_obs, nrm = SN.synthetic_split(sizes, 5, SN.CONFIGS[name]["k"])
    keep = np.r_[0:3, 3 + sizes[1]:sum(sizes)]
    sd = CS.case_state(name, [GN.bridge_input(SN.scene_input(C_obs, nrm, 0, 3))[0]])
    m = net(dev, name, sd)
    d_all = np.random.default_rng(3).normal(0, 1, (1, sum(sizes), 1)).astype(np.float32)
    out, ws = ops.gpgraph_sgcn_train_forward_scenes(m, T(C_obs, dev), T(nrm, dev), sizes)
    assert np.isnan(N_(out)[:, 3:3 + sizes[1]]).all() and np.isfinite(N_(out)[:, keep]).all()
    flat = ops.gpgraph_sgcn_backward_scenes(m, ws, T(d_all, dev), sizes)
    assert bool(flat.any()) and bool(torch.isfinite(flat).all())
    d_nan = d_all.copy()
    d_nan[:, 3:3 + sizes[1]] = np.nan                     # its rows of d_out are not read
    assert torch.equal(flat, ops.gpgraph_sgcn_backward_scenes(m, ws, T(d_nan, dev), sizes))
    # the same two scenes around an EMPTY one: the same partials in the same order (the mix weights' partials are per chunk of
    # rows, whose cut moves with the rows in between: they are left to the comparison above)
    out2, ws2 = ops.gpgraph_sgcn_train_forward_scenes(m, T(C_obs[:, keep], dev), T(nrm[:, keep], dev), [3, 0, 2])
    assert np.array_equal(N_(out2), N_(out)[:, keep])
    flat2 = ops.gpgraph_sgcn_backward_scenes(m, ws2, T(d_all[:, keep], dev), [3, 0, 2])
    a, b = ops.gpgraph_sgcn_grad_views(m, flat), ops.gpgraph_sgcn_grad_views(m, flat2)
    assert all(torch.equal(a[key], b[key]) for key in a if not key.startswith("group_mix")), [key for key in a if not torch.equal(a[key], b[key])]


def test_zero_and_sparse_d_out(dev, ops):
    """a zero upstream gradient: all-zero gradients.  A gradient on one pedestrian only reaches the others through the paths
    that exist: the mix and the tail are per pedestrian (d o_m and d ts are zero off its column / row), the unpool hands d o_1
    to its group's row alone, and in the intra-group pass A_s^T d (A_s x) is zero outside its group (the same-group mask zeroes
    A_s there) while in the pedestrian pass it is not; the mask logits read every pedestrian's attention row, so the input
    gradient itself is dense, and is checked by value against the restatement"""
    name, n = "et", 17
    sd, va, vr, d_out = case(name, n)
    _, _, grads, _, _ = native(ops, dev, name, sd, va, vr, np.zeros_like(d_out), want_views=False)
    assert all(not g.any() for g in grads.values())   # exact zeros
    one = np.zeros_like(d_out)
    one[:, :, 11] = d_out[:, :, 11]
    out, idx, grads, kept, _ = native(ops, dev, name, sd, va, vr, one)
    check("sparse d_out", sd, va, vr, one, out, idx, grads, kept)
    for p_ in range(3):   # the mix is per pedestrian: d o_m is non-zero in column 11 alone
        d_o = kept["d_o"][p_]
        assert d_o[:, 11].any() and not np.delete(d_o, 11, axis=1).any()
    pooled = kept["passes"][1]["d_out"]                  # the unpool: the group of pedestrian 11 alone
    assert pooled[:, idx[11]].any() and not np.delete(pooled, idx[11], axis=1).any()
    for p_, row in ((0, 11), (1, idx[11]), (2, 11)):     # the tail is per node
        d_ts = kept["passes"][p_]["d_ts"]
        assert d_ts[row].any() and not np.delete(d_ts, row, axis=0).any()
    outside = idx != idx[11]
    assert outside.any() and kept["passes"][2]["dx"][1][:, 11].any()
    assert kept["passes"][2]["dx_as"][11].any() and not kept["passes"][2]["dx_as"][outside].any()   # the same-group mask
    assert kept["passes"][0]["dx_as"][outside].any()
    assert grads["group_gen.group_cnn.0.weight"].any() and grads["group_gen.th"].any()
    assert grads["group_mix.st_gcns_mix.1.weight"].any() and grads[CS.BASE + SN.SWA + "temporal_attention.embedding.weight"].any()


G30 = G.load("g30_gpgraph_sgcn_train.npz")
G30_CASES = sorted({k.split(".")[0] for k in G30.files})


@pytest.mark.parametrize("case", G30_CASES)
def test_fixture_g30(dev, ops, case):
    """the reference's GPGraph in training mode (CPU): its group index, its fp32 output within TOL of the largest entry
    (tests/_sgcn_np.py: two fp32 implementations), and its float64 gradients within the restatement's whole-chain bound of the
    device's (the step-by-step check of the same case is ``check``: this one is about the reference)"""
    name = str(G30[f"{case}.config"])
    va, vr, d_out = G30[f"{case}.v_abs"], G30[f"{case}.v_rel"], G30[f"{case}.d_out"]
    n = va.shape[1]
    sd = CS.case_state(name, [va])
    assert float(sd["group_gen.th"][0]) == float(G30[f"{case}.th"])
    out, idx, grads, kept, _ = native(ops, dev, name, sd, va, vr, d_out)
    assert np.array_equal(idx, G30[f"{case}.indices"])
    ref_out = G30[f"{case}.out32"]
    assert np.abs(out - ref_out).max() <= SN.TOL * np.abs(ref_out).max()
    check(f"g30 {case}", sd, va, vr, d_out, out, idx, grads, kept)
    wanted = CS.g30_gradients(G30, case, sd)
    with np.errstate(all="ignore"):
        R = GT.run(sd, va, vr, d_out, propagate=True)   # the distance to the exact gradient: whole-chain bounds
    worst, dist, sharp = {g: 0.0 for g in GT.GROUPS}, {g: 0.0 for g in GT.GROUPS}, 0
    for k, ref in R["grads"].items():
        if "key.bias" in k:
            continue   # the reference's is rounding noise, the device's an exact zero
        if n == 1 and k.startswith("group_gen"):
            assert not grads[k].any(), (case, k)   # P = [[1]]: exact zeros (the reference's: noise)
            continue
        g = GT.group_of(k)
        worst[g] = max(worst[g], TN.compare(grads[k], TN.V(wanted[k], ref.err)))
        if k != "group_gen.group_cnn.0.bias":
            dist[g] = max(dist[g], float(np.abs(grads[k] - wanted[k]).max() / max(np.abs(wanted[k]).max(), 1e-300)))
            sharp += int(R["loose"][k] < 0.5)
    print(f"g30 {case}: device against the reference's float64 gradients, error / whole-chain bound "
          + ", ".join(f"{g} {w:.2e}" for g, w in worst.items()) + "; |device - reference| / largest entry "
          + ", ".join(f"{g} {w:.2e}" for g, w in dist.items()) + f"; tensors whose bound is below half their largest entry: {sharp}")
    assert all(w <= 1.0 for w in worst.values()), (case, worst)


def _wrapped(dev, native_flag):
    import eigentrajectory_amd as ET
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.data import TrajectoryData
    from eigentrajectory_amd.trainer import ETTrainer
    from eigentrajectory_amd.utils import default_hyper_params
    fit_obs, fit_pred = synth(2048, seed=3)
    obs, pred = fit_obs[:96], fit_pred[:96]
    # (clip_grad far above any gradient norm of these scenes: the clipping then multiplies by exactly 1.0)
    hp = default_hyper_params(lr=1e-3, weight_decay=1e-4, static_dist=0.3, batch_size=8, clip_grad=1e6, lr_schd=False)
    model = ET.EigenTrajectory(CS.module("et"), get_hook_func("gpgraphsgcn"), hp).to(dev)
    model.calculate_parameters(T(fit_obs, dev), T(fit_pred, dev))
    if native_flag:
        assert ET.enable_native_training(model) is model and model.baseline_model.native_training is True
    data = TrajectoryData.from_arrays(obs, pred, [(i, i + 3) for i in range(0, 96, 3)])
    return ETTrainer(model, hp, data, data, data, mode="sequenced", device=dev), data


def test_trainer_step(dev, ops):
    """one ETTrainer step of a wrapped model through the gpgraphsgcn bridge: every parameter's .grad is set, and it is what the
    direct ops call gives for the inputs the bridge built and the gradient that arrived at the predictor's output"""
    tr, data = _wrapped(dev, True)
    tr.model.train()
    seen = {}
    h1 = tr.predictor.register_forward_pre_hook(lambda mod, args: seen.__setitem__("in", [a.detach().clone() for a in args]))

    def grab(mod, args, res):   # (returns None: the output stays what it is)
        res[0].register_hook(lambda g: seen.__setitem__("g", g.detach().clone()))
    h2 = tr.predictor.register_forward_hook(grab)
    tr.optimizer.zero_grad(set_to_none=True)
    loss = tr._train_batch(data, [0])   # one scene: the gradients arrive as its backward left them
    h1.remove(), h2.remove()
    params = dict(tr.predictor.named_parameters())
    assert len(params) == 97 + 6 and all(p.grad is not None and p.grad.shape == p.shape for p in params.values())
    assert all(bool(torch.isfinite(p.grad).all()) for p in params.values()) and np.isfinite(loss)
    assert sum(bool(p.grad.any()) for p in params.values()) >= 97 + 6 - 3   # the two key.bias: exact zeros; group_cnn's bias
    m = tr.predictor
    a, r = (x.contiguous() for x in seen["in"])
    ws = ops.gpgraph_sgcn_train_workspace(m, a.shape[3])
    ops.gpgraph_sgcn_train_forward_graph(m, a, r, ws)
    direct = ops.gpgraph_sgcn_grad_views(m, ops.gpgraph_sgcn_backward_graph(m, ws, seen["g"]))
    norm = float(torch.sqrt(sum((g.double() ** 2).sum() for g in direct.values())))
    assert norm < tr.hp.clip_grad, norm   # not clipped: bit for bit what the backward left
    assert all(torch.equal(p.grad, direct[k]) for k, p in params.items()), [k for k, p in params.items() if not torch.equal(p.grad, direct[k])]
    for step in range(3):
        tr.optimizer.zero_grad(set_to_none=True)
        tr._train_batch(data, list(range(8)))
        tr.optimizer.step()
    plain, data = _wrapped(dev, False)
    plain.model.train()
    with pytest.raises(RuntimeError, match="training-mode forward is not implemented"):
        plain._train_batch(data, [0])


def test_autograd_contract(dev, ops):
    import eigentrajectory_amd as ET
    name, n = "et", 5
    sd, va, vr, d_out = case(name, n)
    m = ET.enable_native_training(CS.set_threshold(CS.module(name, dev), sd).train())
    a, r, g = T(va[None, None], dev), T(vr[None], dev), T(d_out[None], dev)
    out, idx = m(a, r)
    assert out.requires_grad and not idx.requires_grad and idx.dtype == torch.int64
    out.backward(g)
    _, ref_idx, grads, _, _ = native(ops, dev, name, sd, va, vr, d_out, want_views=False)
    assert np.array_equal(N_(idx), ref_idx)
    assert all(np.array_equal(N_(p.grad), grads[k]) for k, p in m.named_parameters())   # the direct ops call
    with pytest.raises(RuntimeError, match="no input gradient"):
        m(a, r.clone().requires_grad_(True))
    out3, _ = m(a, r)
    with torch.no_grad():
        m.group_gen.th.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out3.backward(g)
    out4, _ = m(a, r)
    m.group_gen.th = torch.nn.Parameter(m.group_gen.th.detach().clone())   # another tensor under the same name
    with pytest.raises(RuntimeError, match="a parameter tensor was replaced between forward and backward"):
        out4.backward(g)
    m.eval()
    assert m(a, r)[0].requires_grad is False   # eval mode: the inference path, whatever the flag
