"""DMRGCN training without a GPU: the float64 restatement (tests/_dmrgcn_train_np.py) against torch's float64 autograd of the
stock-torch twin (tests/_dmrgcn_twin.py) and against the reference's recorded run (G32, tools/make_golden_dmrgcn_train.py),
its forward against the eval restatement, ``draw_keep`` against the reference's draw, the seed and bound conditions of the
GPU tests' scenes, the enable_native_training contract, the host-side argument checks of the new C entries and their
declarations."""
import copy
import ctypes as C
import re

import numpy as np
import pytest
import torch

from . import _abi_header as H
from . import _dmrgcn_np as DN
from . import _dmrgcn_train_cases as CS
from . import _dmrgcn_train_np as TN
from . import _dmrgcn_twin as TW
from . import _golden as G

F64 = 1e-9   # float64 against float64: of each tensor's largest entry
G32 = G.load("g32_dmrgcn_train.npz")
G32_CASES = sorted({k.split(".")[0] for k in G32.files if k.endswith(".grad64")})


def _equal(got, want, key, tm=None):
    """within F64 of the tensor's largest entry, plus the float64 rounding of the sum itself where the sum of its terms'
    magnitudes ``tm`` is known: 2^-40 of it (a PReLU slope's gradient is one sum over the whole scene that can cancel; with two
    pedestrians and both directions of an edge kept a graph's rows sum to zero and the gcn bias gradients are rounding
    residues on both sides)"""
    tol = F64 * max(float(np.abs(want).max()), 1e-300)
    if tm is not None:
        tol += 2.0 ** -40 * float(np.max(tm))
    assert float(np.abs(got - want).max()) <= tol, key


def twin_grads(m, v, a, d_out, keep):
    """float64 autograd of the twin of ``m`` -> (out (S, k, n), {name: gradient})"""
    tw = TW.Twin(copy.deepcopy(m)).double().train()
    out, _ = tw(torch.from_numpy(v)[None, None], torch.from_numpy(a)[None], None if keep is None else torch.from_numpy(keep))
    out.backward(torch.from_numpy(d_out).double())
    return out.detach().numpy()[0], {q: p.grad.numpy() for q, p in tw.named_parameters()}


@pytest.mark.parametrize("name", list(CS.CONFIGS))
@pytest.mark.parametrize("kind", ["ones", "draw", "zeros", "triu"])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_restatement_equals_autograd_of_the_twin(name, kind, n):
    m = CS.module(name)
    sd = CS.random_state(name)
    (v, a), d_out = CS.scene(name, n), CS.d_out(name, n)
    keep = CS.keep_mask(kind, v.shape[0], n)
    R = TN.run(sd, v, a, d_out[0], keep=keep)
    out, grads = twin_grads(m, v, a, d_out, keep)
    _equal(R["out"].val, out, "out")
    assert list(R["grads"]) == [q for q, _ in m.named_parameters()] == list(grads)
    for q, g in grads.items():
        _equal(R["grads"][q].val, g, q, R["grads"][q].tm)
        assert (R["grads"][q].err >= 0).all() and np.isfinite(R["grads"][q].err).all()
    if n == 1 or kind == "zeros":   # every bin empty: L = 0, both gcn tensors have an exactly zero gradient
        assert all(not R["grads"][q].val.any() and not grads[q].any() for q in TN.gcn_names(sd))
    if kind == "triu" and n > 1:    # [w, v] is not [v, w]: the transposed mask is another function
        Rt = TN.run(sd, v, a, d_out[0], keep=np.ascontiguousarray(np.swapaxes(keep, -1, -2)))
        assert np.abs(Rt["out"].val - R["out"].val).max() > 1e-3 * np.abs(R["out"].val).max()


@pytest.mark.parametrize("name", list(CS.CONFIGS))
def test_null_mask_keeps_everything_and_the_forward_is_the_eval_restatement(name):
    sd = CS.random_state(name)
    (v, a), d_out = CS.scene(name, 5), CS.d_out(name, 5)
    ones = TN.run(sd, v, a, d_out[0], keep=CS.keep_mask("ones", v.shape[0], 5))
    null = TN.run(sd, v, a, d_out[0], keep=None)
    ref = DN.forward(sd, v, a, n_stgcn=1, n_tpcnn=CS.CONFIGS[name][0])
    assert np.array_equal(ones["out"].val, ref) and np.array_equal(null["out"].val, ref)   # exactly
    assert all(np.array_equal(ones["grads"][q].val, null["grads"][q].val) for q in sd)
    keep = CS.keep_mask("draw", v.shape[0], 5)
    drawn = TN.run(sd, v, a, d_out[0], keep=keep)
    assert np.array_equal(drawn["out"].val, DN.forward(sd, v, TN.apply_keep(a, keep), n_stgcn=1, n_tpcnn=CS.CONFIGS[name][0]))
    assert np.abs(drawn["out"].val - ref).max() > 1e-3 * np.abs(ref).max()                 # DropEdge changes the function


def g32_gradients(sd, flat):
    out, at = {}, 0
    for q, t in sd.items():
        out[q] = np.asarray(flat[at:at + t.size]).reshape(t.shape)
        at += t.size
    assert at == len(flat)
    return out


def g32_case(case):
    """-> (config name, sd, v, a, keep, d_out) of a recorded case"""
    name = str(G32[f"{case}.config"])
    sd = {q: G32[f"net.{name}.{q}"] for q in CS.random_state(name)}
    v = G32[f"{case}.v"]
    keep = CS.unpack_bits(G32[f"{case}.keep_bits"], (2, 5, v.shape[0], v.shape[1], v.shape[1]))
    return name, sd, v, DN.adjacency(v), keep, G32[f"{case}.d_out"]


@pytest.mark.parametrize("case", G32_CASES)
def test_restatement_equals_the_reference_g32(case):
    name, sd, v, a, keep, d_out = g32_case(case)
    assert all(np.array_equal(sd[q], t) for q, t in CS.random_state(name).items())
    R = TN.run(sd, v, a, d_out[0], keep=keep)
    _equal(R["out"].val, G32[f"{case}.out64"], "out")
    assert np.abs(G32[f"{case}.out32"] - G32[f"{case}.out64"]).max() <= 1e-4 * np.abs(G32[f"{case}.out64"]).max()
    for q, g in g32_gradients(sd, G32[f"{case}.grad64"]).items():
        _equal(R["grads"][q].val, g, q, R["grads"][q].tm)
    assert R["decisions"]["prelu"]["undecided"] == 0
    if v.shape[1] == 1:
        assert all(not R["grads"][q].val.any() for q in TN.gcn_names(sd))


@pytest.mark.parametrize("case", G32_CASES)
def test_draw_keep_reproduces_the_reference_draw(case):
    import eigentrajectory_amd as ET
    name, _, v, _, keep, _ = g32_case(case)
    m = ET.SocialDMRGCN(**CS.module_kw(name))
    torch.manual_seed(int(G32["seed"]))
    mine = m.draw_keep(v.shape[1], "cpu")
    assert mine.dtype == torch.uint8 and tuple(mine.shape) == keep.shape and np.array_equal(mine.numpy(), keep)
    gen = torch.Generator().manual_seed(int(G32["seed"]))
    assert torch.equal(m.draw_keep(v.shape[1], "cpu", generator=gen), mine)
    assert m.drop_edge_percent == 0.8 and ET.SocialDMRGCN.drop_edge_percent == 0.8
    if v.shape[1] >= 5:   # independent per entry: [w, v] and [v, w] differ, and about 0.8 of the entries stay
        assert not np.array_equal(keep, np.swapaxes(keep, -1, -2)) and 0.7 < keep.mean() < 0.9


def test_seeds_keep_the_bounds_non_vacuous():
    """every scene of the GPU tests: no kept PReLU input inside its own step's bound, and no gradient tensor whose bound
    reaches half its largest entry (the analytically zero gcn tensors of L = 0 excepted)"""
    for name in CS.CONFIGS:
        sd = CS.random_state(name)
        sizes = CS.EXACT_N + ((CS.train_arena_limit(name), CS.train_arena_limit(name) + 1) if name == "et" else ())
        for n in sizes:
            (v, a), d_out = CS.scene(name, n), CS.d_out(name, n)
            for kind in (CS.MASKS if n in CS.EXACT_N else CS.EDGE_MASKS):
                R = TN.run(sd, v, a, d_out[0], keep=CS.keep_mask(kind, v.shape[0], n))
                assert R["decisions"]["prelu"]["undecided"] == 0, (name, n, kind)
                zero = TN.analytic_zero(sd, n, kind)
                assert TN.vacuous(sd, R["grads"], zero) == [], (name, n, kind)
    assert CS.train_arena_limit("et") == 24


def _family(**kw):
    import eigentrajectory_amd as ET
    return ET.SocialDMRGCN(**{**CS.module_kw("et"), **kw})


def test_enable_native_training_contract():
    import eigentrajectory_amd as ET
    from eigentrajectory_amd._lib import ETLibraryError
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    a, b = CS.module("et"), CS.module("et")
    keys = list(a.state_dict())
    assert ET.SocialDMRGCN.native_training is False and a.native_training is False and "native_training" not in vars(a)
    assert ET.enable_native_training(a) is a and a.native_training is True and b.native_training is False  # per instance
    assert list(a.state_dict()) == keys and not any("native" in q for q in keys)
    assert "native_training" not in dict(a.named_buffers()) and "native_training" not in dict(a.named_parameters())
    v, adj = torch.zeros((1, 1, 8, 3)), torch.zeros((1, 2, 8, 3, 3))
    before = {q: t.clone() for q, t in a.state_dict().items()}
    with pytest.raises(RuntimeError, match=re.escape(
            "SocialDMRGCN: only inference is native (no drop_edge, no dropout); training-mode forward and "
            "backward are not implemented -- call .eval() first")):
        b(v, adj)   # without the flag: today's message, word for word
    with pytest.raises(ETLibraryError, match="no CPU path"):
        a(v, adj)   # with it: the library is reached
    with pytest.raises(ETLibraryError, match="no CPU path"):
        a(v, adj, keep=torch.ones((2, 5, 8, 3, 3), dtype=torch.uint8))
    with pytest.raises(ETLibraryError, match="no CPU path"):
        a.eval()(v, adj)   # eval mode: the inference path, whatever the flag
    with pytest.raises(RuntimeError, match="no input gradient"):
        a.train()(v.clone().requires_grad_(True), adj)
    assert all(torch.equal(before[q], t) for q, t in a.state_dict().items())
    assert ET.enable_native_training(a, False) is a and a.native_training is False
    with pytest.raises(RuntimeError, match="training-mode forward and backward are not implemented"):
        a(v, adj)
    wrapped = ET.EigenTrajectory(CS.module("et"), get_hook_func("dmrgcn"), default_hyper_params(static_dist=0.3))
    assert ET.enable_native_training(wrapped) is wrapped and wrapped.baseline_model.native_training is True
    for name in CS.CONFIGS:
        assert CS.module(name).outside_native_training() is None, name
    names = ("LBEBM", "PECNet", "SocialImplicitLight", "SGCN", "SocialSTGCNN", "SocialDMRGCN")
    dropped = _family()
    dropped.tpcnns[2].gtacn[0][2].p = 0.1
    dropped_tcn = _family()
    dropped_tcn.st_dmrgcns[0].tcn[2].p = 0.5
    for m, field in ((_family(n_stgcn=2), "n_stgcn"), (_family(input_feat=2), "input_feat"), (_family(kernel_size=5), "kernel_size"),
                     (_family(seq_len=9), "seq_len"), (_family(n_tpcnn=9), "n_tpcnn"), (_family(output_feat=65), "output_feat"),
                     (_family(pred_seq_len=33, seq_len=35), "pred_seq_len"), (dropped, "tpcnns.2.gtacn.0.2.p"),
                     (dropped_tcn, "st_dmrgcns.0.tcn.2.p")):
        with pytest.raises(NotImplementedError, match="SocialDMRGCN has no native backward pass outside its native family: ") as exc:
            ET.enable_native_training(m)
        assert field in str(exc.value) and all(nm in str(exc.value) for nm in names), (field, str(exc.value))
        assert m.native_training is False
    with pytest.raises(NotImplementedError, match="out of scope"):
        ET.enable_native_training(_family(n_stgcn=2))
    with pytest.raises(NotImplementedError, match="Linear has no native backward pass"):
        ET.enable_native_training(torch.nn.Linear(2, 2))


_params = CS.host_params


def test_arguments_are_validated_on_the_host():
    """every refusal below is answered before a launch: the calls run without a device"""
    from eigentrajectory_amd import _lib
    lib = _lib.lib()
    UNSUPPORTED, INVALID, WORKSPACE = (H.defines()[q] for q in ("ET_ERR_UNSUPPORTED", "ET_ERR_INVALID_ARG", "ET_ERR_WORKSPACE"))
    big = 1 << 40
    G_ = int(lib.et_dmrgcn_grad_floats(C.byref(_params())))
    for name in CS.CONFIGS:
        n_tp, S, k = CS.CONFIGS[name]
        assert int(lib.et_dmrgcn_grad_floats(C.byref(_params(S, k, n_tp)))) == sum(q.numel() for q in CS.module(name).parameters())
    need = int(lib.et_dmrgcn_train_workspace_bytes(C.byref(_params()), 3, 1))
    assert need > 0 and need % 4 == 0
    assert int(lib.et_dmrgcn_train_workspace_bytes(C.byref(_params()), 3, 2)) == need + 4 * G_
    cap = _lib.DMRGCN_TRAIN_MAX_N

    def graph(p, n=3, d=8, grads=8, gf=G_, ws=8, nbytes=big, **_):
        return lib.et_dmrgcn_backward_graph(C.byref(p), n, d, grads, gf, ws, nbytes, None)

    def scenes(p, n=3, off=None, ns=0, d=8, grads=8, gf=G_, ws=8, nbytes=big, **_):
        return lib.et_dmrgcn_backward_scenes(C.byref(p), n, off, ns, d, grads, gf, ws, nbytes, None)

    def fwd_graph(p, v=8, a=8, n=3, keep=None, out=8, ws=8, nbytes=big, **_):
        return lib.et_dmrgcn_train_forward_graph(C.byref(p), v, a, n, keep, out, ws, nbytes, None)

    def fwd_scenes(p, c=8, nrm=8, n=3, off=None, ns=0, keep=None, koff=None, out=8, ws=8, nbytes=big, **_):
        return lib.et_dmrgcn_train_forward_scenes(C.byref(p), c, nrm, n, off, ns, keep, koff, out, ws, nbytes, None)

    for call in (graph, scenes, fwd_graph, fwd_scenes):
        for bad in (dict(n_stgcn=2), dict(n_stgcn=0), dict(input_feat=2), dict(kernel_size=5), dict(n_tpcnn=9), dict(n_tpcnn=0),
                    dict(pred_seq_len=33, seq_len=35), dict(seq_len=9), dict(output_feat=65), dict(output_feat=0)):
            assert call(_params(**bad)) == UNSUPPORTED, (call.__name__, bad)
        p = _params()
        p.split[1][2] = 0.25   # not ascending
        assert call(p) == UNSUPPORTED
        p = _params()
        p.tpcnns[1].gta_w = None
        assert call(p) == INVALID
        p = _params()
        p.tpcnns[1].res_w = 8   # only the first block has a residual convolution
        assert call(p) == INVALID
        assert call(_params(), ws=None) == WORKSPACE and call(_params(), nbytes=need - 1) == WORKSPACE
        assert call(_params(), n=-1) == INVALID
        assert call(_params(), n=cap + 1) == INVALID   # one scene above the training cap
    assert graph(_params(), d=None) == INVALID and graph(_params(), grads=None) == INVALID and graph(_params(), gf=G_ - 1) == INVALID
    assert scenes(_params(), d=None) == INVALID and scenes(_params(), grads=None) == INVALID and scenes(_params(), gf=3) == INVALID
    assert scenes(_params(), off=8, ns=0) == INVALID and fwd_scenes(_params(), off=8, ns=0) == INVALID
    assert fwd_graph(_params(), v=None) == INVALID and fwd_graph(_params(), a=None) == INVALID
    assert fwd_graph(_params(), out=None) == INVALID and fwd_graph(_params(), n=0) == 0   # an empty scene: a no-op
    assert fwd_scenes(_params(), c=None) == INVALID and fwd_scenes(_params(), nrm=None) == INVALID
    assert fwd_scenes(_params(), out=None) == INVALID
    assert fwd_scenes(_params(), off=8, ns=2, keep=8, koff=None) == INVALID   # a packed mask needs its offset table
    assert lib.et_dmrgcn_backward_graph(None, 3, 8, 8, G_, 8, big, None) == INVALID
    assert lib.et_dmrgcn_train_workspace_bytes(C.byref(_params(n_stgcn=2)), 3, 1) == 0
    assert lib.et_dmrgcn_train_workspace_bytes(C.byref(_params()), 0, 1) == 0
    assert lib.et_dmrgcn_train_workspace_bytes(C.byref(_params()), 3, 0) == 0
    assert lib.et_dmrgcn_grad_floats(C.byref(_params(n_stgcn=2))) == 0


def test_abi_names_declared_and_mirrored():
    from eigentrajectory_amd import _lib, ops
    header = H.text()
    names = ("et_dmrgcn_train_workspace_bytes", "et_dmrgcn_grad_floats", "et_dmrgcn_train_layout", "et_dmrgcn_train_forward_graph",
             "et_dmrgcn_train_forward_scenes", "et_dmrgcn_backward_graph", "et_dmrgcn_backward_scenes")
    for name in names:
        assert re.search(rf"\b{name}\(", header) and name in _lib.SYMBOLS and hasattr(_lib.lib(), name), name
    at = [_lib.SYMBOLS.index(q) for q in ("et_dmrgcn_forward_scenes",) + names]
    assert at == list(range(at[0], at[0] + len(at)))   # after the inference section, in header order
    assert [header.index(q + "(") for q in names] == sorted(header.index(q + "(") for q in names)
    d = H.defines()
    assert d["ET_DMRGCN_TRAIN_LAYOUT_FIELDS"] == _lib.DMRGCN_TRAIN_LAYOUT_FIELDS and d["ET_ABI_VERSION"] == 3
    assert d["ET_DMRGCN_TRAIN_MAX_N"] == _lib.DMRGCN_TRAIN_MAX_N == 512
    assert H.struct_fields("et_dmrgcn_params") == [f for f, _ in _lib.DMRGCNParams._fields_]   # unchanged
    off = (C.c_int64 * _lib.DMRGCN_TRAIN_LAYOUT_FIELDS)()
    lib, p = _lib.lib(), _params()
    assert lib.et_dmrgcn_train_layout(C.byref(p), 3, 1, off, _lib.DMRGCN_TRAIN_LAYOUT_FIELDS) == 0
    o = list(off)
    K, S, k, tp = 8, 20, 6, 4
    arena = DN.dims(k, S, 1)[2] + 2 * S
    assert o[:10] == sorted(o[:10]) and o[0] == 0 and o[1] == K and o[2] == K + 20 * K and o[5] == K + 20 * K + 3 * S * K
    assert o[11] == 5 * k * S + S and o[12] == 2 * k * S + S
    assert o[10] == K + 20 * K + 5 * S * K + tp * (o[11] + o[12]) + arena     # floats per pedestrian
    assert o[13] == 3 * o[10] and o[14] == lib.et_dmrgcn_grad_floats(C.byref(p)) and o[15] == o[13] + o[14]
    assert o[15] * 4 == lib.et_dmrgcn_train_workspace_bytes(C.byref(p), 3, 1)
    assert lib.et_dmrgcn_train_layout(C.byref(p), 3, 1, off, 5) == d["ET_ERR_INVALID_ARG"]
    assert lib.et_dmrgcn_train_layout(C.byref(_params(n_stgcn=2)), 3, 1, off, 16) == d["ET_ERR_UNSUPPORTED"]
    for fn in ("dmrgcn_train_workspace", "dmrgcn_train_forward_graph", "dmrgcn_train_forward_scenes", "dmrgcn_backward_graph",
               "dmrgcn_backward_scenes", "dmrgcn_grad_views", "dmrgcn_train_views"):
        assert callable(getattr(ops, fn))
