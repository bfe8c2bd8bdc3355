"""Graph-TERN training without a GPU: the float64 restatement (tests/_graphtern_train_np.py) against torch's float64 autograd
of the stock-torch twin (tests/_graphtern_twin.py) and against the reference's recorded run (G35,
tools/make_golden_graphtern_train.py), its forward against the eval restatement, ``draw_keep`` against the reference's draw,
the seed and bound conditions of the GPU tests' scenes, the restatement's own float32 mode inside its derived bounds, the
enable_native_training contract, the host-side argument checks of the new C entries and their declarations."""
import copy
import ctypes as C
import re

import numpy as np
import pytest
import torch

from . import _abi_header as H
from . import _golden as G
from . import _graphtern_np as GN
from . import _graphtern_train_cases as CS
from . import _graphtern_train_np as TN
from . import _graphtern_twin as TW

F64 = 1e-9   # float64 against float64: of each tensor's largest entry
G35 = G.load("g35_graphtern_train.npz")
G35_CASES = sorted({k.split(".")[0] for k in G35.files if k.endswith(".grad64")})


def _equal(got, want, key, tm=None):
    """within F64 of the tensor's largest entry, plus the float64 rounding of the sum itself where the sum of its terms'
    magnitudes ``tm`` is known: 2^-40 of it (a PReLU slope's gradient is one sum over the whole scene that can cancel)"""
    tol = F64 * max(float(np.abs(want).max()), 1e-300)
    if tm is not None:
        tol += 2.0 ** -40 * float(np.max(tm))
    assert float(np.abs(got - want).max()) <= tol, key


def twin_grads(m, u, d_out, keep):
    """float64 autograd of the twin of ``m`` -> (out (k, n, S), {name: gradient or None})"""
    tw = TW.Twin(copy.deepcopy(m)).double().train()
    if keep is None:
        tw.eval()   # no mask: nothing is drawn (the network has no other training-mode behaviour: every Dropout.p = 0)
    out = tw(torch.from_numpy(GN.s_obs_of(u)), None if keep is None else torch.from_numpy(keep))
    out.backward(torch.from_numpy(d_out).double())
    return out.detach().numpy()[0], {q: None if p.grad is None else p.grad.numpy() for q, p in tw.named_parameters()}


@pytest.mark.parametrize("name", list(CS.CONFIGS))
@pytest.mark.parametrize("kind", ["null", "ones", "draw", "zeros", "triu"])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_restatement_equals_autograd_of_the_twin(name, kind, n):
    m = CS.module(name)
    sd = CS.random_state(name)
    u, d_out = CS.scene(name, n), CS.d_out(name, n)
    keep = CS.keep_mask(kind, u.shape[0], n)
    R = TN.run(sd, u, None, d_out[0], keep=keep)
    out, grads = twin_grads(m, u, d_out, keep)
    _equal(R["out"].val, out, "out")
    assert list(R["grads"]) == [q for q, _ in m.named_parameters()] == list(grads)
    for q, g in grads.items():
        if q == TN.UNUSED:   # never applied: torch leaves no gradient, the restatement an exact zero
            assert g is None and not R["grads"][q].val.any()
            continue
        _equal(R["grads"][q].val, g, q, R["grads"][q].tm)
        assert (R["grads"][q].err >= 0).all() and np.isfinite(R["grads"][q].err).all()
    o64, g64, _ = TN.plain(sd, u, None, d_out[0], keep)   # the plain statements are the same function
    _equal(o64, out, "plain out")
    for q, g in grads.items():
        if g is not None:
            _equal(g64[q], g, "plain " + q, R["grads"][q].tm)
    if kind == "zeros":             # every edge dropped: L = I exactly, P's rows are u and 1
        assert np.array_equal(R["kept"]["P"].val[:, 0], np.broadcast_to(u.astype(np.float64), (4,) + u.shape))
        assert np.array_equal(R["kept"]["P"].val[:, 1], np.ones((4,) + u.shape))
    if kind == "triu" and n > 1:    # [w, v] is not [v, w]: the transposed mask is another function
        Rt = TN.run(sd, u, None, d_out[0], keep=np.ascontiguousarray(np.swapaxes(keep, -1, -2)))
        assert np.abs(Rt["out"].val - R["out"].val).max() > 1e-3 * np.abs(R["out"].val).max()


@pytest.mark.parametrize("name", list(CS.CONFIGS))
def test_null_mask_keeps_everything_and_the_forward_is_the_eval_restatement(name):
    sd = CS.random_state(name)
    u, d_out = CS.scene(name, 5), CS.d_out(name, 5)
    ones = TN.run(sd, u, None, d_out[0], keep=CS.keep_mask("ones", u.shape[0], 5))
    null = TN.run(sd, u, None, d_out[0], keep=None)
    ref = GN.forward(sd, u)
    assert np.array_equal(ones["out"].val, null["out"].val)
    assert np.abs(null["out"].val - ref).max() <= 1e-13 * np.abs(ref).max()   # float64 both, the sums in another order
    assert all(np.array_equal(ones["grads"][q].val, null["grads"][q].val) for q in sd)
    drawn = TN.run(sd, u, None, d_out[0], keep=CS.keep_mask("draw", u.shape[0], 5))
    assert np.abs(drawn["out"].val - ref).max() > 1e-3 * np.abs(ref).max()    # DropEdge changes the function
    diag = CS.keep_mask("ones", u.shape[0], 5) * (1 - np.eye(5, dtype=np.uint8))   # A's diagonal is exactly 0
    assert np.array_equal(TN.run(sd, u, None, d_out[0], keep=diag)["out"].val, null["out"].val)


def g35_gradients(sd, flat):
    out, at = {}, 0
    for q, t in sd.items():
        out[q] = np.asarray(flat[at:at + t.size]).reshape(t.shape)
        at += t.size
    assert at == len(flat)
    return out


def g35_case(case):
    """-> (config name, sd, u, keep, d_out) of a recorded case"""
    name = str(G35[f"{case}.config"])
    sd = {q: G35[f"net.{name}.{q}"] for q in CS.random_state(name)}
    u = G35[f"{case}.u"]
    keep = CS.unpack_bits(G35[f"{case}.keep_bits"], (4, u.shape[0], u.shape[1], u.shape[1]))
    return name, sd, u, keep, G35[f"{case}.d_out"]


@pytest.mark.parametrize("case", G35_CASES)
def test_restatement_equals_the_reference_g35(case):
    name, sd, u, keep, d_out = g35_case(case)
    assert all(np.array_equal(sd[q], t) for q, t in CS.random_state(name).items())
    R = TN.run(sd, u, None, d_out[0], keep=keep)
    _equal(R["out"].val, G35[f"{case}.out64"], "out")
    assert np.abs(G35[f"{case}.out32"] - G35[f"{case}.out64"]).max() <= 1e-4 * np.abs(G35[f"{case}.out64"]).max()
    none = [str(q) for q in G35[f"{case}.grad_none"]]
    assert none == [TN.UNUSED]
    for q, g in g35_gradients(sd, G35[f"{case}.grad64"]).items():
        _equal(R["grads"][q].val, g, q, R["grads"][q].tm)
    assert R["decisions"]["prelu"]["undecided"] == 0


@pytest.mark.parametrize("case", G35_CASES)
def test_draw_keep_reproduces_the_reference_draw(case):
    import eigentrajectory_amd as ET
    name, _, u, keep, _ = g35_case(case)
    m = ET.GraphTERNLight(**CS.module_kw(name))
    torch.manual_seed(int(G35["seed"]))
    mine = m.draw_keep(u.shape[1], "cpu")
    assert mine.dtype == torch.uint8 and tuple(mine.shape) == keep.shape and np.array_equal(mine.numpy(), keep)
    gen = torch.Generator().manual_seed(int(G35["seed"]))
    assert torch.equal(m.draw_keep(u.shape[1], "cpu", generator=gen), mine)
    assert m.drop_edge_percent == 0.8 and ET.GraphTERNLight.drop_edge_percent == 0.8
    if u.shape[1] >= 5:   # independent per entry: [w, v] and [v, w] differ, and about 0.8 of the entries stay
        assert not np.array_equal(keep, np.swapaxes(keep, -1, -2)) and 0.7 < keep.mean() < 0.9


@pytest.mark.parametrize("name", list(CS.CONFIGS))
def test_seeds_keep_the_bounds_non_vacuous_and_float32_stays_inside_them(name):
    """every scene of the GPU tests: no kept PReLU input inside its own step's bound, no gradient tensor whose bound reaches
    half its largest entry, and the restatement's float32 mode within the whole-chain bounds of its float64 mode"""
    sd = CS.random_state(name)
    for n, masks in CS.sizes_of(name):
        for kind in masks:
            u, d_out = CS.scene(name, n, kind), CS.d_out(name, n)
            keep = CS.keep_mask(kind, u.shape[0], n)
            R = TN.run(sd, u, None, d_out[0], keep=keep)
            assert R["decisions"]["prelu"]["undecided"] == 0, (name, n, kind)
            assert TN.vacuous(sd, R["grads"]) == [], (name, n, kind)
            Rp = TN.run(sd, u, None, d_out[0], keep=keep, propagate=True)
            o32, g32, _ = TN.plain(sd, u, None, d_out[0], keep, np.float32)
            assert TN.compare(o32, Rp["out"]) <= 1.0, (name, n, kind)
            for q in sd:
                assert TN.compare(g32[q], Rp["grads"][q]) <= 1.0, (name, n, kind, q)
    assert CS.train_arena_limit("et") == 35


def _family(**kw):
    import eigentrajectory_amd as ET
    return ET.GraphTERNLight(**{**CS.module_kw("et"), **kw})


def test_enable_native_training_contract():
    import eigentrajectory_amd as ET
    from eigentrajectory_amd._lib import ETLibraryError
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    a, b = CS.module("et"), CS.module("et")
    keys = list(a.state_dict())
    assert ET.GraphTERNLight.native_training is False and a.native_training is False and "native_training" not in vars(a)
    assert ET.enable_native_training(a) is a and a.native_training is True and b.native_training is False  # per instance
    assert list(a.state_dict()) == keys and not any("native" in q for q in keys)
    assert "native_training" not in dict(a.named_buffers()) and "native_training" not in dict(a.named_parameters())
    s_obs = torch.zeros((1, 2, 8, 3, 1))
    before = {q: t.clone() for q, t in a.state_dict().items()}
    with pytest.raises(RuntimeError, match=re.escape(
            "GraphTERNLight: only inference is native (no drop_edge, no dropout); training-mode forward "
            "and backward are not implemented -- call .eval() first")):
        b(s_obs)   # without the flag: today's message, word for word
    with pytest.raises(ETLibraryError, match="no CPU path"):
        a(s_obs)   # with it: the library is reached
    with pytest.raises(ETLibraryError, match="no CPU path"):
        a(s_obs, keep=torch.ones((4, 8, 3, 3), dtype=torch.uint8))
    with pytest.raises(ETLibraryError, match="no CPU path"):
        a.eval()(s_obs)   # eval mode: the inference path, whatever the flag
    with pytest.raises(RuntimeError, match="no input gradient"):
        a.train()(s_obs.clone().requires_grad_(True))
    assert all(torch.equal(before[q], t) for q, t in a.state_dict().items())
    assert ET.enable_native_training(a, False) is a and a.native_training is False
    with pytest.raises(RuntimeError, match="training"):
        a(s_obs)
    wrapped = ET.EigenTrajectory(CS.module("et"), get_hook_func("graphtern"), default_hyper_params(static_dist=0.3))
    assert ET.enable_native_training(wrapped) is wrapped and wrapped.baseline_model.native_training is True
    for name in CS.CONFIGS:
        assert CS.module(name).outside_native_training() is None, name
    names = ("LBEBM", "PECNet", "SocialImplicitLight", "SGCN", "SocialSTGCNN", "SocialDMRGCN", "GraphTERNLight")
    dropped = _family()
    dropped.tpcnns[2].cpcns[0][2].p = 0.1
    dropped_tcn = _family()
    dropped_tcn.tp_mrgcns[0].tcn[2].p = 0.5
    for m, field in ((_family(n_epgcn=2), "n_epgcn = 2"), (_family(input_feat=2), "input_feat = 2"), (_family(seq_len=9), "seq_len = 9"),
                     (_family(n_epcnn=9), "n_epcnn"), (_family(n_smpl=65), "n_smpl"),
                     (_family(pred_seq_len=33, seq_len=35), "pred_seq_len"), (dropped, "tpcnns.2.cpcns.0.2.p = 0.1"),
                     (dropped_tcn, "tp_mrgcns.0.tcn.2.p = 0.5")):
        with pytest.raises(NotImplementedError, match="GraphTERNLight has no native backward pass outside its native family: ") as exc:
            ET.enable_native_training(m)
        assert field in str(exc.value) and all(nm in str(exc.value) for nm in names), (field, str(exc.value))
        assert m.native_training is False
    with pytest.raises(NotImplementedError, match="out of scope"):
        ET.enable_native_training(_family(n_epgcn=2))
    with pytest.raises(NotImplementedError, match="Linear has no native backward pass") as exc:
        ET.enable_native_training(torch.nn.Linear(2, 2))
    assert all(nm in str(exc.value) for nm in names)


_params = CS.host_params


def test_arguments_are_validated_on_the_host():
    """every refusal below is answered before a launch: the calls run without a device"""
    from eigentrajectory_amd import _lib
    lib = _lib.lib()
    UNSUPPORTED, INVALID, WORKSPACE = (H.defines()[q] for q in ("ET_ERR_UNSUPPORTED", "ET_ERR_INVALID_ARG", "ET_ERR_WORKSPACE"))
    big = 1 << 40
    G_ = int(lib.et_graphtern_grad_floats(C.byref(_params())))
    for name in CS.CONFIGS:
        k, S, n_cnn = CS.CONFIGS[name]
        assert int(lib.et_graphtern_grad_floats(C.byref(_params(S, k, n_cnn)))) == sum(q.numel() for q in CS.module(name).parameters())
    need = int(lib.et_graphtern_train_workspace_bytes(C.byref(_params()), 3, 1))
    assert need > 0 and need % 4 == 0
    assert int(lib.et_graphtern_train_workspace_bytes(C.byref(_params()), 3, 2)) == need + 4 * G_
    cap = _lib.GRAPHTERN_TRAIN_MAX_N

    def graph(p, n=3, d=8, grads=8, gf=G_, ws=8, nbytes=big, **_):
        return lib.et_graphtern_backward_graph(C.byref(p), n, d, grads, gf, ws, nbytes, None)

    def scenes(p, n=3, off=None, ns=0, d=8, grads=8, gf=G_, ws=8, nbytes=big, **_):
        return lib.et_graphtern_backward_scenes(C.byref(p), n, off, ns, d, grads, gf, ws, nbytes, None)

    def fwd_graph(p, s_obs=8, n=3, keep=None, out=8, ws=8, nbytes=big, **_):
        return lib.et_graphtern_train_forward_graph(C.byref(p), s_obs, n, keep, out, ws, nbytes, None)

    def fwd_scenes(p, c=8, nrm=8, n=3, off=None, ns=0, keep=None, koff=None, out=8, ws=8, nbytes=big, **_):
        return lib.et_graphtern_train_forward_scenes(C.byref(p), c, nrm, n, off, ns, keep, koff, out, ws, nbytes, None)

    for call in (graph, scenes, fwd_graph, fwd_scenes):
        for bad in (dict(n_epgcn=2), dict(n_epgcn=0), dict(input_feat=2), dict(hidden_feat=8), dict(n_epcnn=9), dict(n_epcnn=1),
                    dict(pred_seq_len=33, seq_len=35), dict(seq_len=9), dict(n_smpl=65), dict(n_smpl=0)):
            assert call(_params(**bad)) == UNSUPPORTED, (call.__name__, bad)
        p = _params()
        p.tpcnns[1].cpcn_w = None
        assert call(p) == INVALID
        p = _params()
        p.tpcnns[1].rest_w = 8   # only the first block has a row residual convolution
        assert call(p) == INVALID
        assert call(_params(), ws=None) == WORKSPACE and call(_params(), nbytes=need - 1) == WORKSPACE
        assert call(_params(), n=-1) == INVALID
        assert call(_params(), n=cap + 1) == INVALID   # one scene above the training cap (513 in the graph form)
    assert cap + 1 == CS.BEYOND_N
    assert graph(_params(), d=None) == INVALID and graph(_params(), grads=None) == INVALID and graph(_params(), gf=G_ - 1) == INVALID
    assert scenes(_params(), d=None) == INVALID and scenes(_params(), grads=None) == INVALID and scenes(_params(), gf=3) == INVALID
    assert scenes(_params(), off=8, ns=0) == INVALID and fwd_scenes(_params(), off=8, ns=0) == INVALID
    assert fwd_graph(_params(), s_obs=None) == INVALID
    assert fwd_graph(_params(), out=None) == INVALID and fwd_graph(_params(), n=0) == 0   # an empty scene: a no-op
    assert fwd_scenes(_params(), c=None) == INVALID and fwd_scenes(_params(), nrm=None) == INVALID
    assert fwd_scenes(_params(), out=None) == INVALID
    assert fwd_scenes(_params(), off=8, ns=2, keep=8, koff=None) == INVALID   # a packed mask needs its offset table
    assert lib.et_graphtern_backward_graph(None, 3, 8, 8, G_, 8, big, None) == INVALID
    assert lib.et_graphtern_train_workspace_bytes(C.byref(_params(n_epgcn=2)), 3, 1) == 0
    assert lib.et_graphtern_train_workspace_bytes(C.byref(_params()), 0, 1) == 0
    assert lib.et_graphtern_train_workspace_bytes(C.byref(_params()), 3, 0) == 0
    assert lib.et_graphtern_grad_floats(C.byref(_params(n_epgcn=2))) == 0


def test_abi_names_declared_and_mirrored():
    from eigentrajectory_amd import _lib, ops
    header = H.text()
    names = ("et_graphtern_train_workspace_bytes", "et_graphtern_grad_floats", "et_graphtern_train_layout",
             "et_graphtern_train_forward_graph", "et_graphtern_train_forward_scenes", "et_graphtern_backward_graph",
             "et_graphtern_backward_scenes")
    for name in names:
        assert re.search(rf"\b{name}\(", header) and name in _lib.SYMBOLS and hasattr(_lib.lib(), name), name
    at = [_lib.SYMBOLS.index(q) for q in ("et_graphtern_forward_scenes",) + names]
    assert at == list(range(at[0], at[0] + len(at)))   # after the inference section, in header order
    assert [header.index(q + "(") for q in names] == sorted(header.index(q + "(") for q in names)
    d = H.defines()
    assert d["ET_GRAPHTERN_TRAIN_LAYOUT_FIELDS"] == _lib.GRAPHTERN_TRAIN_LAYOUT_FIELDS and d["ET_ABI_VERSION"] == 3
    assert d["ET_GRAPHTERN_TRAIN_MAX_N"] == _lib.GRAPHTERN_TRAIN_MAX_N == 512
    assert H.struct_fields("et_graphtern_params") == [f for f, _ in _lib.GraphTERNParams._fields_]   # unchanged
    off = (C.c_int64 * _lib.GRAPHTERN_TRAIN_LAYOUT_FIELDS)()
    lib = _lib.lib()
    for name, (k, S, n_cnn) in CS.CONFIGS.items():   # the layout against the restated sizes
        p = _params(S, k, n_cnn)
        assert lib.et_graphtern_train_layout(C.byref(p), 3, 2, off, _lib.GRAPHTERN_TRAIN_LAYOUT_FIELDS) == 0
        o = list(off)
        T, Hd, Cm = k + 2, 16, max(16, S)
        arena = GN.dims(k, S, 1)[2]
        assert o[:10] == sorted(o[:10]) and o[0] == 0 and o[1] == T and o[2] == 5 * T and o[3] == 13 * T, name
        assert o[4] == o[3] + Hd * T and o[5] == o[4] + Hd * T, name
        assert o[11] == 2 * k * Hd + 2 * k * Cm and o[12] == k * Cm + k * Hd, name
        assert o[6] == o[5] + n_cnn * o[11] and o[7] == o[6] + n_cnn * o[12] and o[8] == o[7] + Hd * T and o[9] == o[8] + Hd * T
        assert o[10] == o[9] + arena, name                                      # floats per pedestrian
        assert o[13] == 3 * o[10] and o[14] == lib.et_graphtern_grad_floats(C.byref(p)) and o[15] == o[13] + 2 * o[14]
        assert o[15] * 4 == lib.et_graphtern_train_workspace_bytes(C.byref(p), 3, 2)
    assert lib.et_graphtern_train_layout(C.byref(_params()), 3, 1, off, 5) == d["ET_ERR_INVALID_ARG"]
    assert lib.et_graphtern_train_layout(C.byref(_params(n_epgcn=2)), 3, 1, off, 16) == d["ET_ERR_UNSUPPORTED"]
    for fn in ("graphtern_train_workspace", "graphtern_train_forward_graph", "graphtern_train_forward_scenes",
               "graphtern_backward_graph", "graphtern_backward_scenes", "graphtern_grad_views", "graphtern_train_layout",
               "graphtern_train_views", "graphtern_keep_offsets"):
        assert callable(getattr(ops, fn))
