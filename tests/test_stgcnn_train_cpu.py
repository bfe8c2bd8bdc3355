"""STGCNN training without a GPU: the float64 restatement (tests/_stgcnn_train_np.py) against torch's float64 autograd of
the stock-torch twin (tests/_stgcnn_twin.py: gradients, running statistics, num_batches_tracked), the seed and bound
conditions of the GPU tests' scenes, the enable_native_training contract, the host-side argument checks of the new C entries
and their declarations."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from . import _abi_header as H
from . import _golden as G
from . import _stgcnn_train_cases as CS
from . import _stgcnn_train_np as TN
from . import _stgcnn_twin as TW

F64 = 1e-9   # float64 against float64: of each tensor's largest entry
G31 = G.load("g31_stgcnn_train.npz")
G31_CASES = sorted({k.split(".")[0] for k in G31.files})


def _equal(got, want, key, tm=None):
    """within F64 of the tensor's largest entry -- or, for a one-element tensor, itself a sum that can cancel (a PReLU
    slope's gradient), within F64 of the sum of its terms' magnitudes ``tm``"""
    scale = max(float(np.abs(want).max()), 1e-300)
    if tm is not None and np.size(want) == 1:
        scale = max(scale, float(np.max(tm)))
    assert float(np.abs(got - want).max()) <= F64 * scale, key


@pytest.mark.parametrize("name", list(CS.CONFIGS))
@pytest.mark.parametrize("n", [1, 3])
def test_restatement_equals_autograd_of_the_twin(name, n):
    m = CS.module(name)
    sd = CS.state(m)
    (v, a), d_out = CS.scene(name, n), CS.d_out(name, n)
    R = TN.run(sd, v, a, d_out, momentum=CS.MOMENTUM, eps=CS.EPS)
    tw = TW.clone(m)
    out, grads = TW.grads(tw, v[None, None], a, d_out)
    _equal(R["out"].val, out.numpy()[0], "out")
    zero = TN.exact_zero_names(sd)
    for k, g in grads.items():
        g = g.numpy()
        if k in zero:   # exact zeros here; autograd leaves rounding noise at the two biases in front of a BatchNorm
            assert not R["grads"][k].val.any()
            assert np.abs(g).max() <= 1e-12 * max(np.abs(x.numpy()).max() for x in grads.values()), k
            continue
        _equal(R["grads"][k].val, g, k, R["grads"][k].tm)
        assert (R["grads"][k].err >= 0).all() and np.isfinite(R["grads"][k].err).all()
    assert list(R["grads"]) == [k for k, _ in m.named_parameters()]
    buf = TW.buffers(tw)
    assert sorted(R["buffers"]) == sorted(buf)
    for k, b in buf.items():
        if k.endswith("num_batches_tracked"):
            assert R["buffers"][k] == int(b) == int(sd[k]) + 1
        else:
            _equal(R["buffers"][k].val, b, k)
            assert np.abs(b - sd[k]).max() > 0   # the buffers moved


def g31_gradients(sd, flat):
    """fixture G31's flat state_dict-order vector -> {parameter name: array}"""
    out, at = {}, 0
    for k in TN.parameter_names(sd):
        shape = np.asarray(sd[k]).shape
        cnt = int(np.prod(shape))
        out[k] = np.asarray(flat[at:at + cnt]).reshape(shape)
        at += cnt
    assert at == len(flat)
    return out


@pytest.mark.parametrize("case", G31_CASES)
def test_restatement_equals_the_reference_g31(case):
    """the reference's social_stgcnn in training mode (float64, CPU): its gradients, running statistics and
    num_batches_tracked to 1e-9; its fp32 output within the whole-chain fp32 bound"""
    name = str(G31[f"{case}.config"])
    sd = CS.state(CS.module(name))
    R = TN.run(sd, G31[f"{case}.v"], G31[f"{case}.a"], G31[f"{case}.d_out"], momentum=CS.MOMENTUM, eps=CS.EPS)
    assert R["decisions"]["prelu"]["undecided"] == 0
    zero = TN.exact_zero_names(sd)
    want = g31_gradients(sd, G31[f"{case}.grad64"])
    for k, g in want.items():
        if k in zero:   # the reference: rounding noise at the two biases, zeros (no .grad) at the unused tail
            assert not R["grads"][k].val.any() and np.abs(g).max() <= 1e-12 * max(np.abs(x).max() for x in want.values()), k
            continue
        _equal(R["grads"][k].val, g, k, R["grads"][k].tm)
    for k, ref in R["buffers"].items():
        if k.endswith("num_batches_tracked"):
            assert ref == int(G31[f"{case}.{k}"])
        else:
            _equal(ref.val, G31[f"{case}.{k}"], k)
    whole = TN.run(sd, G31[f"{case}.v"], G31[f"{case}.a"], G31[f"{case}.d_out"], momentum=CS.MOMENTUM, eps=CS.EPS, propagate=True)
    assert TN.compare(G31[f"{case}.out32"], whole["out"]) <= 1.0   # the reference's fp32 run: inside the whole-chain bound


def _cases():
    return [(name, n) for name in CS.CONFIGS for n in CS.EXACT_N] + [("et", n) for n in CS.RAGGED_N]


def test_seeds_keep_the_bounds_non_vacuous():
    """with the restatement ALONE: every exact and ragged scene the GPU tests use, none filtered out.  No kept PReLU input
    lies within its own step's bound of 0; every per-channel 1 / sqrt(var + eps) is determined to 1e-3 of itself; no multi-element
    gradient's bound reaches half of the tensor's largest entry (the exact-zero tensors excepted)."""
    for name, n in _cases():
        sd = CS.state(CS.module(name))
        (v, a), d_out = CS.scene(name, n), CS.d_out(name, n)
        R = TN.run(sd, v, a, d_out, momentum=CS.MOMENTUM, eps=CS.EPS)
        assert R["decisions"]["prelu"]["undecided"] == 0 and R["decisions"]["prelu"]["entries"] > 0, (name, n)
        for st in R["kept"]["stat_fwd"]:
            # a variance near 0 is harmless as long as eps keeps 1 / sqrt(var + eps) determined: its bound stays far below it
            # (n = 1 has L = 0, the gcn output and its variance are exactly 0 there, and only there)
            assert (st.err[2] <= 1e-3 * st.val[2]).all() and (n == 1 or (st.val[1] > 0).all()), (name, n, st.val[1].min())
        assert not TN.vacuous(sd, R["grads"], n), (name, n, TN.vacuous(sd, R["grads"], n))
        for k in TN.exact_zero_names(sd):
            assert not R["grads"][k].val.any() and not R["grads"][k].err.any()


def test_kernel_laplacian_is_the_bridges():
    """the float32 Laplacian in the scene kernel's own order is the bridge's float64 one to float32 rounding"""
    v, a = CS.scene("et", 5)
    d, L = CS.kernel_laplacian(v)
    assert L.dtype == np.float32 and np.abs(L - a).max() <= 8 * 2.0 ** -24 * np.abs(a).max()


def _family(**kw):
    import eigentrajectory_amd as ET
    return ET.SocialSTGCNN(**{**CS.module_kw("et"), **kw})


def test_enable_native_training_contract():
    import eigentrajectory_amd as ET
    from eigentrajectory_amd._lib import ETLibraryError
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.gpgraph import GPGraphSTGCNN
    from eigentrajectory_amd.utils import default_hyper_params
    a, b = CS.module("et"), CS.module("et")
    keys = sorted(a.state_dict())
    assert a.native_training is False and "native_training" not in vars(a)
    assert ET.enable_native_training(a) is a and a.native_training is True and b.native_training is False  # per instance
    assert sorted(a.state_dict()) == keys and not any("native" in k for k in keys)
    assert "native_training" not in dict(a.named_buffers()) and "native_training" not in dict(a.named_parameters())
    v, adj = torch.zeros((1, 1, 8, 3)), torch.zeros((8, 3, 3))
    before = CS.state(a)
    with pytest.raises(RuntimeError, match="training-mode forward and backward are not implemented"):
        b(v, adj)   # without the flag: as before
    with pytest.raises(ETLibraryError, match="no CPU path"):
        a(v, adj)   # with it: the library is reached
    with pytest.raises(ETLibraryError, match="no CPU path"):
        a.eval()(v, adj)   # eval mode: the inference path, whatever the flag
    with pytest.raises(RuntimeError, match="no input gradient"):
        a.train()(v.clone().requires_grad_(True), adj)
    assert all(np.array_equal(before[k], t) for k, t in CS.state(a).items())
    assert ET.enable_native_training(a, False) is a and a.native_training is False
    with pytest.raises(RuntimeError, match="training-mode forward and backward are not implemented"):
        a(v, adj)
    wrapped = ET.EigenTrajectory(CS.module("et"), get_hook_func("stgcnn"), default_hyper_params(static_dist=0.3))
    assert ET.enable_native_training(wrapped) is wrapped and wrapped.baseline_model.native_training is True
    for name in CS.CONFIGS:
        assert CS.module(name).outside_native_training() is None, name
    names = ("LBEBM", "PECNet", "SocialImplicitLight", "SGCN", "SocialSTGCNN")

    def bn_edit(field, value, which="tcn.0"):
        m = _family()
        blk = m.st_gcns[0]
        setattr({"tcn.0": blk.tcn[0], "tcn.3": blk.tcn[3], "residual.1": blk.residual[1]}[which], field, value)
        return m

    no_affine = _family()
    no_affine.st_gcns[0].tcn[3] = torch.nn.BatchNorm2d(20, affine=False)
    no_stats = _family()
    no_stats.st_gcns[0].residual[1] = torch.nn.BatchNorm2d(20, track_running_stats=False)
    dropped = _family()
    dropped.st_gcns[0].tcn[4].p = 0.1
    for m, field in ((_family(n_stgcnn=2), "n_stgcnn"), (_family(graph_per_time_row=True), "graph_per_time_row"),
                     (_family(input_feat=2), "input_feat"), (_family(kernel_size=5), "kernel_size"),
                     (_family(seq_len=9), "seq_len"), (_family(n_txpcnn=9), "n_txpcnn"), (_family(output_feat=65), "output_feat"),
                     (_family(pred_seq_len=33, seq_len=35), "pred_seq_len"), (no_affine, "tcn.3.affine"),
                     (no_stats, "residual.1.track_running_stats"), (bn_edit("momentum", None), "tcn.0.momentum"),
                     (bn_edit("momentum", 0.2, "tcn.3"), "momentum differs"), (bn_edit("eps", 1e-3, "residual.1"), "eps differs"),
                     (dropped, "tcn.4.p")):
        with pytest.raises(NotImplementedError, match="SocialSTGCNN has no native backward pass outside its native family: ") as exc:
            ET.enable_native_training(m)
        assert field in str(exc.value) and all(nm in str(exc.value) for nm in names), (field, str(exc.value))
        assert m.native_training is False
    with pytest.raises(NotImplementedError, match="out of scope"):
        ET.enable_native_training(_family(n_stgcnn=2))
    with pytest.raises(NotImplementedError, match="GPGraph has no native backward pass") as exc:
        ET.enable_native_training(GPGraphSTGCNN(obs_len=8, pred_len=6, in_dims=1, out_dims=20))
    assert "BatchNorm" in str(exc.value) and "per-time-row" in str(exc.value)
    assert a.unused_parameter_names() == {"tpcnns.4.weight", "tpcnns.4.bias", "prelus.4.weight"}
    assert CS.module("tp1").unused_parameter_names() == set()
    assert CS.module("tp2").unused_parameter_names() == {"tpcnns.1.weight", "tpcnns.1.bias", "prelus.1.weight"}


def _params(S=20, k=6, n_tp=5, **kw):
    """et_stgcnn_params whose every pointer is a (never dereferenced) non-NULL host address"""
    from eigentrajectory_amd import _lib
    p = _lib.STGCNNParams()
    p.n_stgcnn, p.n_txpcnn, p.input_feat, p.output_feat, p.seq_len, p.pred_seq_len, p.kernel_size = 1, n_tp, 1, S, k + 2, k, 3
    p.bn_eps = 1e-5
    ly = p.st_gcns[0]
    for f, _ in _lib.STGCNNLayer._fields_:
        if S != 1 or not f.startswith("res_"):
            setattr(ly, f, 8)
    for j in range(max(1, n_tp - 1)):
        p.tpcnn_w[j] = p.tpcnn_b[j] = p.prelus[j] = 8
    p.out_w = p.out_b = 8
    for key, val in kw.items():
        setattr(p, key, val)
    return p


def _train(S=20, momentum=0.1, **kw):
    from eigentrajectory_amd import _lib
    t = _lib.STGCNNTrain()
    t.momentum = momentum
    for f, _ in _lib.STGCNNTrain._fields_[1:]:
        if S != 1 or not f.startswith("res_"):
            setattr(t, f, 8)
    for key, val in kw.items():
        setattr(t, key, val)
    return t


def test_arguments_are_validated_on_the_host():
    """every refusal below is answered before a launch: the calls run without a device"""
    from eigentrajectory_amd import _lib
    lib = _lib.lib()
    UNSUPPORTED, INVALID, WORKSPACE = (H.defines()[k] for k in ("ET_ERR_UNSUPPORTED", "ET_ERR_INVALID_ARG", "ET_ERR_WORKSPACE"))
    big = 1 << 40
    G_ = int(lib.et_stgcnn_grad_floats(C.byref(_params())))
    assert G_ == sum(q.numel() for q in CS.module("et").parameters())
    for name in CS.CONFIGS:
        n_tp, S, k = CS.CONFIGS[name]
        assert int(lib.et_stgcnn_grad_floats(C.byref(_params(S, k, n_tp)))) == sum(q.numel() for q in CS.module(name).parameters())
    need = int(lib.et_stgcnn_train_workspace_bytes(C.byref(_params()), 3, 1))
    assert need > 0 and need % 4 == 0
    assert int(lib.et_stgcnn_train_workspace_bytes(C.byref(_params()), 3, 2)) == need + 4 * (15 * 20 + G_)

    def graph(p, n=3, d=8, grads=8, gf=G_, ws=8, nbytes=big, **_):
        return lib.et_stgcnn_backward_graph(C.byref(p), n, d, grads, gf, ws, nbytes, None)

    def scenes(p, n=3, off=None, ns=0, d=8, grads=8, gf=G_, ws=8, nbytes=big, **_):
        return lib.et_stgcnn_backward_scenes(C.byref(p), n, off, ns, d, grads, gf, ws, nbytes, None)

    def fwd_graph(p, t=None, v=8, a=8, n=3, out=8, ws=8, nbytes=big):
        return lib.et_stgcnn_train_forward_graph(C.byref(p), C.byref(t or _train()), v, a, n, out, ws, nbytes, None)

    def fwd_scenes(p, t=None, c=8, nrm=8, n=3, off=None, ns=0, out=8, ws=8, nbytes=big):
        return lib.et_stgcnn_train_forward_scenes(C.byref(p), C.byref(t or _train()), c, nrm, n, off, ns, out, ws, nbytes, None)

    for call in (graph, scenes, fwd_graph, fwd_scenes):
        for bad in (dict(n_stgcnn=2), dict(input_feat=2), dict(kernel_size=5), dict(n_txpcnn=9), dict(n_txpcnn=0),
                    dict(pred_seq_len=33, seq_len=35), dict(seq_len=9), dict(output_feat=65), dict(output_feat=0)):
            assert call(_params(**bad)) == UNSUPPORTED, (call.__name__, bad)
        p = _params()
        p.st_gcns[0].bn2_w = None
        assert call(p) == INVALID
        assert call(_params(), ws=None) == WORKSPACE and call(_params(), nbytes=need - 1) == WORKSPACE
        assert call(_params(), n=-1) == INVALID
    assert graph(_params(), n=_lib.SCENE_MAX_N + 1) == INVALID and fwd_graph(_params(), n=_lib.SCENE_MAX_N + 1) == INVALID
    assert graph(_params(), d=None) == INVALID and graph(_params(), grads=None) == INVALID and graph(_params(), gf=G_ - 1) == INVALID
    assert scenes(_params(), d=None) == INVALID and scenes(_params(), grads=None) == INVALID and scenes(_params(), gf=3) == INVALID
    assert scenes(_params(), off=8, ns=0) == INVALID and fwd_scenes(_params(), off=8, ns=0) == INVALID
    assert fwd_graph(_params(), v=None) == INVALID and fwd_graph(_params(), a=None) == INVALID
    assert fwd_graph(_params(), out=None) == INVALID and fwd_graph(_params(), n=0) == 0   # an empty scene: a no-op
    assert fwd_scenes(_params(), c=None) == INVALID and fwd_scenes(_params(), nrm=None) == INVALID
    assert fwd_scenes(_params(), out=None) == INVALID
    for call in (fwd_graph, fwd_scenes):
        for bad in (dict(momentum=-0.1), dict(momentum=1.5), dict(momentum=float("nan")), dict(bn1_mean=None),
                    dict(bn2_var=None), dict(res_bn_mean=None), dict(bn1_batches=None), dict(res_bn_batches=None)):
            assert call(_params(), t=_train(**bad)) == INVALID, (call.__name__, bad)
        assert call(_params(1, 1, 3), t=_train(S=20)) == INVALID   # output_feat = 1 has no residual.1
        assert call(_params(1, 1, 3), t=_train(S=1), nbytes=0) == WORKSPACE
    assert lib.et_stgcnn_backward_graph(None, 3, 8, 8, G_, 8, big, None) == INVALID
    assert lib.et_stgcnn_train_forward_graph(C.byref(_params()), None, 8, 8, 3, 8, 8, big, None) == INVALID
    assert lib.et_stgcnn_train_workspace_bytes(C.byref(_params(n_stgcnn=2)), 3, 1) == 0
    assert lib.et_stgcnn_train_workspace_bytes(C.byref(_params()), 0, 1) == 0
    assert lib.et_stgcnn_train_workspace_bytes(C.byref(_params()), 3, 0) == 0
    assert lib.et_stgcnn_grad_floats(C.byref(_params(n_stgcnn=2))) == 0


def test_abi_names_declared_and_mirrored():
    from eigentrajectory_amd import _lib, ops
    header = H.text()
    for name in ("et_stgcnn_train_workspace_bytes", "et_stgcnn_grad_floats", "et_stgcnn_train_layout",
                 "et_stgcnn_train_forward_graph", "et_stgcnn_train_forward_scenes", "et_stgcnn_backward_graph",
                 "et_stgcnn_backward_scenes"):
        assert re.search(rf"\b{name}\(", header) and name in _lib.SYMBOLS and hasattr(_lib.lib(), name), name
    d = H.defines()
    assert d["ET_STGCNN_TRAIN_LAYOUT_FIELDS"] == _lib.STGCNN_TRAIN_LAYOUT_FIELDS and d["ET_ABI_VERSION"] == 3
    assert H.struct_fields("et_stgcnn_train") == [f for f, _ in _lib.STGCNNTrain._fields_]
    assert H.struct_fields("et_stgcnn_layer") == [f for f, _ in _lib.STGCNNLayer._fields_]   # unchanged
    assert H.struct_fields("et_stgcnn_params") == [f for f, _ in _lib.STGCNNParams._fields_]
    assert C.sizeof(_lib.STGCNNTrain) == 8 + 9 * 8
    off = (C.c_int64 * _lib.STGCNN_TRAIN_LAYOUT_FIELDS)()
    lib, p = _lib.lib(), _params()
    assert lib.et_stgcnn_train_layout(C.byref(p), 3, 1, off, _lib.STGCNN_TRAIN_LAYOUT_FIELDS) == 0
    o = list(off)
    K, S, k = 8, 20, 6
    assert o[:20] == sorted(o[:20]) and o[0] == 0 and o[1] == K and o[2] == 2 * K and o[3] == 2 * K + K * (K + 1)
    assert o[20] == 2 * K + K * (K + 1) + 14 * S * K + (2 * 2 * 4 + 1) * k * S       # floats per pedestrian
    assert o[21] == 3 * o[20] and o[22] == 15 * S and o[23] == o[21] + o[22] and o[24] == lib.et_stgcnn_grad_floats(C.byref(p))
    assert o[25] == o[23] + o[24] and o[25] * 4 == lib.et_stgcnn_train_workspace_bytes(C.byref(p), 3, 1)
    assert lib.et_stgcnn_train_layout(C.byref(p), 3, 1, off, 5) == d["ET_ERR_INVALID_ARG"]
    assert lib.et_stgcnn_train_layout(C.byref(_params(n_stgcnn=2)), 3, 1, off, 26) == d["ET_ERR_UNSUPPORTED"]
    for fn in ("stgcnn_train_workspace", "stgcnn_train_forward_graph", "stgcnn_train_forward_scenes", "stgcnn_backward_graph",
               "stgcnn_backward_scenes", "stgcnn_grad_views", "stgcnn_train_views"):
        assert callable(getattr(ops, fn))
