"""CPU checks of the native PECNet / LBEBM predictors (eigentrajectory_amd/pecnet.py, lbebm.py, csrc/et_mlp.hip): the numpy
restatement (tests/_pecnet_np.py) against the reference's recorded outputs (tests/golden/g24_pecnet.npz,
tools/make_golden_pecnet.py), the seeded weights, the state_dict contract, what raises, the bridges, the dispatch of
evaluate_split and the argument checks of the C entry points (none of which launches anything)."""
import ctypes as C

import numpy as np
import pytest
import torch

from . import _abi_header as H
from . import _golden as G
from . import _pecnet_np as PN

Z = G.load("g24_pecnet.npz")
CFGS = ["pecnet", "lbebm", "pecnet_gen", "lbebm_gen"]
TAGS = sorted({k.split(".")[0] for k in Z.files if k.startswith("pick")}, key=lambda t: int(t[4:])) + ["single", "block",
                                                                                                      "zerorow"]
TOL = 1e-5
module = PN.native_module


def scale_err(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def call_inputs(cfg, tag):
    k = int(Z[f"{cfg}.k"])
    u = Z[f"{tag}.u"]
    n = u.shape[1]
    mask = Z[f"{tag}.mask"] if f"{tag}.mask" in Z.files else np.ones((n, n), np.bool_)
    return np.ascontiguousarray(u[:k].T), np.ascontiguousarray(u[-2:].T), mask


@pytest.mark.parametrize("cfg", CFGS)
def test_restatement_equals_every_recorded_output(cfg):
    sd = PN.weights(Z, cfg)
    S = int(Z[f"{cfg}.S"])
    pools = {"pecnet": 3, "pecnet_gen": 2}.get(cfg, 0)
    worst = 0.0
    for tag in TAGS:
        past, ori, mask = call_inputs(cfg, tag)
        got = PN.pecnet_predict(sd, past, ori, mask, ori, pools) if pools else PN.lbebm_predict(sd, past, ori)
        err = scale_err(got, Z[f"{cfg}.{tag}.out"])
        worst = max(worst, err)
        assert err <= TOL, (tag, err)
        assert scale_err(PN.post_hook(got, S), Z[f"{cfg}.{tag}.c_pred_refine"]) <= TOL
        if pools and past.shape[0] >= 8:  # the fixture tells a softmax from uniform attention
            assert scale_err(PN.pecnet_predict(sd, past, ori, mask, ori, pools, uniform=True), Z[f"{cfg}.{tag}.out"]) > 100 * TOL
    print(f"{cfg}: {worst:.2e}; the reference's own fp32 rounding {float(Z['ref_fp32_err']):.2e}")
    assert float(Z["ref_fp32_err"]) <= 2.5e-6


def test_scene_restatement_is_the_module_restatement_under_an_all_ones_mask():
    sd = PN.weights(Z, "pecnet_gen")
    u = Z["pick3.u"][[0, 1, 2, 3, 6, 7]]
    got = PN.scene_forward("pecnet", sd, u, 2, 3)
    assert scale_err(got, Z["pecnet_gen.pick3.c_pred_refine"]) <= TOL
    nrm = np.vstack([u[4:] + np.float32(3.0), np.zeros_like(u[4:])])
    assert np.abs(PN.scene_input(u[:4], nrm, 0, u.shape[1])[4:] - u[4:]).max() <= 1e-5


@pytest.mark.parametrize("cfg", CFGS)
def test_seeded_weights_reproduce_the_stored_sums(cfg):
    keys, shapes = PN.shapes_of(Z, cfg)
    sd = PN.make_weights(keys, shapes, Z[f"{cfg}.seed"], Z[f"{cfg}.factor"])
    PN.check_weights(Z, cfg, sd)
    assert all(sd[k].dtype == np.float32 and sd[k].shape == s for k, s in zip(keys, shapes))
    other = PN.make_weights(keys, shapes, int(Z[f"{cfg}.seed"]) + 1, Z[f"{cfg}.factor"])
    with pytest.raises(AssertionError, match="regenerate"):
        PN.check_weights(Z, cfg, other)


@pytest.mark.parametrize("cfg", CFGS)
def test_native_module_has_the_recorded_keys_and_loads_strictly(cfg):
    m = module(cfg)
    keys, shapes = PN.shapes_of(Z, cfg)
    sd = m.state_dict()
    assert list(sd) == keys and [tuple(v.shape) for v in sd.values()] == shapes
    m.load_state_dict({k: torch.from_numpy(v) for k, v in PN.weights(Z, cfg).items()}, strict=True)
    assert "encoder_past.layers.0.weight" in sd and "non_local_g.layers.2.bias" in sd and "decoder.layers.1.weight" in sd
    if cfg.startswith("lbebm"):
        assert {"EBM.0.weight", "EBM.2.weight", "EBM.4.bias"} <= set(sd)


def test_a_reference_checkpoint_loads_through_the_wrapper():
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    for cfg in ("pecnet_gen", "lbebm_gen"):
        model = EigenTrajectory(module(cfg), get_hook_func(cfg.split("_")[0]), default_hyper_params(static_dist=0.3))
        ckpt = {k: v.clone() for k, v in model.state_dict().items() if not k.startswith("baseline_model.")}
        w = PN.weights(Z, cfg)
        ckpt.update({"baseline_model." + k: torch.from_numpy(v) for k, v in w.items()})
        model.load_state_dict(ckpt, strict=True)
        assert torch.equal(model.baseline_model.predictor.layers[2].bias, torch.from_numpy(w["predictor.layers.2.bias"]))


def test_what_is_not_native_raises():
    from eigentrajectory_amd._lib import ETLibraryError
    for cfg in ("pecnet_gen", "lbebm_gen"):
        m = module(cfg)
        past, ori = torch.zeros(3, 4), torch.zeros(3, 2)
        args = (past, ori, torch.ones(3, 3), ori) if cfg.startswith("pecnet") else (past, ori)
        with pytest.raises(NotImplementedError, match="only predict"):
            m(past, ori)
        assert m.training
        with pytest.raises(RuntimeError, match="eval"):
            m.predict(*args)
        m.eval()
        with pytest.raises(ETLibraryError, match="no CPU path"):
            m.predict(*args)
        m.predictor.activation_name = "sigmoid"
        with pytest.raises(ETLibraryError, match="activation"):
            m.predict(*args)
    from eigentrajectory_amd.pecnet import MLP
    bad = MLP(4, 2, (8,), activation="sigmoid")
    with pytest.raises(ETLibraryError, match="activation"):
        bad.et_chain(None, "MLP")
    for kw in (dict(discrim=True), dict(dropout=0.5)):
        with pytest.raises(ETLibraryError, match="native"):
            MLP(4, 2, (8,), **kw).et_chain(None, "MLP")


class _Recorder(torch.nn.Module):
    def __init__(self, out):
        super().__init__()
        self.out, self.seen = out, None

    def predict(self, *args):
        self.seen = args
        return self.out


@pytest.mark.parametrize("name", ["pecnet", "lbebm"])
def test_bridge_calls_predict_and_the_post_hook_lays_out_c_pred_refine(name):
    from eigentrajectory_amd.bridges import get_hook_func
    hooks = get_hook_func(name)
    u = torch.from_numpy(Z["pick2.u"])
    n = u.shape[1]
    info = {"scene_mask": torch.ones(n, n, dtype=torch.bool), "num_samples": 20}
    rec = _Recorder(torch.from_numpy(Z[f"{name}.pick2.out"]))
    net_in = hooks.model_forward_pre_hook(u[:6], u[6:], info)
    out = hooks.model_forward(net_in, rec)
    assert len(rec.seen) == (4 if name == "pecnet" else 2)
    assert torch.equal(rec.seen[0], u[:6].T) and torch.equal(rec.seen[1], u[6:].T)
    if name == "pecnet":
        assert rec.seen[2] is info["scene_mask"] and torch.equal(rec.seen[3], u[6:].T)
    assert torch.equal(hooks.model_forward_post_hook(out, info), torch.from_numpy(Z[f"{name}.pick2.c_pred_refine"]))


def test_evaluate_split_dispatch():
    """the new pairings get past the dispatch (and stop at the missing device); a PECNet under the lbebm hooks does not"""
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd._lib import ETLibraryError
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    obs, pred = torch.zeros(3, 8, 2), torch.zeros(3, 12, 2)
    for cfg, hooks in (("pecnet_gen", "pecnet"), ("lbebm_gen", "lbebm")):
        model = EigenTrajectory(module(cfg), get_hook_func(hooks), default_hyper_params(static_dist=0.3)).eval()
        with pytest.raises((ETLibraryError, RuntimeError, ValueError)) as exc:
            model.evaluate_split(obs, pred, [[0, 3]])
        assert not isinstance(exc.value, NotImplementedError)
        model.train()
        with pytest.raises(RuntimeError, match="training mode"):
            model.evaluate_split(obs, pred, [[0, 3]])
    for cfg, hooks in (("pecnet_gen", "lbebm"), ("lbebm_gen", "pecnet"), ("pecnet_gen", "stgcnn")):
        model = EigenTrajectory(module(cfg), get_hook_func(hooks), default_hyper_params(static_dist=0.3)).eval()
        with pytest.raises(NotImplementedError, match="pecnet"):
            model.evaluate_split(obs, pred, [[0, 3]])


def _params(pecnet=True, **kw):
    """et_mlp_params of the ET configuration whose every pointer is a (never dereferenced) non-NULL host address"""
    from eigentrajectory_amd import _lib
    p = _lib.MLPParams()
    p.fdim, p.nonlocal_pools, p.non_local_dim, p.out_width, p.pos_width = 16, 3 if pecnet else 0, 128, 120, 2 if pecnet else 0
    F = 34 if pecnet else 32
    chains = dict(encoder_past=[6, 512, 256, 16], encoder_dest=[2, 8, 16, 16], predictor=[F, 1024, 512, 256, 120])
    if pecnet:
        chains.update(non_local_theta=[F, 256, 128, 64, 128], non_local_phi=[F, 256, 128, 64, 128],
                      non_local_g=[F, 256, 128, 64, F])
    chains.update({k: v for k, v in kw.items() if k in chains})
    for name, widths in chains.items():
        c = getattr(p, name)
        c.n_layers = len(widths) - 1
        for i, w in enumerate(widths[:_lib.MLP_MAX_LAYERS + 1]):
            c.widths[i] = w
        for i in range(min(c.n_layers, _lib.MLP_MAX_LAYERS)):
            c.w[i] = c.b[i] = 8
    for k, v in kw.items():
        if k not in chains:
            setattr(p, k, v)
    return p


def test_c_entry_points_check_their_arguments_before_any_launch():
    from eigentrajectory_amd import _lib
    lib = _lib.lib()
    INVALID, UNSUPPORTED, WORKSPACE = 1, 3, 4  # ET_ERR_INVALID_ARG, ET_ERR_UNSUPPORTED, ET_ERR_WORKSPACE

    def predict(p, pecnet=True, n=3):
        if pecnet:
            return lib.et_pecnet_predict(C.byref(p), 8, 8, None, 8, n, 8, None, 0, None)
        return lib.et_lbebm_predict(C.byref(p), 8, 8, n, 8, None, 0, None)

    def scenes(p, pecnet=True, n=3):
        fn = lib.et_pecnet_forward_scenes if pecnet else lib.et_lbebm_forward_scenes
        return fn(C.byref(p), 8, 8, n, None, 0, 8, None, None, 0, None)

    for pecnet in (True, False):
        for call in (predict, scenes):
            F = 34 if pecnet else 32
            assert call(_params(pecnet, predictor=[F, 2048, 120]), pecnet) == UNSUPPORTED            # a width of 2048
            assert call(_params(pecnet, predictor=[F, 8, 8, 8, 8, 8, 120]), pecnet) == UNSUPPORTED   # five hidden layers
            assert call(_params(pecnet, encoder_past=[6, 512, 17]), pecnet) == UNSUPPORTED           # not fdim wide
            assert call(_params(pecnet, out_width=119), pecnet) == UNSUPPORTED
            assert call(_params(pecnet, nonlocal_pools=9), pecnet) == UNSUPPORTED
            assert call(_params(pecnet, pos_width=1), pecnet) == UNSUPPORTED
            p = _params(pecnet)
            p.predictor.w[1] = None
            assert call(p, pecnet) == INVALID
            assert call(_params(pecnet), pecnet, n=0) == 0      # nothing to do
            assert call(_params(pecnet), pecnet, n=-1) == INVALID
            assert call(_params(pecnet), pecnet) == WORKSPACE   # refused before the launch
    assert predict(_params(True), n=_lib.MLP_MAX_RANGE + 1) == UNSUPPORTED
    assert predict(_params(True, nonlocal_pools=0), n=_lib.MLP_MAX_RANGE + 1) == WORKSPACE  # no pooling, no range limit
    assert lib.et_pecnet_predict(None, 8, 8, None, 8, 3, 8, None, 0, None) == INVALID
    assert scenes(_params(True, encoder_dest=[4, 8, 16, 16])) == UNSUPPORTED  # the scene form's dest is obs_ori
    ws = lambda p, n, pecnet=True: int((lib.et_pecnet_workspace_bytes if pecnet else lib.et_lbebm_workspace_bytes)(C.byref(p), n))
    assert ws(_params(True), 0) == 0 and ws(_params(True, out_width=119), 100) == 0
    assert ws(_params(True), 100) == 4 * 100 * (16 + 16 + 2 + 128 + 128 + 34 + 34 + 34)
    assert ws(_params(False), 100, False) == 4 * 100 * (16 + 16 + 2)
    assert ws(_params(False), 100, True) == 0  # an LBEBM parameter block is no PECNet


def test_abi_names_declared_and_mirrored():
    from eigentrajectory_amd import _lib
    protos, d = H.functions(), H.defines()
    for name in ("et_pecnet_workspace_bytes", "et_pecnet_predict", "et_pecnet_forward_scenes", "et_lbebm_workspace_bytes",
                 "et_lbebm_predict", "et_lbebm_forward_scenes"):
        assert name in protos and name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    for struct, mirror in (("et_mlp_chain", _lib.MLPChain), ("et_mlp_params", _lib.MLPParams)):
        assert H.struct_fields(struct) == [f[0] for f in mirror._fields_], struct
    assert (d["ET_MLP_MAX_LAYERS"], d["ET_MLP_MAX_WIDTH"], d["ET_MLP_MAX_POOLS"], d["ET_MLP_MAX_RANGE"]) == (
        _lib.MLP_MAX_LAYERS, _lib.MLP_MAX_WIDTH, _lib.MLP_MAX_POOLS, _lib.MLP_MAX_RANGE)
    assert d["ET_ABI_VERSION"] == 3
    assert C.sizeof(_lib.MLPChain) == 4 * 7 + 4 + 2 * 5 * 8 and C.sizeof(_lib.MLPParams) == 5 * 4 + 4 + 6 * C.sizeof(_lib.MLPChain)
