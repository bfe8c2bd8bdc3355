"""CPU checks of the native AgentFormer predictor (eigentrajectory_amd/agentformer.py, csrc/et_agentformer.hip): the numpy
restatement (tests/_agentformer_np.py) against the reference's recorded outputs (tests/golden/g26_agentformer_net.npz,
tools/make_golden_agentformer_net.py), its k-pass form against its one-pass form, the mutants, the helper's CONFIGS (each
inside the family, the mutants visible at each, float32 mode within TOL of float64), the module's state_dict
against the reference's key and shape lists, the positional rows, what raises, the dispatch of evaluate_split and the entry
points' argument validation (host side, before any device work)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from . import _abi_header as H
from . import _agentformer_np as AN
from . import _golden as G

Z = G.load("g26_agentformer_net.npz")
ET_SCENES = ["univ57", "univ_mid", "n1", "n2", "n16", "n17", "n128"]
GEN_SCENES = ["n1", "n2", "n16", "n17"]
GEN = dict(tf_model_dim=64, tf_nhead=4, tf_ff_dim=96, context_encoder={"nlayer": 1}, future_decoder={"nlayer": 3})
TOL = 1e-5  # of the largest entry, the project's bound for a fp32 result against fp64


def keys_shapes(tag):
    return AN.fixture_keys_shapes(Z, tag)


def weights(tag):
    return AN.fixture_weights(Z, tag)


def module(tag="et"):
    from eigentrajectory_amd.agentformer import AgentFormerLight, et_config
    return AgentFormerLight(et_config(6, 20) if tag == "et" else et_config(4, 3, **GEN))


def torch_state(tag, net):
    """the drawn weights as a state_dict for ``net`` (the pe buffers are the module's own)"""
    own = net.state_dict()
    return {k: own[k] if v is None else torch.from_numpy(v) for k, v in weights(tag).items()}


def scale_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref))
    return float(np.nanmax(np.abs(got - ref)) / np.nanmax(np.abs(ref)))


def test_fixture_covers_the_cases_the_tests_need():
    assert Z["et.univ57.u"].shape == (8, 57) and 17 <= Z["et.univ_mid.u"].shape[1] <= 31
    assert [Z[f"et.n{n}.u"].shape for n in (1, 2, 16, 17, 128)] == [(8, n) for n in (1, 2, 16, 17, 128)]
    assert all(Z[f"et.{s}.seq_out"].shape == (6, Z[f"et.{s}.u"].shape[1], 20) for s in ET_SCENES)
    assert all(Z[f"gen.{s}.seq_out"].shape == (4, Z[f"gen.{s}.u"].shape[1], 3) for s in GEN_SCENES)
    assert float(Z["ref_fp32_err"].max()) <= 2.5e-6 and len(Z["ref_fp32_err"]) == len(ET_SCENES) + len(GEN_SCENES)
    keys, _ = keys_shapes("et")
    sd = weights("et")
    # no two layers alike, no bias at zero: a swapped layer or a dropped bias changes the output
    for stem in ("context_encoder.tf_encoder.layers.", "future_decoder.tf_decoder.layers."):
        for k0 in [k for k in keys if k.startswith(stem + "0.")]:
            assert not np.array_equal(sd[k0], sd[k0.replace(stem + "0.", stem + "1.")]), k0
    assert all(np.abs(sd[k]).min() > 0 for k in keys if k.endswith("bias"))
    for s in ("eth", "hotel", "univ"):
        n = int(Z[f"{s}.scene_size"].sum())
        assert Z[f"{s}.ade"].shape == Z[f"{s}.fde"].shape == (n,) and float(Z[f"{s}.robust"].mean()) >= 0.95
    assert np.array_equal(Z["univ.scene_index"], np.arange(0, 947, 10))


@pytest.mark.parametrize("tag,scene", [("et", s) for s in ET_SCENES] + [("gen", s) for s in GEN_SCENES])
def test_numpy_restatement_reproduces_the_reference(tag, scene):
    err = scale_err(AN.forward(weights(tag), Z[f"{tag}.{scene}.u"], int(Z[f"{tag}.nhead"])), Z[f"{tag}.{scene}.seq_out"])
    print(f"{tag}.{scene}: {err:.2e}")
    assert err <= TOL


@pytest.mark.parametrize("tag,scene", [("et", "n2"), ("et", "n17"), ("gen", "n1"), ("gen", "n16")])
def test_k_pass_form_equals_the_one_pass_form(tag, scene):
    """every pass's newest block already has the value the last pass gives it: one decoder pass is enough"""
    u, nhead = Z[f"{tag}.{scene}.u"], int(Z[f"{tag}.nhead"])
    one = AN.forward(weights(tag), u, nhead)
    assert np.abs(AN.forward(weights(tag), u, nhead, loop=True) - one).max() <= 1e-12
    # ... which is the block-causal mask's doing: without it the k-pass form differs
    assert np.abs(AN.forward(weights(tag), u, nhead, loop=True, mutant="no_causal") - one).max() > 1e-3


@pytest.mark.parametrize("mutant", AN.MUTANTS)
def test_every_mutant_misses_the_recorded_outputs(mutant):
    for tag, scene in (("et", "n1"), ("et", "n17"), ("gen", "n2")):
        ref = Z[f"{tag}.{scene}.seq_out"]
        got = AN.forward(weights(tag), Z[f"{tag}.{scene}.u"], int(Z[f"{tag}.nhead"]), mutant=mutant)
        assert np.abs(got - ref).max() / np.abs(ref).max() > 1e-3, (tag, scene)


# ------------------------------------------------------------------------- the configurations of the GPU shape tests
_REF = {}


def config_case(name, n):
    """(state_dict, u (T, n), the fp64 restatement's output) of CONFIGS[name] on one seeded scene of n, computed once"""
    if (name, n) not in _REF:
        c = AN.CONFIGS[name]
        _, sd = AN.config_module(name)
        C_obs, nrm = AN.random_scenes([n], 3 + n, c["T"] - 2)
        u = AN.scene_input(C_obs, nrm, 0, n)
        ref = AN.forward(sd, u, c["nhead"], frames=c["k"])
        ref.setflags(write=False)
        _REF[name, n] = (sd, u, ref)
    return _REF[name, n]


def test_configs_name_the_paths_they_open():
    C_ = AN.CONFIGS
    assert AN.SCENE_CONFIGS == ("min", "h3", "h6", "hd4", "hd20", "hd128", "hd256", "deep")
    assert AN.MODULE_ONLY_CONFIGS == ("long_dec", "long_enc")
    assert [C_[n]["D"] // C_[n]["nhead"] for n in AN.SCENE_CONFIGS] == [16, 16, 16, 4, 20, 128, 256, 16]
    assert [C_[n]["nhead"] % 4 for n in ("min", "h3", "h6")] == [1, 3, 2]             # three, one, two idle wavefronts
    assert [C_[n]["ff"] % 4 for n in ("min", "h3", "h6", "hd20", "hd128")] == [1, 2, 1, 0, 3]  # live k of the partial step
    assert [C_[n]["D"] // 16 for n in ("min", "h3", "hd20", "h6")] == [1, 3, 5, 6]    # column blocks, none a multiple of 8
    assert [C_[n]["S"] for n in ("min", "h3", "hd128")] == [1, 17, 64]
    assert (C_["deep"]["n_enc"], C_["deep"]["n_dec"], C_["deep"]["T"]) == (4, 4, 16)
    assert (C_["long_dec"]["T"], C_["long_dec"]["k"], C_["long_enc"]["T"], C_["long_enc"]["k"]) == (3, 16, 16, 1)


@pytest.mark.parametrize("name", list(AN.CONFIGS))
def test_every_config_is_inside_the_family_and_loads_strictly(name):
    c = AN.CONFIGS[name]
    net, sd = AN.config_module(name)  # constructs (inside the family) and loads strict=True
    assert (net.model_dim, net.nhead, net.ff_dim, net.forecast_dim) == (c["D"], c["nhead"], c["ff"], c["S"])
    assert (net.past_frames, net.future_frames) == (c["T"], c["k"])
    assert (len(net.context_encoder.tf_encoder.layers), len(net.future_decoder.tf_decoder.layers)) == (c["n_enc"], c["n_dec"])
    back = {k: v.numpy() for k, v in net.state_dict().items()}
    assert sorted(back) == sorted(sd) and all(np.array_equal(back[k], v) for k, v in sd.items() if v is not None)
    drawn = [v for v in sd.values() if v is not None]
    assert all(v.dtype == np.float32 and np.abs(v).min() > 0 for v in drawn)  # nothing left at zero
    for stem, count in ((AN.E + "tf_encoder.layers.", c["n_enc"]), (AN.F + "tf_decoder.layers.", c["n_dec"])):
        for i in range(1, count):  # no two layers alike
            for k0 in [k for k in sd if k.startswith(stem + "0.")]:
                assert not np.array_equal(sd[k0], sd[k0.replace(stem + "0.", f"{stem}{i}.")]), (k0, i)


@pytest.mark.parametrize("name", ["long_dec", "deep"])
def test_frames_k_pass_form_equals_the_one_pass_form(name):
    c = AN.CONFIGS[name]
    for n in (2, 17):
        sd, u, one = config_case(name, n)
        assert one.shape == (c["k"], n, c["S"])
        assert np.abs(AN.forward(sd, u, c["nhead"], loop=True, frames=c["k"]) - one).max() <= 1e-12
        if c["n_dec"] >= 2:  # (one decoder layer attends over embeddings only: a pass's newest block sees them all anyway)
            assert np.abs(AN.forward(sd, u, c["nhead"], loop=True, frames=c["k"], mutant="no_causal") - one).max() > 1e-3
    if name == "deep":  # frames = None is T - 2, today's behaviour
        assert np.array_equal(AN.forward(sd, u, c["nhead"]), one)


@pytest.mark.parametrize("name", list(AN.CONFIGS))
@pytest.mark.parametrize("mutant", AN.MUTANTS)
def test_every_mutant_misses_the_restatement_at_every_config(mutant, name):
    """by more than 100 TOL on scenes of 2 and 17.  Where a mutant cannot be expressed (layers 0 and 1 swapped with one
    layer a side, no causal mask over one decoder frame: AN.vacuous) it must be the identity instead."""
    c = AN.CONFIGS[name]
    for n in (2, 17):
        sd, u, ref = config_case(name, n)
        got = AN.forward(sd, u, c["nhead"], frames=c["k"], mutant=mutant)
        miss = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"{name} {mutant} n={n}: {miss:.2e}")
        if AN.vacuous(mutant, name):
            assert miss == 0.0, (name, mutant, n)
        else:
            assert miss > 100 * TOL, (name, mutant, n, miss)


@pytest.mark.parametrize("name", list(AN.CONFIGS))
def test_float32_mode_is_float32_and_within_tol_of_float64(name):
    """the reference arithmetic's own error (measured 1.2e-7 .. 6.1e-7 of the largest entry over all configurations)"""
    c = AN.CONFIGS[name]
    for n in (1, 2, 17):
        sd, u, ref = config_case(name, n)
        stats = {}
        got = AN.forward(sd, u, c["nhead"], frames=c["k"], dtype=np.float32, stats=stats)
        assert got.dtype == np.float32 and ref.dtype == np.float64 and got.shape == ref.shape
        assert np.isfinite(stats["max_score"])
        err = scale_err(got, ref)
        print(f"{name} n={n}: fp32 against fp64 {err:.2e}, max score {stats['max_score']:.1f}")
        assert err <= TOL, (name, n, err)


@pytest.mark.parametrize("name", AN.LARGE_LOGITS["configs"])
def test_large_logit_inputs_need_the_row_maximum(name):
    """in_proj weights x 8: the largest score passes 88.7, above which exp overflows fp32 unless the row maximum is taken
    off first.  Near-argmax attention is ill-conditioned in fp32 itself: the float32 restatement's error against fp64
    (measured 1.5e-5 at h3, 3.6e-5 at hd20; largest scores 136 and 318) is what the GPU test scales its bound from."""
    c, sizes = AN.CONFIGS[name], AN.LARGE_LOGITS["sizes"]
    _, sd = AN.config_module(name, in_proj_scale=AN.LARGE_LOGITS["scale"])
    C_obs, nrm = AN.random_scenes(sizes, AN.LARGE_LOGITS["seed"], c["k"])
    stats, lo, e32 = {}, 0, 0.0
    for n in sizes:
        u = AN.scene_input(C_obs, nrm, lo, lo + n)
        ref = AN.forward(sd, u, c["nhead"], stats=stats)
        got = AN.forward(sd, u, c["nhead"], dtype=np.float32)
        assert np.isfinite(ref).all() and np.isfinite(got).all()
        e32 = max(e32, scale_err(got, ref))
        lo += n
    print(f"{name}: max score {stats['max_score']:.1f}, fp32 against fp64 {e32:.2e}")
    assert stats["max_score"] > 88.7
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(np.float32(stats["max_score"])))


@pytest.mark.parametrize("tag", ["et", "gen"])
def test_state_dict_has_the_reference_keys_and_shapes(tag):
    keys, shapes = keys_shapes(tag)
    net = module(tag)
    own = net.state_dict()
    assert list(own) == keys
    assert [tuple(v.shape) for v in own.values()] == shapes
    net.load_state_dict(torch_state(tag, net), strict=True)
    back = {k: v.numpy() for k, v in net.state_dict().items()}
    assert all(np.array_equal(back[k], v) for k, v in weights(tag).items() if v is not None)
    # ... and the other way: a checkpoint saved from this module has exactly the recorded keys
    assert sorted(back) == sorted(keys)
    with pytest.raises(RuntimeError):
        net.load_state_dict({k: v for k, v in own.items() if not k.endswith("in_proj_bias_self")}, strict=True)


@pytest.mark.parametrize("tag", ["et", "gen"])
def test_positional_rows(tag):
    net = module(tag)
    T = Z[f"{tag}.pe_enc"].shape[0]
    for name, pe in (("pe_enc", net.context_encoder.pos_encoder.pe), ("pe_dec", net.future_decoder.pos_encoder.pe)):
        assert pe.shape == (200, 1, net.model_dim)
        assert np.abs(pe[:T, 0].numpy() - Z[f"{tag}.{name}"]).max() <= 1e-6
        assert np.abs(AN.pos_enc(T, net.model_dim) - Z[f"{tag}.{name}"]).max() <= 1e-6


def test_constructor_errors_name_the_field():
    from eigentrajectory_amd.agentformer import AgentFormerLight, et_config
    cases = [("nz", dict(nz=32)), ("learn_prior", dict(learn_prior=True)), ("input_type", dict(input_type=["scene_norm", "vel"])),
             ("pred_type", dict(pred_type="scene_norm")), ("pos_concat", dict(pos_concat=False)),
             ("use_agent_enc", dict(use_agent_enc=True)), (r"tf_cfg\.gaussian_kernel", dict(tf_cfg={"gaussian_kernel": True})),
             (r"tf_cfg\.sep_attn", dict(tf_cfg={"sep_attn": False})), ("conn_dist", dict(conn_dist=10.0)),
             (r"future_decoder\.out_mlp_dim", dict(future_decoder={"nlayer": 2, "out_mlp_dim": [512, 256]})),
             ("motion_dim", dict(motion_dim=2)), ("tf_model_dim", dict(tf_model_dim=512)), ("tf_nhead", dict(tf_nhead=3)),
             ("tf_ff_dim", dict(tf_ff_dim=1024)), (r"context_encoder\.nlayer", dict(context_encoder={"nlayer": 5})),
             ("past_frames", dict(past_frames=17)), ("forecast_dim", dict(forecast_dim=65))]
    for field, over in cases:
        with pytest.raises(ValueError, match=field):
            AgentFormerLight(et_config(6, 20, **over))

    class Namespace:  # a configuration object with attributes and the reference's get(), sub-sections as mappings
        def get(self, name, default=None):
            return getattr(self, name, default)

    ns = Namespace()
    for key, val in et_config(6, 20).items():
        setattr(ns, key, val)
    assert list(AgentFormerLight(ns).state_dict()) == keys_shapes("et")[0]
    ns.nz = 8
    with pytest.raises(ValueError, match="nz"):
        AgentFormerLight(ns)


def test_training_mode_and_cpu_forward_raise():
    from eigentrajectory_amd._lib import ETLibraryError
    net = module("gen")
    net.set_data({"pre_motion": torch.zeros(6, 3, 1)})
    assert net.training and net.data["agent_num"] == 3 and net.data["missing"] is None
    with pytest.raises(RuntimeError, match="training"):
        net()
    with pytest.raises(ETLibraryError, match="CPU"):
        net.eval()()


def test_evaluate_split_dispatch():
    """the agentformer pairing gets past the dispatch (and stops at the missing device); under other hooks it does not"""
    from eigentrajectory_amd import EigenTrajectory
    from eigentrajectory_amd._lib import ETLibraryError
    from eigentrajectory_amd.bridges import get_hook_func
    from eigentrajectory_amd.utils import default_hyper_params
    obs, pred = torch.zeros(3, 8, 2), torch.zeros(3, 12, 2)
    model = EigenTrajectory(module(), get_hook_func("agentformer"), default_hyper_params(static_dist=0.3)).eval()
    if not torch.cuda.is_available():
        with pytest.raises((ETLibraryError, RuntimeError, ValueError)) as exc:
            model.evaluate_split(obs, pred, [[0, 3]])
        assert not isinstance(exc.value, NotImplementedError)
    model.train()
    with pytest.raises(RuntimeError, match="training mode"):
        model.evaluate_split(obs, pred, [[0, 3]])
    for predictor, hooks in ((module(), "stgcnn"), (module(), "implicit"), (torch.nn.Linear(2, 2), "agentformer")):
        model = EigenTrajectory(predictor, get_hook_func(hooks), default_hyper_params(static_dist=0.3)).eval()
        with pytest.raises(NotImplementedError, match="AgentFormerLight.*'agentformer'"):
            model.evaluate_split(obs, pred, [[0, 3]])


def _params(**kw):
    """et_agentformer_params of the ET configuration whose every pointer is a (never dereferenced) non-NULL host address"""
    from eigentrajectory_amd import _lib
    p = _lib.AgentFormerParams()
    p.motion_dim, p.model_dim, p.ff_dim, p.nhead, p.forecast_dim = 1, 256, 512, 8, 20
    p.past_frames, p.future_frames, p.n_enc, p.n_dec = 8, 6, 2, 2
    dummy = 8

    def fill(struct):
        for name, ctype in struct._fields_:
            if ctype is C.c_void_p:
                setattr(struct, name, dummy)
            elif ctype is C.c_int:
                pass
            elif hasattr(ctype, "_length_"):
                arr = getattr(struct, name)
                for i in range(len(arr)):
                    if isinstance(arr[i], C.Structure):
                        fill(arr[i])
                    else:
                        arr[i] = dummy
            else:
                fill(getattr(struct, name))

    fill(p)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_arguments_are_validated_on_the_host():
    """Every refusal below is answered before a launch: the calls run without a device."""
    from eigentrajectory_amd import _lib
    lib = _lib.lib()
    UNSUPPORTED, INVALID, WORKSPACE = (H.defines()[k] for k in ("ET_ERR_UNSUPPORTED", "ET_ERR_INVALID_ARG",
                                                                "ET_ERR_WORKSPACE"))

    def graph(p):
        return lib.et_agentformer_forward_graph(C.byref(p), 8, 3, 8, 8, 1 << 30, None)

    def scenes(p):
        return lib.et_agentformer_forward_scenes(C.byref(p), 8, 8, 3, None, 0, 8, None, 8, 1 << 30, None)

    for call in (graph, scenes):
        for bad in (dict(motion_dim=2), dict(model_dim=272), dict(model_dim=40, nhead=4), dict(nhead=3), dict(model_dim=24,
                    nhead=4), dict(model_dim=32, nhead=16), dict(model_dim=96, nhead=16), dict(ff_dim=513), dict(ff_dim=0), dict(n_enc=0), dict(n_dec=5), dict(past_frames=17),
                    dict(future_frames=0), dict(forecast_dim=65), dict(forecast_dim=0)):
            assert call(_params(**bad)) == UNSUPPORTED, bad
        p = _params()
        p.dec[1].multihead_attn.in_proj_bias_self = None
        assert call(p) == INVALID
        p = _params()
        p.enc[1].norm_weight[1] = None
        assert call(p) == INVALID
        p = _params()
        p.dec_embed.pe = None
        assert call(p) == INVALID
        p = _params()
        p.enc[0].multihead_attn.in_proj_weight = None  # encoder layers have no cross-attention: not looked at
        p.enc[0].norm_bias[2] = None
        p.dec[3].linear1_weight = None                 # nor are layers past n_dec
        short = (lib.et_agentformer_forward_graph(C.byref(p), 8, 3, 8, 8, 16, None) if call is graph else
                 lib.et_agentformer_forward_scenes(C.byref(p), 8, 8, 3, None, 0, 8, None, 8, 16, None))
        assert short == WORKSPACE  # the parameters are accepted; the refusal is the short workspace's
    assert scenes(_params(past_frames=9)) == UNSUPPORTED  # u = [C_obs; obs_ori]: past_frames = future_frames + 2
    assert lib.et_agentformer_forward_graph(None, 8, 3, 8, 8, 1 << 30, None) == INVALID
    assert lib.et_agentformer_forward_graph(C.byref(_params()), None, 0, None, None, 0, None) == 0
    assert lib.et_agentformer_forward_graph(C.byref(_params()), None, 3, 8, 8, 1 << 30, None) == INVALID
    assert lib.et_agentformer_forward_graph(C.byref(_params()), 8, 3, 8, None, 0, None) == WORKSPACE
    assert lib.et_agentformer_forward_graph(C.byref(_params()), 8, _lib.AGENTFORMER_MAX_SCENE_N + 1, 8, 8, 1 << 40, None) == INVALID
    ws = lambda p, n, m=0: int(lib.et_agentformer_workspace_bytes(C.byref(p), n, m))
    assert lib.et_agentformer_forward_graph(C.byref(_params()), 8, 3, 8, 8, ws(_params(), 3) - 1, None) == WORKSPACE
    assert lib.et_agentformer_forward_scenes(C.byref(_params()), None, 8, 3, None, 0, 8, None, 8, 1 << 30, None) == INVALID
    assert lib.et_agentformer_forward_scenes(C.byref(_params()), 8, 8, 3, None, 0, 8, None, 8, ws(_params(), 3) - 1, None) == WORKSPACE
    assert lib.et_agentformer_forward_scenes(C.byref(_params()), 8, 8, 0, 8, 0, 8, None, None, 0, None) == 0
    assert lib.et_agentformer_forward_scenes(C.byref(_params()), 8, 8, 3, 8, 0, 8, None, 8, 1 << 30, None) == INVALID
    assert lib.et_agentformer_forward_scenes(C.byref(_params()), 8, 8, 129, None, 0, 8, None, 8, 1 << 40, None) == INVALID
    # workspace: per pedestrian T (1 + 7 D) + k 9 D floats, linear in N whatever the scenes; 0 outside the family
    per = 8 * (1 + 7 * 256) + 6 * 9 * 256
    assert ws(_params(), 1000) == ws(_params(), 1000, 57) == 1000 * per * 4 and ws(_params(), 0) == 0
    assert ws(_params(ff_dim=513), 1000) == 0


def test_agentformer_abi_names_declared_and_mirrored():
    from eigentrajectory_amd import _lib
    header = H.text()
    for name in ("et_agentformer_workspace_bytes", "et_agentformer_forward_graph", "et_agentformer_forward_scenes"):
        assert re.search(rf"\b{name}\(", header) and name in _lib.SYMBOLS and name in _lib.SIGNATURES, name
    for struct, mirror in (("et_agentformer_attn", _lib.AgentFormerAttn), ("et_agentformer_layer", _lib.AgentFormerLayer),
                           ("et_agentformer_embed", _lib.AgentFormerEmbed), ("et_agentformer_params", _lib.AgentFormerParams)):
        assert H.struct_fields(struct) == [f for f, _ in mirror._fields_], struct
    d = H.defines()
    assert d["ET_AGENTFORMER_MAX_LAYERS"] == _lib.AGENTFORMER_MAX_LAYERS == 4
    assert d["ET_AGENTFORMER_MAX_SCENE_N"] == _lib.AGENTFORMER_MAX_SCENE_N == 128 and d["ET_ABI_VERSION"] == 3
    assert C.sizeof(_lib.AgentFormerAttn) == 6 * 8 and C.sizeof(_lib.AgentFormerLayer) == (12 + 4 + 6) * 8
    assert C.sizeof(_lib.AgentFormerParams) == 40 + 2 * 5 * 8 + 2 * 8 + 8 * 22 * 8  # ints + padding, embeds, out_fc, layers
