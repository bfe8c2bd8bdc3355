"""AgentFormer in the ET configuration, restated in float64 numpy from the published architecture (agent-aware attention,
post-norm transformer layers, concatenated sinusoidal positions) -- the yardstick of tests/test_agentformer_cpu.py and
tests/test_gpu_agentformer.py.  Hand-written; nothing here is the reference's program text.

A scene of n pedestrians with input u (T, n): encoder tokens t n + a, x = fc(cat[input_fc(u[t, a]), pe[t]]); layers
LN(x + attn(x, x)), LN(x + W2 relu(W1 x)).  Decoder tokens t n + a for t < k, every one fed u[T-1, a] with pe[t]; layers
add LN(x + attn(x, memory)) in between; self-attention is block-causal.  score(i, j) = q_self_i . k_self_j when
i % n == j % n, else q_i . k_j; both q are scaled by head_dim^-0.5.  ``forward(..., loop=True)`` runs the decoder the way the
reference does: k passes over 1, 2, .. k frames; frame f - 1 of the result is the block pass f newly produced.
``frames`` sets the number of decoder frames apart from T (the module form allows any pair up to 16); ``dtype=np.float32``
runs the same arithmetic in float32 throughout, the measure of what fp32 itself loses.

CONFIGS names the members of the supported family that tests/test_gpu_agentformer_shapes.py runs, each chosen for a kernel
path it opens; ``module_cfg`` turns one into the module's configuration and ``random_state`` draws its weights.

MUTANTS names the switches that break one property each; the fixture tool asserts that every one of them misses the
recorded outputs by far more than the tests' tolerance."""
import numpy as np

E, F = "context_encoder.", "future_decoder."
MUTANTS = ("no_agent_aware", "no_causal", "swap_layers", "pe_shift", "q_unscaled", "dec_in_prev")


def make_weights(keys, shapes, seed):
    """every tensor its own draw from default_rng(seed): matrices uniform in +-1/sqrt(fan_in), biases non-zero, LayerNorm
    weights around 1 -- nothing left at an initialiser's value, no two layers alike.  ``pe`` buffers are not drawn (None)."""
    rng = np.random.default_rng(seed)
    out = {}
    for key, shape in zip(keys, shapes):
        shape = tuple(int(s) for s in shape)
        if key.endswith(".pe"):
            out[key] = None
        elif ".norm" in key and key.endswith(".weight"):
            out[key] = (1.0 + rng.uniform(-0.3, 0.3, shape)).astype(np.float32)
        elif len(shape) == 1:
            val = rng.uniform(0.05, 0.3, shape) * rng.choice([-1.0, 1.0], shape)
            out[key] = val.astype(np.float32)
        else:
            bound = 1.0 / np.sqrt(shape[1])
            out[key] = rng.uniform(-bound, bound, shape).astype(np.float32)
    return out


def check_weights(sd, keys, sums, rtol=1e-12):
    """the fp64 sum of every drawn tensor equals the recorded one: the generator gave the tool's weights"""
    for key, want in zip(keys, sums):
        if key.endswith(".pe"):
            continue
        got = float(np.asarray(sd[key], np.float64).sum())
        assert abs(got - want) <= rtol * max(1.0, abs(want)), (key, got, want)


_CACHE = {}


def fixture_keys_shapes(Z, tag):
    """the recorded state_dict keys (in order) and shapes of configuration ``tag`` ('et' / 'gen') of fixture ``Z``"""
    return [str(k) for k in Z[f"{tag}.keys"]], [tuple(int(v) for v in row if v) for row in Z[f"{tag}.shapes"]]


def fixture_weights(Z, tag):
    """the fixture tool's weights, drawn again from the recorded seed (once per session) and held against the recorded sums"""
    if tag not in _CACHE:
        keys, shapes = fixture_keys_shapes(Z, tag)
        sd = make_weights(keys, shapes, int(Z[f"{tag}.seed"]))
        check_weights(sd, keys, Z[f"{tag}.sums"])
        _CACHE[tag] = sd
    return _CACHE[tag]


# name: model_dim, nhead, ff, encoder + decoder layers, forecast_dim S, past_frames T, future_frames k.  Scene form needs
# T = k + 2 (u = [C_obs; obs_ori]); long_dec and long_enc exist in the module form only.
CONFIGS = {
    "min": dict(D=16, nhead=1, ff=1, n_enc=1, n_dec=1, S=1, T=3, k=1),
    "h3": dict(D=48, nhead=3, ff=30, n_enc=1, n_dec=2, S=17, T=5, k=3),
    "h6": dict(D=96, nhead=6, ff=97, n_enc=2, n_dec=1, S=5, T=6, k=4),
    "hd4": dict(D=64, nhead=16, ff=64, n_enc=1, n_dec=1, S=16, T=4, k=2),
    "hd20": dict(D=80, nhead=4, ff=100, n_enc=1, n_dec=1, S=33, T=7, k=5),
    "hd128": dict(D=256, nhead=2, ff=511, n_enc=1, n_dec=1, S=64, T=5, k=3),
    "hd256": dict(D=256, nhead=1, ff=48, n_enc=1, n_dec=1, S=7, T=4, k=2),
    "deep": dict(D=32, nhead=2, ff=40, n_enc=4, n_dec=4, S=20, T=16, k=14),
    "long_dec": dict(D=32, nhead=4, ff=40, n_enc=1, n_dec=1, S=4, T=3, k=16),
    "long_enc": dict(D=32, nhead=4, ff=40, n_enc=1, n_dec=1, S=4, T=16, k=1),
}
# scores beyond exp's fp32 range: every in_proj_weight and in_proj_weight_self times ``scale`` on scenes of ``sizes`` drawn
# by random_scenes(sizes, seed, k)
LARGE_LOGITS = dict(configs=("h3", "hd20"), scale=8, sizes=[1, 2, 17], seed=3)
SCENE_CONFIGS = tuple(name for name, c in CONFIGS.items() if c["T"] == c["k"] + 2)
MODULE_ONLY_CONFIGS = tuple(name for name in CONFIGS if name not in SCENE_CONFIGS)


def module_cfg(name):
    """the configuration mapping ``AgentFormerLight`` takes for CONFIGS[name]"""
    from eigentrajectory_amd.agentformer import et_config
    c = CONFIGS[name]
    return et_config(c["k"], c["S"], past_frames=c["T"], tf_model_dim=c["D"], tf_nhead=c["nhead"], tf_ff_dim=c["ff"],
                     context_encoder={"nlayer": c["n_enc"]}, future_decoder={"nlayer": c["n_dec"]})


def random_state(keys, shapes, seed):
    """a state_dict (numpy; ``pe`` entries None: the module keeps its own) for the given keys and shapes: make_weights'
    draw, so nothing is left at an initialiser's value and no two layers are alike"""
    return make_weights(list(keys), list(shapes), seed)


def config_module(name, seed=11, in_proj_scale=None):
    """-> (AgentFormerLight of CONFIGS[name] holding random_state's draw, loaded strict; that draw as numpy).
    in_proj_scale: every in_proj_weight and in_proj_weight_self times this (a power of two: exact), for large logits"""
    import torch
    from eigentrajectory_amd.agentformer import AgentFormerLight
    m = AgentFormerLight(module_cfg(name))
    own = m.state_dict()
    sd = random_state(list(own), [tuple(v.shape) for v in own.values()], seed)
    if in_proj_scale is not None:
        sd = {k: v * np.float32(in_proj_scale) if k.endswith(("in_proj_weight", "in_proj_weight_self")) else v
              for k, v in sd.items()}
    m.load_state_dict({k: own[k] if v is None else torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m, sd


def random_scenes(sizes, seed, k):
    """C_obs (k, N) ~ N(0, 1) and nrm (4, N) ~ N(0, 5) for scenes of the given sizes, float32"""
    rng = np.random.default_rng(seed)
    n = sum(sizes)
    return rng.normal(0, 1, (k, n)).astype(np.float32), rng.normal(0, 5, (4, n)).astype(np.float32)


def vacuous(mutant, name):
    """a mutant that cannot differ at CONFIGS[name]: swapping layers 0 and 1 where neither side has two, dropping the causal
    mask where the decoder has one frame"""
    c = CONFIGS[name]
    return (mutant == "swap_layers" and max(c["n_enc"], c["n_dec"]) < 2) or (mutant == "no_causal" and c["k"] == 1)


def pos_enc(n_rows, d_model):
    pos = np.arange(n_rows, dtype=np.float64)[:, None]
    div = np.exp(np.arange(0, d_model, 2, dtype=np.float64) * (-np.log(10000.0) / d_model))
    pe = np.zeros((n_rows, d_model))
    pe[:, 0::2], pe[:, 1::2] = np.sin(pos * div), np.cos(pos * div)
    return pe


def _ln(x, w, b):
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return (x - mu) / np.sqrt(var + x.dtype.type(1e-5)) * w + b


def _attention(g, pre, x, mem, n, nhead, causal, mut, stats=None):
    """x (Lq, D) queries' rows, mem (Lk, D) keys' rows of one scene; token i is frame i // n of pedestrian i % n"""
    D = x.shape[1]
    ninf = x.dtype.type(-np.inf)
    hd = D // nhead
    W, B, Ws, Bs = g(pre + "in_proj_weight"), g(pre + "in_proj_bias"), g(pre + "in_proj_weight_self"), \
        g(pre + "in_proj_bias_self")
    scale = x.dtype.type(1.0 if "q_unscaled" in mut else float(hd) ** -0.5)
    q = (x @ W[:D].T + B[:D]) * scale
    k = mem @ W[D:2 * D].T + B[D:2 * D]
    v = mem @ W[2 * D:].T + B[2 * D:]
    qs = (x @ Ws[:D].T + Bs[:D]) * scale
    ks = mem @ Ws[D:].T + Bs[D:]
    Lq, Lk = x.shape[0], mem.shape[0]
    same = (np.arange(Lq)[:, None] % n) == (np.arange(Lk)[None, :] % n)
    later = (np.arange(Lk)[None, :] // n) > (np.arange(Lq)[:, None] // n)
    out = np.empty((Lq, D), x.dtype)
    for h in range(nhead):
        sl = slice(h * hd, (h + 1) * hd)
        s = q[:, sl] @ k[:, sl].T
        if "no_agent_aware" not in mut:
            s = np.where(same, qs[:, sl] @ ks[:, sl].T, s)
        if causal and "no_causal" not in mut:
            s = np.where(later, ninf, s)
        if stats is not None and np.isfinite(s).any():
            stats["max_score"] = max(stats.get("max_score", -np.inf), float(s[np.isfinite(s)].max()))
        s = s - np.max(np.where(np.isnan(s), ninf, s), axis=1, keepdims=True)
        e = np.exp(s)
        out[:, sl] = (e / e.sum(axis=1, keepdims=True)) @ v[:, sl]
    return out @ g(pre + "out_proj.weight").T + g(pre + "out_proj.bias")


def _layer(g, pre, x, mem, n, nhead, decoder, mut, stats=None):
    x = _ln(x + _attention(g, pre + "self_attn.", x, x, n, nhead, decoder, mut, stats), g(pre + "norm1.weight"),
            g(pre + "norm1.bias"))
    nxt = 2
    if decoder:
        x = _ln(x + _attention(g, pre + "multihead_attn.", x, mem, n, nhead, False, mut, stats), g(pre + "norm2.weight"),
                g(pre + "norm2.bias"))
        nxt = 3
    h = np.maximum(x @ g(pre + "linear1.weight").T + g(pre + "linear1.bias"), x.dtype.type(0))
    y = h @ g(pre + "linear2.weight").T + g(pre + "linear2.bias")
    return _ln(x + y, g(f"{pre}norm{nxt}.weight"), g(f"{pre}norm{nxt}.bias"))


def _count(sd, stem):
    return len({key[len(stem):].split(".")[0] for key in sd if key.startswith(stem)})


def forward(sd, u, nhead, loop=False, mutant=(), frames=None, dtype=np.float64, stats=None):
    """sd: state_dict (numpy; the ``pe`` entries are not read), u (T, n) of ONE scene -> ``_seq_out`` (k', n, S) in ``dtype``,
    k' = ``frames``, the number of decoder frames; None: T - 2 (ET: past_frames = k + 2, future_frames = k).  dtype:
    np.float64, the yardstick, or np.float32: every array and accumulator float32 (the positional rows are formed in
    float64 and rounded once, as the module's buffer is).  stats: a dict that receives ``max_score``, the largest finite
    attention score met (before the row maximum is taken off)."""
    assert dtype in (np.float64, np.float32)
    mut = (mutant,) if isinstance(mutant, str) else tuple(mutant)
    assert all(m in MUTANTS for m in mut), mut
    sd64 = {key: np.asarray(val, dtype) for key, val in sd.items() if val is not None and not key.endswith(".pe")}
    n_enc, n_dec = _count(sd64, E + "tf_encoder.layers."), _count(sd64, F + "tf_decoder.layers.")
    swap = "swap_layers" in mut

    def layer_index(i, count):
        return {0: 1, 1: 0}.get(i, i) if swap and count >= 2 else i

    g = sd64.__getitem__
    u = np.asarray(u, dtype)
    T, n = u.shape
    k = T - 2 if frames is None else int(frames)
    assert k >= 1
    D = sd64[E + "input_fc.weight"].shape[0]
    pe = pos_enc(max(T, k) + 1, D).astype(dtype)  # (one row more than max(T, k): the pe_shift mutant's)

    def embed(side, vals, frames):
        x = vals[:, None] * g(side + "input_fc.weight")[:, 0][None] + g(side + "input_fc.bias")[None]
        cat = np.concatenate([x, pe[frames]], axis=1)
        return cat @ g(side + "pos_encoder.fc.weight").T + g(side + "pos_encoder.fc.bias")

    x = embed(E, u.reshape(-1), np.repeat(np.arange(T), n))
    for i in range(n_enc):
        x = _layer(g, f"{E}tf_encoder.layers.{layer_index(i, n_enc)}.", x, None, n, nhead, False, mut, stats)
    mem = x
    dec_in = u[-2] if "dec_in_prev" in mut else u[-1]
    shift = 1 if "pe_shift" in mut else 0

    def decode(frames):
        y = embed(F, np.tile(dec_in, frames), np.repeat(np.arange(frames), n) + shift)
        for i in range(n_dec):
            y = _layer(g, f"{F}tf_decoder.layers.{layer_index(i, n_dec)}.", y, mem, n, nhead, True, mut, stats)
        return (y @ g(F + "out_fc.weight").T + g(F + "out_fc.bias")).reshape(frames, n, -1)

    if not loop:
        out = decode(k)
        assert out.dtype == dtype
        return out
    # the reference's form: pass f runs the decoder over f frames, the same input re-appended; frame f - 1 is the block that
    # pass newly produced.  The reference keeps its last pass whole; under the block-causal mask every earlier pass already
    # gave its newest block the same value, which is what this returns (frame f - 1 from pass f) for the tests to compare.
    return np.stack([decode(frames)[frames - 1] for frames in range(1, k + 1)])


def c_pred_refine(seq_out):
    """``_seq_out`` (k, N, S) -> ``_dec_motion`` (N, k, S) -> the post-hook's permute back: (k, N, S)"""
    return np.ascontiguousarray(np.transpose(np.transpose(seq_out, (1, 0, 2)), (1, 0, 2)))


def scene_input(C_obs, nrm, lo, hi):
    """u (k+2, n) of the rows [lo, hi) of a split: [C_obs; last observed position - its mean over the scene]"""
    ori = np.asarray(nrm[:2, lo:hi], np.float32)
    ori = ori - ori.mean(axis=1, keepdims=True, dtype=np.float32)
    return np.concatenate([np.asarray(C_obs[:, lo:hi], np.float32), ori]).astype(np.float32)
