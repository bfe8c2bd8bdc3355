#!/usr/bin/env python3
"""G27: ET-Graph-TERN inference fixture -- the reference's wrapper + its graphtern bridge + its graph_tern_light with the
ET constructor arguments (utils/trainer.py:540: n_epgcn=1, n_epcnn=6, input_feat=1, seq_len=k+2, pred_seq_len=k,
n_smpl=S), seeded, run on CPU in the build container.

    python tools/make_golden_graphtern.py --ref /root/reference --out tests/golden
    python tools/make_golden_graphtern.py --family [--ref ... --out ...]    # G33 only, see family(); G27 is left alone

The reference's normalizer moves its identity matrices to the GPU (`torch.eye(...).cuda()`, baseline/graphtern/
normalizer.py); there is no GPU here, so for the duration of this script `Tensor.cuda` / `Module.cuda` are the identity --
the arithmetic is the reference's own.  Before anything is recorded EVERY PReLU slope is set to its own random value, the
one the network never applies (tp_mrgcns.{i}.prelu) included.  The ET descriptors and anchors are G2's
(tests/golden/g2_fit_all_scenes.npz), per split; they are not copied here.

ET-Graph-TERN's graphs hold 1 / |u_i - u_j| (0 where the distance is exactly 0), so the reference's ADE / FDE are NOT
stable under a 1-ulp change of a coefficient: what is recorded per pedestrian is the NETWORK's output on the network's own
fp32 input, and per split only the means with the reference's own measured spread.  Stored:
  net.<state_dict key>          the predictor's state_dict (one set for all splits: they share k = 6, S = 20)
  eth.scene_size, eth.s_obs, eth.net_out, eth.c_obs
                                EVERY eth test scene, concatenated along the pedestrian axis in scene order: the bridge's
                                S_obs as (2, T, N) = [abs, rel], the raw network output (k, N, S), and the reference's own
                                coefficients (k, N) (a printed diagnostic of the GPU test only)
  <split>.scene_size, .ade_mean, .fde_mean, .ade_spread, .fde_spread, .moved_share
                                float64 means of the per-pedestrian best-of-S ADE / FDE over the split's test scenes; the
                                largest |mean under perturbation - mean| over 8 seeded draws; the share of scenes whose
                                network output moved by more than 1e-5 of its largest entry in the first draw.  Draws 0-3,
                                kind (a): every non-zero C_obs entry moved by d 2^-23 max|C_obs| of its scene, d drawn from
                                (-1, 0, +1), and each obs_ori row shifted as a whole by d 2^-22 max|obs_ori|; draws 4-7,
                                kind (b): the same plus d 2^-23 max|C_obs| on the all-zero columns (static pedestrians)
  pick<i>.{split,index,s_obs,net_out}
                                the largest test scene of each split, and the first scene with 2 <= n <= 30 that has an
                                off-diagonal exact zero of A_abs between two non-zero values
  grid.*, single.*, pair.*, edge.*
                                hand-built scenes through the reference's bridge and network: n = 12 with every entry a
                                multiple of 0.25 and columns 2 and 5 identical; n = 1, 2, 3
  gen.<state_dict key>, gen.net_out<i>
                                a second weight set, n_epgcn = 2, n_epcnn = 3, n_smpl = 12, on the inputs of picks 0 and 1
  keys.s16                      the reference's state_dict key names for n_smpl = 16 (no rescconv)
The script asserts what the tests rely on: the fp64 restatement (tests/_graphtern_np.py) reproduces EVERY recorded output
within 1e-5 of its largest entry, the reference's A equals |x_i - x_j| in fp32 bit for bit on every recorded scene, and the
reference's fp32 run is within 1e-5 of its own fp64 run on the same input.
Only data is written; nothing of the reference is copied."""
import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

ET_ARGS = dict(n_epgcn=1, n_epcnn=6, input_feat=1, seq_len=8, pred_seq_len=6, n_smpl=20)
GEN_ARGS = dict(n_epgcn=2, n_epcnn=3, input_feat=1, seq_len=8, pred_seq_len=6, n_smpl=12)
DRAWS = 8


def randomise(net, gen):
    """every PReLU slope its own non-default value"""
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.PReLU):
                m.weight.copy_(0.05 + 0.4 * torch.rand(m.weight.shape, generator=gen))


def perturb(C_obs, obs_ori, rng, static_too):
    """one draw: (C_obs (k, n), obs_ori (2, n)) fp32 -> the same a unit in the last place of the scene's scale away"""
    C = C_obs.clone()
    step = float(C.abs().max()) * 2.0 ** -23
    d = torch.from_numpy(rng.integers(-1, 2, size=tuple(C.shape)).astype(np.float32))
    move = C != 0
    if static_too:
        move = move | (C == 0).all(dim=0, keepdim=True)
    C = torch.where(move, C + d * step, C)
    o = obs_ori.clone()
    shift = torch.from_numpy(rng.integers(-1, 2, size=(2, 1)).astype(np.float32))
    o = o + shift * (float(o.abs().max()) * 2.0 ** -22)
    return C, o


def tied_zero(u):
    """u (T, n) -> an off-diagonal exact zero of A_abs between two NON-zero values in some time row"""
    for row in u:
        nz = row[row != 0]
        if len(np.unique(nz)) < len(nz):
            return True
    return False


def family(args):
    """G33 (--family): the reference's graph_tern_light at every member of tests/_graphtern_np.py: CONFIGS, under that
    configuration's seeded weights (GN.random_state, loaded with strict=True), on the bridge's S_obs of the two scenes of
    GN.fixture_inputs (3 and 13 pedestrians from the edge generator).  Stored per configuration and scene size n:
      <name>.s_obs<n>     the bridge's S_obs as (2, T, n) = [abs, rel]
      <name>.net_out<n>   the raw network output (k, n, S)
    The weights are not stored: the tests regenerate them from the seed.  Asserted before anything is written: S_obs is
    GN.s_obs_of(u) bit for bit, the fp64 restatement reproduces every output within 1e-5 of its largest entry, and the
    reference's fp32 run is within 1e-5 of its own fp64 run.  A configuration the reference refuses to build or run is left
    out and named in the manifest (MANIFEST_g33_graphtern_family.json).  Only data is written."""
    import json
    from tests import _graphtern_np as GN
    sys.path.insert(0, args.ref)
    os.chdir(args.ref)
    torch.Tensor.cuda = lambda self, *a, **k: self  # no GPU in the build container (see the module docstring)
    torch.nn.Module.cuda = lambda self, *a, **k: self
    from baseline.graphtern import TrajectoryPredictor, model_forward, model_forward_pre_hook
    torch.set_num_threads(1)
    out, per_case, refused = {}, {}, {}
    for name in GN.CONFIGS:
        sd = GN.random_state(name)
        try:
            nets = []
            for _ in range(2):  # (the residuals are lambdas closing over the instance: the fp64 copy is built afresh)
                net = TrajectoryPredictor(**GN.module_cfg(name))
                net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
                nets.append(net.eval())
            nets[1].double()
            sizes, C_obs, nrm = GN.fixture_inputs(name)
            case = {}
            for _, lo, n, u in GN.scenes_of(sizes, C_obs, nrm):
                k = C_obs.shape[0]
                with torch.no_grad():
                    inp = model_forward_pre_hook(torch.from_numpy(u[:k]), torch.from_numpy(u[k:]))
                    res = model_forward(inp, nets[0])
                    r64 = nets[1](inp[0].double())
                case[n] = (inp[0].numpy(), res[0].numpy(), r64[0].numpy(), u)
        except Exception as exc:  # noqa: BLE001 -- the reference's own refusal of a shape
            refused[name] = f"{type(exc).__name__}: {exc}"
            print(f"{name}: the reference refuses this shape ({refused[name]}); left out", flush=True)
            continue
        c = GN.CONFIGS[name]
        for n, (s_obs, ref, r64, u) in case.items():
            assert s_obs.shape == (1, 2, c["k"] + 2, n, 1) and ref.shape == (c["k"], n, c["S"]) and ref.dtype == np.float32
            assert np.array_equal(s_obs, GN.s_obs_of(u)), (name, n)
            scale = np.abs(ref).max()
            e_np = float(np.abs(GN.forward(sd, s_obs[0, 0, :, :, 0], s_obs[0, 1, :, :, 0]) - ref).max() / scale)
            e_64 = float(np.abs(r64 - ref).max() / scale)
            assert e_np <= 1e-5 and e_64 <= 1e-5, (name, n, e_np, e_64)
            out[f"{name}.s_obs{n}"], out[f"{name}.net_out{n}"] = s_obs[0, :, :, :, 0], ref
            per_case[f"{name}.{n}"] = {"restatement_vs_reference": e_np, "reference_fp32_vs_fp64": e_64,
                                       "largest_entry": float(scale)}
            print(f"{name} n = {n}: restatement {e_np:.2e}, the reference's fp32 against its fp64 run {e_64:.2e}", flush=True)
    path = os.path.join(args.out, "g33_graphtern_family.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1024 * 1024
    manifest = {"g33_graphtern_family": {
        "cases": sorted(per_case), "refused_by_the_reference": refused, "state_seed": GN.STATE_SEED,
        "configs": {n: {k: v for k, v in c.items()} for n, c in GN.CONFIGS.items()}, "scene_sizes": list(GN.FIXTURE_SIZES),
        "numpy": np.__version__, "torch": torch.__version__, "bytes": size, "per_case": per_case}}
    with open(os.path.join(args.out, "MANIFEST_g33_graphtern_family.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")
    print("wrote", path, size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    ap.add_argument("--family", action="store_true",
                    help="write g33_graphtern_family.npz (the members of tests/_graphtern_np.py: CONFIGS) and leave g27 alone")
    args = ap.parse_args()
    if args.family:
        return family(args)
    from tests import _golden as G
    from tests import _graphtern_np as GN
    sys.path.insert(0, args.ref)
    os.chdir(args.ref)

    # no GPU in the build container: keep the reference's normalizer on the CPU
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self

    from baseline.graphtern import TrajectoryPredictor, model_forward, model_forward_post_hook, model_forward_pre_hook
    from baseline.graphtern.model import generate_adjacency_matrix
    from EigenTrajectory import EigenTrajectory
    from utils.metrics import compute_batch_ade, compute_batch_fde
    from utils.utils import DotDict, get_exp_config

    torch.set_num_threads(1)
    g2 = G.load("g2_fit_all_scenes.npz")
    out = {}
    recorded = []  # (tag, s_obs (1,2,T,n,1) tensor, net_out (k,n,S) numpy, which weights)
    picks = []
    t0 = time.time()
    net_state = None
    first_tied = None

    def fresh(kw, state=None, seed=1234, slopes=4321):
        torch.manual_seed(seed)
        net = TrajectoryPredictor(**kw)
        randomise(net, torch.Generator().manual_seed(slopes))
        if state is not None:
            net.load_state_dict(state)
        return net.eval()

    for scene in G.SCENES:
        hp = get_exp_config(f"./config/eigentrajectory-{{baseline}}-{scene}.json")
        assert hp.k == 6 and hp.num_samples == 20, (hp.k, hp.num_samples)
        predictor = fresh(ET_ARGS)
        if net_state is None:
            net_state = {k: v.detach().clone() for k, v in predictor.state_dict().items()}
        captured = {}
        draw = {"rng": None, "static": False}

        def pre_and_perturb(obs_data, obs_ori, addl_info=None):
            if draw["rng"] is not None:
                obs_data, obs_ori = perturb(obs_data, obs_ori, draw["rng"], draw["static"])
            captured["c_obs"] = obs_data.detach().clone()
            return model_forward_pre_hook(obs_data, obs_ori, addl_info)

        def forward_and_capture(input_data, baseline_model):
            captured["s_obs"] = input_data[0].detach().clone()
            res = model_forward(input_data, baseline_model)
            captured["net_out"] = res.detach().clone()
            return res

        hook = DotDict(model_forward_pre_hook=pre_and_perturb, model_forward=forward_and_capture,
                       model_forward_post_hook=model_forward_post_hook)
        model = EigenTrajectory(predictor, hook, hp).eval()
        sd = model.state_dict()
        for key in list(sd):
            if key.startswith("ET_"):
                sd[key] = torch.from_numpy(g2[f"{scene}.{key}"])
        model.load_state_dict(sd)
        obs, pred, sse = G.dataset(scene, "test")

        def run_split(keep):
            ades, fdes, outs, records = [], [], [], []
            for i, (s, e) in enumerate(sse):
                o, p = torch.from_numpy(obs[s:e]), torch.from_numpy(pred[s:e])
                with torch.no_grad():
                    res = model(o)  # the test loop's call (utils/trainer.py:183)
                ades.append(np.asarray(compute_batch_ade(res["recon_traj"], p), np.float64))
                fdes.append(np.asarray(compute_batch_fde(res["recon_traj"], p), np.float64))
                outs.append(captured["net_out"][0].numpy())
                if keep:
                    records.append((e - s, i, {k: captured[k].clone() for k in captured}))
            return float(np.concatenate(ades).mean()), float(np.concatenate(fdes).mean()), outs, records

        ade, fde, base_outs, records = run_split(True)
        spread_a = spread_f = 0.0
        moved = 0.0
        for j in range(DRAWS):
            draw["rng"], draw["static"] = np.random.default_rng(1000 + j), j >= DRAWS // 2
            a_j, f_j, outs_j, _ = run_split(False)
            spread_a, spread_f = max(spread_a, abs(a_j - ade)), max(spread_f, abs(f_j - fde))
            if j == 0:
                moved = float(np.mean([np.abs(x - y).max() > 1e-5 * np.abs(y).max() for x, y in zip(outs_j, base_outs)]))
        draw["rng"] = None
        sizes = [r[0] for r in records]
        out[f"{scene}.scene_size"] = np.asarray(sizes, np.int64)
        out[f"{scene}.ade_mean"], out[f"{scene}.fde_mean"] = np.float64(ade), np.float64(fde)
        out[f"{scene}.ade_spread"], out[f"{scene}.fde_spread"] = np.float64(spread_a), np.float64(spread_f)
        out[f"{scene}.moved_share"] = np.float64(moved)
        if scene == "eth":
            out["eth.s_obs"] = np.concatenate([r[2]["s_obs"][0, :, :, :, 0].numpy() for r in records], axis=2)
            out["eth.net_out"] = np.concatenate([r[2]["net_out"][0].numpy() for r in records], axis=1)
            out["eth.c_obs"] = np.concatenate([r[2]["c_obs"].numpy() for r in records], axis=1)
            for size, idx, cap in records:
                recorded.append((f"eth[{idx}]", cap["s_obs"], cap["net_out"][0].numpy(), "net"))
        largest = max(records, key=lambda r: r[0])
        chosen = [largest]
        if first_tied is None:
            tied = [r for r in records if 2 <= r[0] <= 30 and r[1] != largest[1]
                    and tied_zero(r[2]["s_obs"][0, 0, :, :, 0].numpy())]
            if tied:
                first_tied = tied[0]
                chosen.append(tied[0])
        for size, idx, cap in chosen:
            tag = f"pick{len(picks)}"
            picks.append(tag)
            out[f"{tag}.split"] = np.asarray(scene)
            out[f"{tag}.index"] = np.int64(idx)
            out[f"{tag}.s_obs"] = cap["s_obs"].numpy().astype(np.float32)
            out[f"{tag}.net_out"] = cap["net_out"].numpy().astype(np.float32)
            recorded.append((tag, cap["s_obs"], cap["net_out"][0].numpy(), "net"))
        print(f"{scene}: {len(sse)} scenes, {sum(sizes)} pedestrians, largest {largest[0]}, ADE {ade:.6f} +- {spread_a:.1e} "
              f"FDE {fde:.6f} +- {spread_f:.1e}, scenes moved by more than 1e-5: {moved:.3f}  ({time.time() - t0:.0f} s)",
              flush=True)
    assert first_tied is not None
    for key, val in net_state.items():
        out[f"net.{key}"] = val.numpy()

    # hand-built scenes through the reference's bridge and network
    predictor = fresh(ET_ARGS, net_state)
    rng = np.random.default_rng(27)
    grid = (rng.integers(-12, 13, size=(8, 12)) * 0.25).astype(np.float32)
    grid[:, 5] = grid[:, 2]  # identical columns
    hand = {"grid": grid, "single": np.asarray([[0.5], [-1.25], [2.0], [0.0], [3.0], [-0.75], [1.5], [-2.0]], np.float32),
            "pair": (rng.integers(-12, 13, size=(8, 2)) * 0.25).astype(np.float32),
            "edge": rng.normal(0, 1, size=(8, 3)).astype(np.float32)}
    for tag, v in hand.items():
        with torch.no_grad():
            inp = model_forward_pre_hook(torch.from_numpy(v[:6]), torch.from_numpy(v[6:]))
            res = model_forward(inp, predictor)
        out[f"{tag}.s_obs"], out[f"{tag}.net_out"] = inp[0].numpy(), res.numpy()
        recorded.append((tag, inp[0], res[0].numpy(), "net"))
    g_abs = GN.distances(out["grid.s_obs"][0, 0, :, :, 0])
    assert int(((g_abs == 0) & ~np.eye(12, dtype=bool)).sum()) > 2 * 8  # zeros beyond the identical pair of columns

    # the generic loop structure: two st_mrgcn blocks (the second with C_in = 16 and an identity residual), three epcnn blocks
    gen_net = fresh(GEN_ARGS, seed=99, slopes=77)
    for key, val in gen_net.state_dict().items():
        out[f"gen.{key}"] = val.detach().numpy()
    for i, tag in enumerate(picks[:2]):
        s_obs = torch.from_numpy(out[f"{tag}.s_obs"])
        with torch.no_grad():
            res = gen_net(s_obs)
        out[f"gen.net_out{i}"] = res.numpy()
        recorded.append((f"gen {tag}", s_obs, res[0].numpy(), "gen"))
    out["keys.s16"] = np.asarray(sorted(TrajectoryPredictor(**dict(ET_ARGS, n_smpl=16)).state_dict()))
    assert not any("rescconv" in k for k in out["keys.s16"])

    # what the tests rely on
    sd_np = {k[4:]: v for k, v in out.items() if k.startswith("net.")}
    gen_np = {k[4:]: v for k, v in out.items() if k.startswith("gen.") and not k.startswith("gen.net_out")}
    # (the reference's residuals are lambdas closing over the instance: a deepcopy keeps the fp32 convs; build afresh)
    dbl = {"net": fresh(ET_ARGS, net_state).double(), "gen": fresh(GEN_ARGS, gen_net.state_dict()).double()}
    worst = worst64 = 0.0
    for tag, s_obs, ref, which in recorded:
        u, rel = s_obs[0, 0, :, :, 0].numpy(), s_obs[0, 1, :, :, 0].numpy()
        A = generate_adjacency_matrix(s_obs)[0].numpy()
        assert np.array_equal(A[0], GN.distances(u)) and np.array_equal(A[1], GN.distances(rel)), tag
        assert np.array_equal(rel, GN.rel_of(u)), tag
        got = GN.forward(sd_np if which == "net" else gen_np, u, rel)
        scale = np.abs(ref).max()
        worst = max(worst, float(np.abs(got - ref).max() / scale))
        with torch.no_grad():
            r64 = dbl[which](s_obs.double())[0].numpy()
        worst64 = max(worst64, float(np.abs(r64 - ref).max() / scale))
    print(f"{len(recorded)} recorded scenes; fp64 restatement against the recorded outputs: {worst:.2e} of the largest "
          f"entry; the reference's fp32 run against its fp64 run: {worst64:.2e}")
    assert worst <= 1e-5 and worst64 <= 1e-5, (worst, worst64)
    path = os.path.join(args.out, "g27_graphtern.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "picks",
          [(str(out[f'{t}.split']), int(out[f'{t}.index']), out[f'{t}.s_obs'].shape[3]) for t in picks])
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()
