"""CPU-side checks: the C-ABI library loads and exports everything include/eigentraj.h declares,
the host mirror of the reference interface has the reference's names/shapes, and the product
path fails loudly without a HIP device (no CPU fallback).  No kernels are launched here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from . import _abi_header as H
from . import _golden as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="asserts the behaviour on a box without a GPU")


def header_functions():
    return sorted(set(re.findall(r"\b(et_[a-z0-9_]+)\s*\(", H.text())))


def test_library_exports_every_declared_symbol():
    from eigentrajectory_amd import _lib
    lib = _lib.lib()
    declared = header_functions()
    assert len(declared) >= 25
    for name in declared:
        assert hasattr(lib, name), f"libetamd.so does not export {name}"
    assert sorted(_lib.SYMBOLS) == declared
    assert lib.et_abi_version() == _lib.ABI_VERSION == 3
    assert lib.et_compiled_arch() == b"gfx950"
    assert lib.et_status_string(0) == b"ok" and b"workspace" in lib.et_status_string(4)


def test_options_table_and_no_environment_reads():
    """include/eigentraj.h "tuning switches": et_set_option / et_get_option are the library's only mutable configuration
    -- unknown keys and values are rejected, values round-trip -- and no kernel source reads the environment (the test
    hook of one GPU test lives in libetamd_testhooks.so, not in the product library)."""
    from eigentrajectory_amd import _lib
    assert _lib.get_option("kmeans_loop") == "a" and _lib.get_option("kmeans_packed") == "1"
    with _lib.option("kmeans_loop", "chain"):
        assert _lib.get_option("kmeans_loop") == "c"
    assert _lib.get_option("kmeans_loop") == "a"
    with _lib.option("kmeans_packed_min", 262144):
        assert _lib.get_option("kmeans_packed_min") == "262144"
    for key, value in (("no_such_key", "1"), ("kmeans_loop", "x"), ("kmeans_packed", "yes"), ("kmeans_packed", "")):
        with pytest.raises(ValueError):
            _lib.set_option(key, value)
    csrc = os.path.join(ROOT, "eigentrajectory_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h")):
            assert "getenv" not in open(os.path.join(csrc, name)).read(), name
    import subprocess
    syms = subprocess.run(["nm", "-D", _lib.LIB_PATH], capture_output=True, text=True).stdout
    # (test hooks are in libetamd_testhooks.so only; the stamp readers come with the patches of tools/archive/instrumentation/)
    assert "et_testhook" not in syms and "et_debug" not in syms


def test_csrc_has_one_conditional_and_the_makefile_one_define():
    """The product source is what a default build compiles: the only conditional compilation under csrc/ is ET_TEST_HOOKS
    (measurement switches and stamps live in tools/archive/, as patches), and the Makefile defines nothing else."""
    import re
    import subprocess
    csrc = os.path.join(ROOT, "eigentrajectory_amd", "csrc")
    directive = re.compile(r"^\s*#\s*(if|ifdef|ifndef|elif)\b(.*)$")  # (#pragma once is no conditional; #else / #endif follow one)
    seen = []
    for name in sorted(os.listdir(csrc)):
        path = os.path.join(csrc, name)
        if not os.path.isfile(path) or name.endswith((".o", ".so")):
            continue
        for no, line in enumerate(open(path, errors="replace"), 1):
            m = directive.match(line)
            if m:
                seen.append(name)
                assert re.search(r"\bET_TEST_HOOKS\b", m.group(2)), f"{name}:{no}: {line.strip()}"
    assert seen, "the ET_TEST_HOOKS sites were not found: the scan reads the wrong files"
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert set(re.findall(r"(?<![\w-])-D\s*\w+", makefile)) == {"-DET_TEST_HOOKS"}
    # ... and none reaches a compile line through a variable: the commands of a full build, not run
    dry = subprocess.run(["make", "-n", "-B", "-C", csrc, "all"], capture_output=True, text=True, check=True).stdout
    n_srcs = len(subprocess.run(["make", "-s", "-C", csrc, "print-srcs"], capture_output=True, text=True, check=True).stdout.split())
    assert n_srcs >= 15 and dry.count(" -c ") == n_srcs + 1  # every source, and et_kmeans.hip once more for the hooks
    assert set(re.findall(r"(?<![\w-])-D\s*\w+", dry)) == {"-DET_TEST_HOOKS"}


def test_state_struct_layout_matches_header():
    from eigentrajectory_amd import _lib
    assert _lib.STATE_BYTES == 96
    offs = {n: getattr(_lib.KMeansState, n).offset for n, _ in _lib.KMeansState._fields_}
    assert offs == dict(max_abs_x=0, max_abs_c=8, n_total=16, frac=24, sim_frac=32, iter=40, done=48, bad_input=56,
                        error=64, inertia=72, fast_ok=80, min_nz_x_bits=88)
    lib = _lib.lib()
    assert lib.et_kmeans_partials_len(6, 20) == 6 * 20 + 20 + 2
    assert lib.et_kmeans_workspace_bytes(ctypes.c_int64(1000), 6, 20) > 1000 * 5
    assert lib.et_kmeans_workspace_bytes(ctypes.c_int64(1000), 33, 20) == 0  # d out of range
    assert lib.et_fit_gram_workspace_bytes(ctypes.c_int64(10 ** 7), 8, 12) >= 512 * (256 + 576 + 1) * 8


def test_argument_validation_without_device_work():
    """Invalid arguments are rejected on the host side before any launch."""
    from eigentrajectory_amd import _lib
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    z = ctypes.c_int64(0)
    assert lib.et_norm_project(null, null, ctypes.c_int64(-1), 8, 12, 6, null, null, null, null, 2,
                               ctypes.c_float(0), null, null, null, null, null) == 1
    assert lib.et_norm_project(null, null, z, 8, 12, 6, null, null, null, null, 2, ctypes.c_float(0), null, null, null,
                               null, null) == 0  # N == 0 is a valid no-op
    assert lib.et_norm_project(null, null, z, 2, 12, 6, null, null, null, null, 2, ctypes.c_float(0), null, null, null,
                               null, null) == 1  # T_obs < 3: obs[-3] does not exist
    assert lib.et_anchor_reconstruct_fwd(null, z, 0, 6, 8, 12, null, null, null, null, null, null, 2,
                                         ctypes.c_float(0), null, null) == 1
    assert lib.et_eigh_topk(null, 16, 6, null, null, null) == 1
    assert lib.et_eigh_topk_batch(1, null, null, null, null, null, null) == 1
    assert lib.et_eigh_topk_batch(9, null, null, null, null, null, null) == 1  # more than ET_EIGH_MAX_BATCH
    assert lib.et_eigh_topk_batch(0, null, null, null, null, null, null) == 0  # empty batch: no-op
    assert lib.et_kmeans_predict(null, z, 6, null, 20, null, null, null) == 1


def _fill_pointers(obj, value):
    """Every pointer field of a ctypes struct (nested structs and arrays included) := value."""
    if isinstance(obj, ctypes.Array):
        for i in range(len(obj)):
            if obj._type_ is ctypes.c_void_p:
                obj[i] = value
            elif not issubclass(obj._type_, ctypes._SimpleCData):
                _fill_pointers(obj[i], value)
        return
    for name, typ in obj._fields_:
        if typ is ctypes.c_void_p:
            setattr(obj, name, value)
        elif not issubclass(typ, ctypes._SimpleCData):
            _fill_pointers(getattr(obj, name), value)


def _scene_entry_params(ph):
    """{predictor: (params struct of a small supported configuration (k = 6, S = 20, one layer of each kind), the field
    whose value -- second item -- takes it outside the native family)}.  ``ph`` stands for every weight pointer: the host
    checks them against NULL and never reads through them."""
    from eigentrajectory_amd import _lib as L

    def stgcnn(n_txpcnn=1):
        p = L.STGCNNParams(n_stgcnn=1, n_txpcnn=n_txpcnn, input_feat=1, output_feat=20, seq_len=8, pred_seq_len=6,
                           kernel_size=3, bn_eps=1e-5)
        _fill_pointers(p, ph)
        return p

    def sgcn():
        p = L.SGCNParams(n_asym=1, embedding_dims=64, n_gcn_layers=1, obs_len=8, pred_len=6, n_tcn=1, in_dims=1, out_dims=20,
                         num_heads=4, dropout=0.0)
        _fill_pointers(p, ph)
        return p

    gp_sgcn, gp_stgcnn = L.GPGraphSGCNParams(), L.GPGraphSTGCNNParams()
    _fill_pointers(gp_sgcn, ph)
    _fill_pointers(gp_stgcnn, ph)
    gp_sgcn.base, gp_sgcn.tau, gp_stgcnn.base, gp_stgcnn.tau = sgcn(), 0.1, stgcnn(), 0.1

    dm = L.DMRGCNParams(n_stgcn=1, n_tpcnn=1, input_feat=1, output_feat=20, seq_len=8, pred_seq_len=6, kernel_size=3)
    _fill_pointers(dm, ph)
    for r, split in enumerate(([0, 1 / 4, 2 / 4, 3 / 4, 1], [0, 1 / 2, 1, 2, 4])):
        for b, v in enumerate(split):
            dm.split[r][b] = v

    im = L.ImplicitParams(spatial_input=1, spatial_output=20, temporal_input=8, temporal_output=6, n_bins=1)
    _fill_pointers(im, ph)

    af = L.AgentFormerParams(motion_dim=1, model_dim=16, ff_dim=16, nhead=1, forecast_dim=20, past_frames=8, future_frames=6,
                             n_enc=1, n_dec=1)
    _fill_pointers(af, ph)

    gt = L.GraphTERNParams(n_epgcn=1, n_epcnn=2, input_feat=1, hidden_feat=16, seq_len=8, pred_seq_len=6, n_smpl=20)
    _fill_pointers(gt, ph)
    # the residual convolutions exist only where the widths differ: T != k in the first epcnn block, 16 != S in the last
    gt.tpcnns[0].resc_w = gt.tpcnns[0].resc_b = gt.tpcnns[1].rest_w = gt.tpcnns[1].rest_b = None

    def mlp(pecnet):
        p = L.MLPParams(fdim=4, nonlocal_pools=0, non_local_dim=0, out_width=12, pos_width=2 if pecnet else 0)
        _fill_pointers(p, ph)
        for chain, widths in ((p.encoder_past, (6, 8, 4)), (p.encoder_dest, (2, 8, 4)),
                              (p.predictor, (2 * 4 + p.pos_width, 8, 12))):
            chain.n_layers = 2
            for i, w in enumerate(widths):
                chain.widths[i] = w
        return p

    return {"stgcnn": (stgcnn(), "kernel_size", 5), "sgcn": (sgcn(), "num_heads", 2),
            "gpgraph_sgcn": (gp_sgcn, "base.num_heads", 2), "gpgraph_stgcnn": (gp_stgcnn, "base.kernel_size", 5),
            "dmrgcn": (dm, "kernel_size", 5), "implicit": (im, "spatial_input", 2), "agentformer": (af, "motion_dim", 2),
            "graphtern": (gt, "hidden_feat", 8), "pecnet": (mlp(True), "fdim", 0), "lbebm": (mlp(False), "fdim", 0),
            "stgcnn_3tpcnn": (stgcnn(3), None, None)}


@needs_no_gpu
def test_scene_entry_points_answer_before_any_launch():
    """The status every et_*_forward_scenes entry point answers to arguments it refuses, or finishes, on the host: no row
    gets as far as a launch, and none makes the host read scene_offsets (a placeholder address, like every other
    pointer here).  Then the workspace sizes of the three predictors that keep a per-scene arena."""
    from eigentrajectory_amd import _lib as L
    lib = L.lib()
    backing = (ctypes.c_char * 64)()
    ph = ctypes.addressof(backing)
    params = _scene_entry_params(ph)
    # predictor: (arguments between n_scenes and C_pred_refine, optional outputs after it, largest unlisted batch)
    table = {"stgcnn": ((), 0, L.SCENE_MAX_N), "sgcn": ((0, 0), 2, L.SGCN_MAX_N), "gpgraph_sgcn": ((0, 0), 4, L.SGCN_MAX_N),
             "gpgraph_stgcnn": ((0, 0), 3, L.SGCN_MAX_N), "dmrgcn": ((), 1, L.SCENE_MAX_N), "implicit": ((), 2, L.SCENE_MAX_N),
             "agentformer": ((), 1, L.AGENTFORMER_MAX_SCENE_N), "graphtern": ((), 1, L.SCENE_MAX_N),
             "pecnet": ((), 1, L.SCENE_MAX_N), "lbebm": ((), 1, L.SCENE_MAX_N)}
    assert len(table) == 10
    for name, (mid, n_optional, one_scene_cap) in table.items():
        fn = getattr(lib, f"et_{name}_forward_scenes")
        good, bad_field, bad_value = params[name]

        def status(p, N, off, n_scenes, data=ph, ws=ph, ws_bytes=1 << 20):
            return fn(p, data, data, N, off, n_scenes, *mid, data, *([None] * n_optional), ws, ws_bytes, None)

        ref = ctypes.byref(good)
        assert status(None, 3, None, 0) == 1, name                      # no parameters
        assert status(ref, -1, None, 0) == 1, name                      # N < 0
        assert status(ref, 3, ph, -1) == 1, name                        # n_scenes < 0
        assert status(ref, 5, ph, 0) == 1, name                         # offsets without scenes, for 5 rows
        assert status(ref, 0, ph, 0) == 0, name                         # offsets without scenes, for no rows: nothing to do
        assert status(ref, one_scene_cap + 1, None, 0) == 1, name       # one unlisted scene above the limit
        assert status(ref, 0, None, 0) == 0, name                       # N == 0: nothing to do
        assert status(ref, 3, None, 0, data=None) == 1, name            # no C_obs / nrm / C_pred_refine
        if name in ("implicit", "agentformer"):
            assert status(ref, 3, None, 0, ws=None, ws_bytes=0) == 4, name  # these two need a workspace for any N > 0
        owner, _, field = bad_field.rpartition(".")
        owner = getattr(good, owner) if owner else good
        keep = getattr(owner, field)
        setattr(owner, field, bad_value)
        assert status(ref, 3, None, 0) == 3, name                       # outside the native family
        setattr(owner, field, keep)
        assert status(ref, 0, None, 0) == 0, name                       # (the struct is whole again)

    # arena predictors: floats per pedestrian from the header comment of each source file, K = T = k + 2 = 8, S = 20
    K, k, S = 8, 6, 20
    arenas = {"stgcnn": (params["stgcnn_3tpcnn"][0], 2 * K + 2 * S * K + k * S),   # 2K + 2SK + Q, Q = k S with 3 tpcnn layers
              "dmrgcn": (params["dmrgcn"][0], 2 * K + 10 * K + 3 * S * K),          # 2K + 10K + 3Q, Q = S K
              "graphtern": (params["graphtern"][0], 6 * K + 3 * 16 * K)}            # 6T + 3Q, Q = 16 T
    assert [4 * per for _, per in arenas.values()] == [1824, 2304, 1728]           # the bytes those comments state
    for name, (p, per) in arenas.items():
        fn = getattr(lib, f"et_{name}_workspace_bytes")
        ref = ctypes.byref(p)
        fits = (60 * 1024) // (per * 4)  # the largest scene whose arena fits the 60 KiB of LDS
        assert fn(None, 100, 10) == 0 and fn(ref, -1, 10) == 0 and fn(ref, 100, -1) == 0, name
        assert fn(ref, 100, 0) == 0 and fn(ref, 100, fits) == 0 and fn(ref, 10 ** 6, fits) == 0, name
        assert fn(ref, 100, fits + 1) == per * 100 * 4 and fn(ref, 10 ** 6, fits + 1) == per * 10 ** 6 * 4, name
        setattr(p, *params[name][1:])
        assert fn(ref, 100, fits + 1) == 0, name                                   # outside the native family


@needs_no_gpu
def test_product_path_fails_loudly_without_gpu():
    from eigentrajectory_amd import TrajNorm, ops
    from eigentrajectory_amd._lib import ETLibraryError
    with pytest.raises(ETLibraryError):
        TrajNorm().calculate_params(torch.zeros(4, 8, 2))
    with pytest.raises(ETLibraryError):
        ops.kmeans_predict(torch.zeros(6, 10), torch.zeros(6, 20))


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "eigentrajectory_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in text and "from oracle" not in text and "et_oracle" not in text.replace(
                    "oracle/et_oracle.c", ""), f


def test_wrapper_has_the_reference_interface():
    """Sub-module names, state_dict keys and shapes of EigenTrajectory/model.py:16-32."""
    from eigentrajectory_amd import BatchKMeans, EigenTrajectory, ETAnchor, ETDescriptor, TrajNorm
    from eigentrajectory_amd.utils import DotDict, default_hyper_params
    hp = default_hyper_params()
    assert isinstance(hp, DotDict) and hp.k == 6 and hp.missing is None
    base = torch.nn.Linear(3, 3)
    hooks = DotDict(model_forward_pre_hook=None, model_forward=None, model_forward_post_hook=None)
    m = EigenTrajectory(base, hooks, hp)
    sd = m.state_dict()
    expect = {"ET_m_descriptor.U_obs_trunc": (16, 6), "ET_m_descriptor.U_pred_trunc": (24, 6),
              "ET_s_descriptor.U_obs_trunc": (16, 6), "ET_s_descriptor.U_pred_trunc": (24, 6),
              "ET_m_anchor.C_anchor": (6, 20), "ET_s_anchor.C_anchor": (6, 20),
              "baseline_model.weight": (3, 3), "baseline_model.bias": (3,)}
    assert {k: tuple(v.shape) for k, v in sd.items()} == expect
    g2 = G.load("g2_fit_all_scenes.npz")
    ref_sd = {k[4:]: torch.from_numpy(g2[k]) for k in g2.files if k.startswith("eth.ET_")}
    ref_sd.update({"baseline_model.weight": base.weight.data, "baseline_model.bias": base.bias.data})
    m.load_state_dict(ref_sd)  # a reference checkpoint loads unchanged
    assert torch.equal(m.ET_s_anchor.C_anchor.data, ref_sd["ET_s_anchor.C_anchor"])
    assert m.ET_m_descriptor.traj_normalizer.sca is True and m.ET_s_descriptor.traj_normalizer.sca is False
    for cls, names in ((TrajNorm, ["calculate_params", "get_params", "set_params", "normalize", "denormalize"]),
                       (ETDescriptor, ["normalize_trajectory", "denormalize_trajectory", "to_ET_space",
                                       "to_Euclidean_space", "truncated_SVD", "parameter_initialization", "projection",
                                       "reconstruction", "forward"]),
                       (ETAnchor, ["to_ET_space", "to_Euclidean_space", "anchor_generation", "forward"]),
                       (BatchKMeans, ["calculate_error", "calculate_inertia", "euc_sim", "kmeanspp",
                                      "initialize_centroids", "get_labels", "compute_centroids", "fit", "predict",
                                      "load_state_dict"])):
        for n in names:
            assert callable(getattr(cls, n)), f"{cls.__name__}.{n}"
    km = BatchKMeans(n_clusters=20)
    assert km.centroids is None and km.max_iter == 100 and km.tol == 1e-4 and km.init_mode == "kmeans++"
    km.load_state_dict({"centroids": torch.zeros(1, 6, 20)})
    assert km.centroids.shape == (1, 6, 20)
    a = ETAnchor(hp)
    c = torch.randn(6, 5, 20)
    assert torch.equal(a(c), c)  # zero anchors: identity (anchor.py:87)


def test_augment_and_metrics_helpers():
    from eigentrajectory_amd.utils import augment_trajectory, compute_batch_ade, compute_batch_fde
    z = G.load("g9_metrics.npz")
    np.testing.assert_allclose(compute_batch_ade(torch.from_numpy(z["pred"]), torch.from_numpy(z["gt"])).numpy(),
                               z["ade"], rtol=1e-6)
    np.testing.assert_allclose(compute_batch_fde(torch.from_numpy(z["pred"]), torch.from_numpy(z["gt"])).numpy(),
                               z["fde"], rtol=1e-6)
    o, p, _ = G.dataset("eth", "val")
    ao, ap = augment_trajectory(torch.from_numpy(o), torch.from_numpy(p))
    fo, fp = G.eth_fit_input()
    assert ao.shape[0] == 2 * o.shape[0] and np.array_equal(ao[len(o):, :, 1].numpy(), -o[:, :, 1])
    assert fo.shape == (70316, 8, 2) and fp.shape == (70316, 12, 2)


def test_round2_entry_points_validate_arguments_on_the_host():
    """The entry points added for the sklearn-recipe anchors, the scene path and the sharded drivers reject bad
    arguments before touching a device or RCCL."""
    from eigentrajectory_amd import _lib
    lib = _lib.lib()
    null, i64, f32 = ctypes.c_void_p(0), ctypes.c_int64, ctypes.c_float
    assert lib.et_kmeanspp_workspace_bytes(i64(10_000), 6, 4) > 4 * 10_000 * 5
    assert lib.et_kmeanspp_workspace_bytes(i64(10_000), 6, 9) == 0          # more candidates than 2 + ln(255)
    assert lib.et_kmeanspp_workspace_bytes(i64(0), 6, 4) == 0
    assert lib.et_kmeanspp_seed(null, i64(100), 6, 20, 4, null, null, null, null, ctypes.c_size_t(0), null) == 1
    assert lib.et_center_columns(null, i64(100), 6, f32(1e-4), null, null, null, ctypes.c_size_t(0), null) == 1
    assert lib.et_scene_project(null, i64(0), 8, 6, null, null, 2, f32(0.3), null, null, null, null, null) == 0   # N == 0
    assert lib.et_scene_project(null, i64(5), 8, 6, null, null, 2, f32(0.3), null, null, null, null, null) == 1   # no obs
    assert lib.et_scene_project(null, i64(_lib.SCENE_MAX_N + 1), 8, 6, null, null, 2, f32(0.3), null, null, null, null,
                                null) == 1
    base = lib.et_kmeans_workspace_bytes(i64(4096), 6, 20)
    assert lib.et_kmeans_sharded_workspace_bytes(i64(4096), 6, 20, 8) >= base + 8 * 32
    assert lib.et_kmeans_sharded_workspace_bytes(i64(4096), 6, 20, 0) == 0
    assert lib.et_comm_info(null, null, null) == 1
    assert lib.et_comm_destroy(null) == 0                                      # NULL communicator: nothing to destroy
    assert lib.et_comm_init_rank(null, 2, 0, null) == 1
    assert lib.et_kmeans_fit_sharded(null, i64(10), i64(5), 6, 20, 100, f32(1e-4), null, null, null, null, null, null, null,
                                     null, ctypes.c_size_t(0), null, null) == 1   # N_total < N_local
    assert b"RCCL" in lib.et_status_string(6)


def test_reference_order_shard_geometry_on_the_host():
    """The shard rule of et_kmeans_fit_reforder_sharded (include/eigentraj.h) is host arithmetic: block = 4 L^3 points
    with L the level step of ATen's cascade for N_total / 4 items per lane (SumKernel.cpp: 2^max(4, ceil_log2(n) / 4));
    every rank before the last non-empty one holds whole blocks; anything else has no workspace (= is refused)."""
    import ctypes as C
    from eigentrajectory_amd import _lib as L
    from eigentrajectory_amd import ops
    lib = L.lib()
    block = lambda n: int(lib.et_kmeans_reforder_shard_block(L.i64(n), 6, 20))
    assert block(1023) == 0 and block(1024) == 4 * 16 ** 3
    assert block(4 << 19) == 4 * 16 ** 3 and block((4 << 19) + 4) == 4 * 32 ** 3  # ceil_log2(N / 4) 19 -> 20
    assert block(4 << 23) == 4 * 32 ** 3 and block((4 << 23) + 4) == 4 * 64 ** 3
    assert block(1 << 29) == 0 and int(lib.et_kmeans_reforder_shard_block(L.i64(100000), 5, 20)) == 0

    def ws(sizes, rank, K=20):
        arr = (C.c_int64 * len(sizes))(*sizes)
        return int(lib.et_kmeans_reforder_sharded_workspace_bytes(arr, len(sizes), rank, 6, K))

    for n, world in [(100000, 8), (1000000, 8), (10000000, 8), (50000, 3), (16384, 2), (1024, 4)]:
        sizes = ops.reference_order_shard_sizes(n, world)
        assert sum(sizes) == n and len(sizes) == world
        last = max(i for i, v in enumerate(sizes) if v)
        assert all(v % block(n) == 0 for v in sizes[:last]) and all(v == 0 for v in sizes[last + 1:])
        assert all(ws(sizes, r) > 0 for r in range(world))
    assert ws([25000, 25000], 0) == 0          # a cut inside a block
    assert ws([16384, 0, 1000], 1) > 0         # (an empty rank holds zero blocks wherever it sits)
    assert ws([16384, 1000], 2) == 0 and ws([16384, 1000], 0, K=33) == 0
    assert ws([16384, 16384, 0], 2) > 0        # trailing empty ranks take part in the collectives


def c_type_to_ctypes(spelling):
    """The binding's mapping rule (eigentrajectory_amd/_lib.py); None for a spelling outside it."""
    t = " ".join(spelling.replace("const", " ").split())
    if "*" in t:
        return ctypes.c_char_p if t.replace(" ", "") == "char*" else ctypes.c_void_p
    return {"et_stream_t": ctypes.c_void_p, "et_comm_t": ctypes.c_void_p, "int": ctypes.c_int, "int64_t": ctypes.c_int64,
            "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t}.get(t)


def test_signature_table_matches_the_header():
    """Every prototype of include/eigentraj.h, mapped by the rule, is the table's entry; the prototypes the parser reads
    are all the et_*( names of the header and all the table's keys; lib() declares exactly the table on the handle."""
    from eigentrajectory_amd import _lib
    protos = H.functions()
    assert sorted(protos) == header_functions() == sorted(_lib.SIGNATURES)
    assert list(protos) == list(_lib.SIGNATURES) == _lib.SYMBOLS  # the header's order
    for name, (ret, params) in protos.items():
        mapped = [c_type_to_ctypes(t) for t in [ret] + params]
        assert None not in mapped, f"{name}: C type outside the mapping rule in {[ret] + params}"
        assert _lib.SIGNATURES[name] == (mapped[0], mapped[1:]), name
    lib = _lib.lib()
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_mirrored_constants_equal_the_headers_defines():
    from eigentrajectory_amd import _lib
    d = H.defines()
    mirrored = dict(ET_ABI_VERSION=_lib.ABI_VERSION, ET_OK=_lib.ET_OK, ET_ERR_BAD_DATA=_lib.ET_ERR_BAD_DATA,
                    ET_MODE_STATIC=_lib.MODE_STATIC, ET_MODE_MOVING=_lib.MODE_MOVING, ET_MODE_SPLIT=_lib.MODE_SPLIT,
                    ET_MODE_IDENTITY=_lib.MODE_IDENTITY, ET_MAX_T=_lib.MAX_T, ET_MAX_K=_lib.MAX_K,
                    ET_KMEANS_MAX_D=_lib.KMEANS_MAX_D, ET_KMEANS_MAX_CLUSTERS=_lib.KMEANS_MAX_CLUSTERS,
                    ET_SCENE_MAX_N=_lib.SCENE_MAX_N, ET_CURVE_MAX_FITS=_lib.CURVE_MAX_FITS,
                    ET_STGCNN_MAX_LAYERS=_lib.STGCNN_MAX_LAYERS, ET_SGCN_MAX_LAYERS=_lib.SGCN_MAX_LAYERS,
                    ET_SGCN_MAX_N=_lib.SGCN_MAX_N)
    for name, value in mirrored.items():
        assert d[name] == value, name


def test_binding_refuses_wrong_calls_without_device_work():
    """Declared signatures: a missing argument and a float in an integer slot are errors, and a plain int beyond 32 bits
    reaches an int64_t parameter whole (as does the size_t on the way back)."""
    from eigentrajectory_amd import _lib
    lib = _lib.lib()
    with pytest.raises(TypeError):
        lib.et_kmeans_partials_len(6)
    with pytest.raises(ctypes.ArgumentError):
        lib.et_kmeans_partials_len(6.0, 20)
    assert lib.et_kmeans_workspace_bytes(2**33, 6, 20) > 2**32


def test_call_sites_pass_as_many_arguments_as_the_table_declares():
    """ctypes accepts surplus arguments (cdecl), so the count is checked on the source: every L.call("et_x", ...) and
    every ....et_x(...) of the package whose name is in the table and that spreads no * / ** argument."""
    import ast
    import glob
    from eigentrajectory_amd import _lib
    checked = 0
    for path in sorted(glob.glob(os.path.join(ROOT, "eigentrajectory_amd", "*.py"))):
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if not isinstance(node, ast.Call) or not isinstance(node.func, ast.Attribute):
                continue
            name, args = node.func.attr, node.args
            if (name == "call" and args and isinstance(args[0], ast.Constant) and isinstance(args[0].value, str)
                    and args[0].value.startswith("et_")):
                name, args = args[0].value, args[1:]
                assert name in _lib.SIGNATURES, f"{path}:{node.lineno}: call() of {name}, which the table lacks"
            if name not in _lib.SIGNATURES or node.keywords or any(isinstance(a, ast.Starred) for a in args):
                continue
            assert len(args) == len(_lib.SIGNATURES[name][1]), f"{path}:{node.lineno}: {name}"
            checked += 1
    assert checked >= 70, checked
