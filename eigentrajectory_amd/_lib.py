"""ctypes binding of libetamd.so (C ABI: include/eigentraj.h).

PyTorch is used here only for device memory and streams: every call passes raw
device pointers (``tensor.data_ptr()``) and the current HIP stream across the C
ABI.  There is no CPU fallback: if the shared library is missing, or no HIP
device is present, the operations raise.

``SIGNATURES`` states the C type of every entry point once; ``lib()`` declares them (``argtypes`` / ``restype``) on the
one ``CDLL`` handle everybody shares, so call sites pass plain Python values -- ``data_ptr()`` ints, ``None`` for NULL,
ints and floats, ``byref(struct)`` and ctypes arrays for host-side structs and tables -- and ctypes refuses a missing
argument or a float where an integer or pointer belongs.  ``call(name, ...)`` is the usual way in (it raises on a
non-zero status); the scene-size paths of model.py, where host microseconds are the cost, call ``lib().et_x(...)``
themselves and look at the status inline.  Symbols outside the table (test hooks, the stamp readers of variant builds)
stay reachable as plain attributes of ``lib()``, undeclared.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
#: ET_LIBETAMD selects another build of the library (kernel-variant A/B runs, tools/build_variant.sh)
LIB_PATH = os.environ.get("ET_LIBETAMD") or os.path.join(_HERE, "libetamd.so")

ET_OK = 0
ET_ERR_BAD_DATA = 5
ABI_VERSION = 3  # include/eigentraj.h ET_ABI_VERSION: the struct mirrors below are for this version
MODE_STATIC, MODE_MOVING, MODE_SPLIT, MODE_IDENTITY = 0, 1, 2, 3
MAX_T, MAX_K, KMEANS_MAX_D, KMEANS_MAX_CLUSTERS = 32, 32, 32, 255
SCENE_MAX_N = 16384  # ET_SCENE_MAX_N
CURVE_MAX_FITS = 64  # ET_CURVE_MAX_FITS

# One line per entry point of include/eigentraj.h, in its order: (return type, [argument types]).  const char * / char * ->
# _S; every other pointer, et_stream_t, et_comm_t -> _P; int -> _I; int64_t -> _I64; float -> _F; double -> _D; size_t -> _Z
# (tests/test_host_abi.py holds this table against the header's prototypes).
_P, _S, _I, _I64, _F, _D, _Z = C.c_void_p, C.c_char_p, C.c_int, C.c_int64, C.c_float, C.c_double, C.c_size_t
SIGNATURES = {
    "et_abi_version": (_I, []),
    "et_status_string": (_S, [_I]),
    "et_compiled_arch": (_S, []),
    # ---- tuning switches
    "et_set_option": (_I, [_S, _S]),
    "et_get_option": (_I, [_S, _S, _Z]),
    # ---- TrajNorm
    "et_norm_params": (_I, [_P, _I64, _I, _P, _P, _P, _P]),
    "et_norm_params_from_nrm": (_I, [_P, _I64, _P, _P, _P, _P]),
    "et_normalize": (_I, [_P, _I64, _I, _P, _P, _P, _P, _P]),
    "et_denormalize": (_I, [_P, _I64, _I, _P, _P, _P, _P, _P]),
    # ---- projection
    "et_norm_project": (_I, [_P, _P, _I64, _I, _I, _I, _P, _P, _P, _P, _I, _F, _P, _P, _P, _P, _P]),
    "et_norm_project_pose": (_I, [_P, _P, _I64, _I, _I, _I, _P, _P, _P, _P, _I, _F, _P, _P, _P, _P, _P, _P]),
    "et_scene_project": (_I, [_P, _I64, _I, _I, _P, _P, _I, _F, _P, _P, _P, _P, _P]),
    # ---- training form of a wrapper call on one scene
    "et_scene_project_train": (_I, [_P, _P, _I64, _I, _I, _I, _P, _P, _P, _P, _I, _F, _P, _P, _P, _P, _P, _P]),
    "et_wrapper_losses_fwd": (_I, [_P, _I64, _I, _I, _I, _P, _P, _P, _P, _P, _I, _F, _P, _P, _P, _P, _P, _P, _P]),
    "et_wrapper_losses_bwd": (_I, [_P, _P, _P, _P, _I64, _I, _I, _I, _P, _P, _P, _P, _P, _I, _F, _P, _P, _P, _P, _P, _P]),
    # ---- anchor refinement + reconstruction
    "et_anchor_reconstruct_fwd": (_I, [_P, _I64, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _F, _P, _P]),
    "et_anchor_reconstruct_metrics": (_I, [_P, _I64, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _F, _P, _P, _P, _P]),
    "et_anchor_reconstruct_metrics_pose": (_I, [_P, _I64, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _F, _P, _P, _P, _P]),
    # ---- the reference's test metrics
    "et_traj_metrics": (_I, [_P, _I64, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P]),
    "et_anchor_reconstruct_metrics_scenes": (_I, [_P, _I64, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _F, _P, _P, _I, _P, _P, _P, _P, _P, _P]),
    "et_anchor_reconstruct_bwd": (_I, [_P, _I64, _I, _I, _I, _I, _P, _P, _P, _P, _I, _F, _P, _P]),
    # ---- curve-fitting baselines
    "et_curve_fit_batch_workspace_bytes": (_Z, [_I, _I64]),
    "et_curve_fit_batch": (_I, [_P, _P, _P, _I, _I64, _D, _D, _D, _D, _P, _P, _P, _P, _P, _Z, _P]),
    # ---- t-SNE of descriptor coefficients
    "et_tsne_neighbors": (_I, [_I64, _D]),
    "et_tsne_affinities_workspace_bytes": (_Z, [_I64, _I, _I]),
    "et_tsne_affinities": (_I, [_P, _I64, _I, _D, _I, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "et_tsne_kl_grad_workspace_bytes": (_Z, [_I64]),
    "et_tsne_kl_grad": (_I, [_P, _I64, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "et_tsne_update": (_I, [_P, _P, _P, _P, _I64, _D, _D, _P]),
    "et_tsne_optimize_workspace_bytes": (_Z, [_I64, _I64]),
    "et_tsne_optimize": (_I, [_P, _I64, _P, _P, _P, _I64, _D, _D, _I, _P, _P, _P, _Z, _P]),
    "et_tsne_pca_init_workspace_bytes": (_Z, [_I64, _I]),
    "et_tsne_pca_init": (_I, [_P, _I64, _I, _P, _P, _Z, _P]),
    # ---- Social-STGCNN predictor, inference
    "et_stgcnn_workspace_bytes": (_Z, [_P, _I64, _I64]),
    "et_stgcnn_forward_scenes": (_I, [_P, _P, _P, _I64, _P, _I, _P, _P, _Z, _P]),
    "et_stgcnn_forward_graph": (_I, [_P, _P, _P, _I64, _P, _P, _Z, _P]),
    # ---- SGCN predictor, inference
    "et_sgcn_workspace_bytes": (_Z, [_P, _I64, _I64, _I]),
    "et_sgcn_forward_scenes": (_I, [_P, _P, _P, _I64, _P, _I, _I64, _I64, _P, _P, _P, _P, _Z, _P]),
    "et_sgcn_forward_graph": (_I, [_P, _P, _P, _I, _P, _I, _I64, _P, _P, _P, _P, _Z, _P]),
    # ---- SGCN predictor, training
    "et_sgcn_train_workspace_bytes": (_Z, [_P, _I64, _I64, _I]),
    "et_sgcn_grad_floats": (_I64, [_P]),
    "et_sgcn_train_layout": (_I, [_P, _I64, _I64, _I, _P, _I]),
    "et_sgcn_train_forward_scenes": (_I, [_P, _P, _P, _I64, _P, _I, _I64, _I64, _P, _P, _P, _P, _Z, _P]),
    "et_sgcn_train_forward_graph": (_I, [_P, _P, _P, _I, _P, _I, _I64, _P, _P, _P, _P, _Z, _P]),
    "et_sgcn_backward_scenes": (_I, [_P, _I64, _P, _I, _I64, _I64, _P, _P, _I64, _P, _Z, _P]),
    "et_sgcn_backward_graph": (_I, [_P, _P, _I, _P, _I, _I64, _P, _P, _I64, _P, _Z, _P]),
    # ---- Social-STGCNN predictor, training
    "et_stgcnn_train_workspace_bytes": (_Z, [_P, _I64, _I]),
    "et_stgcnn_grad_floats": (_I64, [_P]),
    "et_stgcnn_train_layout": (_I, [_P, _I64, _I, _P, _I]),
    "et_stgcnn_train_forward_scenes": (_I, [_P, _P, _P, _P, _I64, _P, _I, _P, _P, _Z, _P]),
    "et_stgcnn_train_forward_graph": (_I, [_P, _P, _P, _P, _I64, _P, _P, _Z, _P]),
    "et_stgcnn_backward_scenes": (_I, [_P, _I64, _P, _I, _P, _P, _I64, _P, _Z, _P]),
    "et_stgcnn_backward_graph": (_I, [_P, _I64, _P, _P, _I64, _P, _Z, _P]),
    # ---- GP-Graph-SGCN predictor, inference
    "et_gpgraph_sgcn_workspace_bytes": (_Z, [_P, _I64, _I64, _I]),
    "et_gpgraph_sgcn_forward_graph": (_I, [_P, _P, _P, _I64, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "et_gpgraph_sgcn_forward_scenes": (_I, [_P, _P, _P, _I64, _P, _I, _I64, _I64, _P, _P, _P, _P, _P, _P, _Z, _P]),
    # ---- GP-Graph-SGCN predictor, training
    "et_gpgraph_sgcn_train_workspace_bytes": (_Z, [_P, _I64, _I64, _I]),
    "et_gpgraph_sgcn_grad_floats": (_I64, [_P]),
    "et_gpgraph_sgcn_train_layout": (_I, [_P, _I64, _I64, _I, _P, _I]),
    "et_gpgraph_sgcn_train_forward_scenes": (_I, [_P, _P, _P, _I64, _P, _I, _I64, _I64, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "et_gpgraph_sgcn_train_forward_graph": (_I, [_P, _P, _P, _I64, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "et_gpgraph_sgcn_backward_scenes": (_I, [_P, _I64, _P, _I, _I64, _I64, _P, _P, _I64, _P, _Z, _P]),
    "et_gpgraph_sgcn_backward_graph": (_I, [_P, _I64, _P, _P, _I64, _P, _Z, _P]),
    # ---- GP-Graph-STGCNN predictor, inference
    "et_gpgraph_stgcnn_workspace_bytes": (_Z, [_P, _I64, _I64, _I]),
    "et_gpgraph_stgcnn_forward_graph": (_I, [_P, _P, _P, _I64, _P, _P, _P, _P, _P, _Z, _P]),
    "et_gpgraph_stgcnn_forward_scenes": (_I, [_P, _P, _P, _I64, _P, _I, _I64, _I64, _P, _P, _P, _P, _P, _Z, _P]),
    # ---- DMRGCN predictor, inference
    "et_dmrgcn_workspace_bytes": (_Z, [_P, _I64, _I64]),
    "et_dmrgcn_forward_graph": (_I, [_P, _P, _P, _I64, _P, _P, _Z, _P]),
    "et_dmrgcn_forward_scenes": (_I, [_P, _P, _P, _I64, _P, _I, _P, _P, _P, _Z, _P]),
    # ---- DMRGCN predictor, training
    "et_dmrgcn_train_workspace_bytes": (_Z, [_P, _I64, _I]),
    "et_dmrgcn_grad_floats": (_I64, [_P]),
    "et_dmrgcn_train_layout": (_I, [_P, _I64, _I, _P, _I]),
    "et_dmrgcn_train_forward_graph": (_I, [_P, _P, _P, _I64, _P, _P, _P, _Z, _P]),
    "et_dmrgcn_train_forward_scenes": (_I, [_P, _P, _P, _I64, _P, _I, _P, _P, _P, _P, _Z, _P]),
    "et_dmrgcn_backward_graph": (_I, [_P, _I64, _P, _P, _I64, _P, _Z, _P]),
    "et_dmrgcn_backward_scenes": (_I, [_P, _I64, _P, _I, _P, _P, _I64, _P, _Z, _P]),
    # ---- Social-Implicit predictor, inference
    "et_implicit_workspace_bytes": (_Z, [_P, _I64]),
    "et_implicit_forward_graph": (_I, [_P, _P, _I64, _P, _P, _Z, _P]),
    "et_implicit_forward_scenes": (_I, [_P, _P, _P, _I64, _P, _I, _P, _P, _P, _P, _Z, _P]),
    # ---- Social-Implicit predictor, training
    "et_implicit_backward_workspace_bytes": (_Z, [_P, _I64]),
    "et_implicit_backward_graph": (_I, [_P, _P, _I64, _P, _Z, _P, _I, _P, _P, _Z, _P]),
    "et_implicit_backward_scenes": (_I, [_P, _I64, _P, _Z, _P, _P, _P, _Z, _P]),
    # ---- PECNet / LBEBM predictors, inference
    "et_pecnet_workspace_bytes": (_Z, [_P, _I64]),
    "et_pecnet_predict": (_I, [_P, _P, _P, _P, _P, _I64, _P, _P, _Z, _P]),
    "et_pecnet_forward_scenes": (_I, [_P, _P, _P, _I64, _P, _I, _P, _P, _P, _Z, _P]),
    "et_lbebm_workspace_bytes": (_Z, [_P, _I64]),
    "et_lbebm_predict": (_I, [_P, _P, _P, _I64, _P, _P, _Z, _P]),
    "et_lbebm_forward_scenes": (_I, [_P, _P, _P, _I64, _P, _I, _P, _P, _P, _Z, _P]),
    # ---- LBEBM predictor, training
    "et_lbebm_train_workspace_bytes": (_Z, [_P, _I64]),
    "et_lbebm_train_fwd": (_I, [_P, _P, _I64, _I64, _P, _I64, _I64, _I64, _P, _P, _P, _Z, _P]),
    "et_lbebm_train_bwd": (_I, [_P, _P, _I64, _I64, _P, _I64, _I64, _I64, _P, _P, _P, _P, _P, _P, _Z, _P]),
    # ---- PECNet predictor, training
    "et_pecnet_train_saved_bytes": (_Z, [_P, _I64]),
    "et_pecnet_train_workspace_bytes": (_Z, [_P, _I64]),
    "et_pecnet_train_fwd": (_I, [_P, _P, _I64, _I64, _P, _I64, _I64, _P, _I64, _I64, _P, _I64, _P, _P, _P, _Z, _P]),
    "et_pecnet_train_bwd": (_I, [_P, _P, _I64, _I64, _P, _I64, _I64, _P, _I64, _I64, _P, _I64, _P, _P, _P, _P, _P, _P, _P,
                                 _Z, _P]),
    # ---- AgentFormer predictor, inference
    "et_agentformer_workspace_bytes": (_Z, [_P, _I64, _I64]),
    "et_agentformer_forward_graph": (_I, [_P, _P, _I64, _P, _P, _Z, _P]),
    "et_agentformer_forward_scenes": (_I, [_P, _P, _P, _I64, _P, _I, _P, _P, _P, _Z, _P]),
    # ---- Graph-TERN predictor, inference
    "et_graphtern_workspace_bytes": (_Z, [_P, _I64, _I64]),
    "et_graphtern_forward_graph": (_I, [_P, _P, _I64, _P, _P, _Z, _P]),
    "et_graphtern_forward_scenes": (_I, [_P, _P, _P, _I64, _P, _I, _P, _P, _P, _Z, _P]),
    # ---- Graph-TERN predictor, training
    "et_graphtern_train_workspace_bytes": (_Z, [_P, _I64, _I]),
    "et_graphtern_grad_floats": (_I64, [_P]),
    "et_graphtern_train_layout": (_I, [_P, _I64, _I, _P, _I]),
    "et_graphtern_train_forward_graph": (_I, [_P, _P, _I64, _P, _P, _P, _Z, _P]),
    "et_graphtern_train_forward_scenes": (_I, [_P, _P, _P, _I64, _P, _I, _P, _P, _P, _P, _Z, _P]),
    "et_graphtern_backward_graph": (_I, [_P, _I64, _P, _P, _I64, _P, _Z, _P]),
    "et_graphtern_backward_scenes": (_I, [_P, _I64, _P, _I, _P, _P, _I64, _P, _Z, _P]),
    # ---- fit
    "et_fit_gram_workspace_bytes": (_Z, [_I64, _I, _I]),
    "et_fit_gram": (_I, [_P, _P, _I64, _I, _I, _I, _F, _I, _P, _P, _P, _P, _Z, _P]),
    "et_fit_descriptor_workspace_bytes": (_Z, [_I64, _I, _I]),
    "et_fit_descriptor": (_I, [_P, _P, _I64, _I, _I, _I, _I, _F, _I, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "et_eigh_topk": (_I, [_P, _I, _I, _P, _P, _P]),
    "et_eigh_topk_batch": (_I, [_I, _P, _P, _P, _P, _P, _P]),
    # ---- BatchKMeans
    "et_euc_sim": (_I, [_P, _P, _I, _I64, _I64, _P, _P]),
    "et_euc_sim_batch": (_I, [_P, _P, _I64, _I, _I64, _I64, _P, _P]),
    "et_kmeans_partials_len": (_Z, [_I, _I]),
    "et_kmeans_workspace_bytes": (_Z, [_I64, _I, _I]),
    "et_kmeans_scan": (_I, [_P, _I64, _I, _P, _P]),
    "et_kmeans_begin": (_I, [_P, _I64, _P, _I, _I, _P]),
    "et_kmeans_init_step": (_I, [_P, _I64, _I, _I, _I, _P, _P, _I64, _P, _P, _Z, _P]),
    "et_kmeans_init_set": (_I, [_P, _I, _I, _I, _P, _P]),
    "et_kmeans_init_select": (_I, [_P, _I, _I, _I, _I, _I, _P, _P]),
    "et_kmeans_gather_point": (_I, [_P, _I64, _I, _I64, _P, _P]),
    "et_kmeans_init_farthest": (_I, [_P, _I64, _I, _I, _I64, _P, _P, _Z, _P]),
    "et_kmeans_assign_accumulate": (_I, [_P, _I64, _I, _I, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "et_kmeans_update": (_I, [_P, _P, _I, _I, _F, _P, _P, _P]),
    "et_kmeans_joint_done": (_I, [_P, _I, _F, _P]),
    "et_kmeans_labels_i64": (_I, [_P, _I64, _P, _P]),
    "et_kmeans_fit": (_I, [_P, _I64, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "et_kmeans_batch_workspace_bytes": (_Z, [_I64, _I, _I, _I64]),
    "et_kmeans_fit_batch": (_I, [_P, _I64, _I64, _I, _I, _I64, _I, _F, _P, _P, _P, _P, _Z, _P]),
    # ---- opt-in: BatchKMeans in the reference's own fp32 summation orders
    "et_kmeans_reforder_workspace_bytes": (_Z, [_I64, _I, _I]),
    "et_euc_sim_reforder": (_I, [_P, _P, _I, _I64, _I64, _P, _P]),
    "et_kmeans_init_farthest_reforder": (_I, [_P, _I64, _I, _I, _I64, _P, _P, _Z, _P]),
    "et_kmeans_predict_reforder": (_I, [_P, _I64, _I, _P, _I, _P, _P, _P, _Z, _P]),
    "et_kmeans_fit_reforder": (_I, [_P, _I64, _I, _I, _I, _F, _P, _P, _P, _P, _P, _Z, _P]),
    "et_kmeans_reforder_batch_workspace_bytes": (_Z, [_I64, _I, _I, _I64]),
    "et_kmeans_fit_reforder_batch": (_I, [_P, _I64, _I64, _I, _I, _I64, _I, _F, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "et_kmeans_predict": (_I, [_P, _I64, _I, _P, _I, _P, _P, _P]),
    "et_kmeans_predict_batch": (_I, [_P, _I64, _I64, _I64, _I, _P, _I, _P, _P, _P]),
    # ---- anchor clustering as the reference runs it
    "et_center_columns": (_I, [_P, _I64, _I, _F, _P, _P, _P, _Z, _P]),
    "et_kmeanspp_workspace_bytes": (_Z, [_I64, _I, _I]),
    "et_kmeanspp_seed": (_I, [_P, _I64, _I, _I, _I, _P, _P, _P, _P, _Z, _P]),
    "et_kmeanspp_batch_workspace_bytes": (_Z, [_I64, _I, _I, _I64]),
    "et_kmeanspp_seed_batch": (_I, [_P, _I64, _I, _I, _I, _P, _I64, _P, _P, _P, _Z, _P]),
    # ---- data-sharded fit and k-means (RCCL)
    "et_comm_load": (_I, [_S]),
    "et_comm_unique_id": (_I, [_P]),
    "et_comm_init_rank": (_I, [_P, _I, _I, _P]),
    "et_comm_destroy": (_I, [_P]),
    "et_comm_info": (_I, [_P, _P, _P]),
    "et_fit_gram_sharded": (_I, [_P, _P, _I64, _I, _I, _I, _F, _I, _P, _P, _P, _P, _Z, _P, _P]),
    "et_kmeans_sharded_workspace_bytes": (_Z, [_I64, _I, _I, _I]),
    "et_kmeans_init_farthest_sharded": (_I, [_P, _I64, _I, _I, _I64, _I64, _P, _P, _P, _Z, _P, _P]),
    "et_kmeans_fit_sharded": (_I, [_P, _I64, _I64, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P, _P]),
    "et_kmeans_reforder_shard_block": (_I64, [_I64, _I, _I]),
    "et_kmeans_reforder_sharded_workspace_bytes": (_Z, [_P, _I, _I, _I, _I]),
    "et_kmeans_fit_reforder_sharded": (_I, [_P, _P, _I, _I, _I, _I, _I, _F, _P, _P, _P, _P, _P, _Z, _P, _P]),
}
#: every symbol include/eigentraj.h declares (tests check the library exports all of them)
SYMBOLS = list(SIGNATURES)


class KMeansState(C.Structure):
    """Mirror of ``et_kmeans_state`` (include/eigentraj.h)."""
    _fields_ = [("max_abs_x", C.c_double), ("max_abs_c", C.c_double), ("n_total", C.c_int64), ("frac", C.c_int64),
                ("sim_frac", C.c_int64), ("iter", C.c_int64), ("done", C.c_int64), ("bad_input", C.c_int64),
                ("error", C.c_double), ("inertia", C.c_double), ("fast_ok", C.c_int64),
                ("min_nz_x_bits", C.c_int64)]


class KMeansTiming(C.Structure):
    """Mirror of ``et_kmeans_timing``."""
    _fields_ = [("assign_ms", C.c_double), ("assign_launches", C.c_int64), ("first_assign_ms", C.c_double),
                ("iterations", C.c_int64)]


STGCNN_MAX_LAYERS = 8  # ET_STGCNN_MAX_LAYERS


class STGCNNLayer(C.Structure):
    """Mirror of ``et_stgcnn_layer``: device pointers to one st_gcn block's tensors (field order: include/eigentraj.h)."""
    _fields_ = [(name, C.c_void_p) for name in (
        "gcn_w", "gcn_b", "bn1_w", "bn1_b", "bn1_mean", "bn1_var", "prelu1", "tcn_w", "tcn_b", "bn2_w", "bn2_b",
        "bn2_mean", "bn2_var", "res_w", "res_b", "res_bn_w", "res_bn_b", "res_bn_mean", "res_bn_var", "prelu")]


class STGCNNParams(C.Structure):
    """Mirror of ``et_stgcnn_params``."""
    _fields_ = [("n_stgcnn", C.c_int), ("n_txpcnn", C.c_int), ("input_feat", C.c_int), ("output_feat", C.c_int),
                ("seq_len", C.c_int), ("pred_seq_len", C.c_int), ("kernel_size", C.c_int), ("bn_eps", C.c_float),
                ("st_gcns", STGCNNLayer * STGCNN_MAX_LAYERS), ("tpcnn_w", C.c_void_p * STGCNN_MAX_LAYERS),
                ("tpcnn_b", C.c_void_p * STGCNN_MAX_LAYERS), ("prelus", C.c_void_p * STGCNN_MAX_LAYERS),
                ("out_w", C.c_void_p), ("out_b", C.c_void_p)]


STGCNN_TRAIN_LAYOUT_FIELDS = 26  # ET_STGCNN_TRAIN_LAYOUT_FIELDS
# ... by name, in the C enum's order (include/eigentraj.h names them in et_stgcnn_train_layout's comment)
STGCNN_TRAIN_LAYOUT_NAMES = ("u", "d", "P", "g", "a1", "y", "t", "r", "s", "x", "tp", "dfin", "dtp", "dx", "ds", "dt", "dr", "dy",
                             "da1", "dg", "per", "stats", "stat_stride", "partials", "grads", "total")


class STGCNNTrain(C.Structure):
    """Mirror of ``et_stgcnn_train``: what training adds to ``et_stgcnn_params`` -- the BatchNorm momentum, the writable
    running statistics of st_gcns.0's three BatchNorms and their num_batches_tracked (int64)."""
    _fields_ = [("momentum", C.c_float)] + [(name, C.c_void_p) for name in (
        "bn1_mean", "bn1_var", "bn2_mean", "bn2_var", "res_bn_mean", "res_bn_var", "bn1_batches", "bn2_batches",
        "res_bn_batches")]


SGCN_MAX_LAYERS = 8  # ET_SGCN_MAX_LAYERS
SGCN_MAX_N = 512     # ET_SGCN_MAX_N
SGCN_TRAIN_LAYOUT_FIELDS = 24  # ET_SGCN_TRAIN_LAYOUT_FIELDS
SGCN_TRAIN_LAYOUT_NAMES = ("v", "rows_s", "rows_t", "stack_s", "stack_s_stride", "stack_t", "stack_t_stride", "at", "f2", "f1",
                           "ts", "keep", "keep_stride", "d_at", "d_f1", "d_ts", "d_f2", "rrec", "g_s", "g_t", "dir_s", "dir_t",
                           "dd_s", "total")  # the C enum's order
SGCN_BWD_CHUNK = 4     # ET_SGCN_BWD_CHUNK: pedestrians whose tail gradients one workgroup adds, in row order
SGCN_BWD_ROWS = 1024   # ET_SGCN_BWD_ROWS: softmax rows per workgroup of the row kernels
SGCN_BWD_ITEMS = 4096  # ET_SGCN_BWD_ITEMS: stack positions / entries per workgroup of the asym and fuse kernels
GPGRAPH_SGCN_TRAIN_LAYOUT_FIELDS = 49  # ET_GPGRAPH_SGCN_TRAIN_LAYOUT_FIELDS
GPGRAPH_SGCN_TRAIN_LAYOUT_NAMES = SGCN_TRAIN_LAYOUT_NAMES[:-1] + (  # SGCN's without its total, then the wrapper's
    "vp", "vn", "gidx", "dax", "srec", "trec", "dacct", "dxas", "dxp", "dxv", "va", "feat", "dist", "sn", "po", "sig", "cs", "cnt",
    "dmix", "dpo", "dvp", "dP", "dsig", "dd", "df", "total")
GPGRAPH_BWD_ROWS = 64  # ET_GPGRAPH_BWD_ROWS: pedestrians per workgroup partial of the mix weights' gradients


class SGCNAttention(C.Structure):
    """Mirror of ``et_sgcn_attention`` (field order: include/eigentraj.h)."""
    _fields_ = [(name, C.c_void_p) for name in ("emb_w", "emb_b", "q_w", "q_b", "k_w", "k_b")]


class SGCNAsym(C.Structure):
    """Mirror of ``et_sgcn_asym``."""
    _fields_ = [(name, C.c_void_p) for name in ("conv1_w", "conv2_w", "conv2_b", "act")]


class SGCNGcn(C.Structure):
    """Mirror of ``et_sgcn_gcn``."""
    _fields_ = [(name, C.c_void_p) for name in ("w", "act")]


class SGCNParams(C.Structure):
    """Mirror of ``et_sgcn_params``."""
    _fields_ = [("n_asym", C.c_int), ("embedding_dims", C.c_int), ("n_gcn_layers", C.c_int), ("obs_len", C.c_int),
                ("pred_len", C.c_int), ("n_tcn", C.c_int), ("in_dims", C.c_int), ("out_dims", C.c_int),
                ("num_heads", C.c_int), ("dropout", C.c_float),
                ("att", SGCNAttention * 2), ("fus_w", C.c_void_p), ("fus_b", C.c_void_p), ("fus_a", C.c_void_p),
                ("asym_s", SGCNAsym * SGCN_MAX_LAYERS), ("asym_t", SGCNAsym * SGCN_MAX_LAYERS), ("gcn", SGCNGcn * 4),
                ("fusion_w", C.c_void_p), ("tcn_w", C.c_void_p * SGCN_MAX_LAYERS), ("tcn_b", C.c_void_p * SGCN_MAX_LAYERS),
                ("tcn_a", C.c_void_p * SGCN_MAX_LAYERS), ("out_w", C.c_void_p), ("out_b", C.c_void_p)]


class GPGraphSGCNParams(C.Structure):
    """Mirror of ``et_gpgraph_sgcn_params``."""
    _fields_ = [("base", SGCNParams), ("group_w", C.c_void_p), ("group_b", C.c_void_p), ("th", C.c_void_p),
                ("tau", C.c_float), ("mix_a", C.c_void_p), ("mix_w", C.c_void_p), ("mix_b", C.c_void_p)]


class GPGraphSTGCNNParams(C.Structure):
    """Mirror of ``et_gpgraph_stgcnn_params``."""
    _fields_ = [("base", STGCNNParams), ("group_w", C.c_void_p), ("group_b", C.c_void_p), ("th", C.c_void_p),
                ("tau", C.c_float), ("mix_a", C.c_void_p), ("mix_w", C.c_void_p), ("mix_b", C.c_void_p)]


DMRGCN_MAX_STGCN = 4  # ET_DMRGCN_MAX_STGCN
DMRGCN_MAX_TPCNN = 8  # ET_DMRGCN_MAX_TPCNN
DMRGCN_BINS = 5       # ET_DMRGCN_BINS
DMRGCN_TRAIN_MAX_N = 512          # ET_DMRGCN_TRAIN_MAX_N
DMRGCN_TRAIN_LAYOUT_FIELDS = 16   # ET_DMRGCN_TRAIN_LAYOUT_FIELDS
DMRGCN_TRAIN_LAYOUT_NAMES = ("u", "P", "yp", "s", "x", "tp", "dtp", "dx", "dy", "arena", "per", "tp_stride", "dtp_stride",
                             "partials", "grads", "total")  # the C enum's order


class DMRGCNLayer(C.Structure):
    """Mirror of ``et_dmrgcn_layer``: device pointers to one st_dmrgcn block's tensors (field order: include/eigentraj.h)."""
    _fields_ = [("gcn_w", C.c_void_p * 2), ("gcn_b", C.c_void_p * 2)] + [(name, C.c_void_p) for name in (
        "tcn_prelu", "tcn_w", "tcn_b", "res_w", "res_b", "prelu")]


class DMRGCNTpcnn(C.Structure):
    """Mirror of ``et_dmrgcn_tpcnn``: device pointers to one tpcnn block's tensors."""
    _fields_ = [("conv_w", C.c_void_p * 2), ("conv_b", C.c_void_p * 2), ("conv_a", C.c_void_p * 2)] + [
        (name, C.c_void_p) for name in ("gta_w", "gta_b", "gta_a", "res_w", "res_b")]


class DMRGCNParams(C.Structure):
    """Mirror of ``et_dmrgcn_params``."""
    _fields_ = [("n_stgcn", C.c_int), ("n_tpcnn", C.c_int), ("input_feat", C.c_int), ("output_feat", C.c_int),
                ("seq_len", C.c_int), ("pred_seq_len", C.c_int), ("kernel_size", C.c_int),
                ("split", (C.c_float * DMRGCN_BINS) * 2), ("st_dmrgcns", DMRGCNLayer * DMRGCN_MAX_STGCN),
                ("tpcnns", DMRGCNTpcnn * DMRGCN_MAX_TPCNN)]


IMPLICIT_MAX_BINS = 8  # ET_IMPLICIT_MAX_BINS
IMPLICIT_BWD_CHUNK = 8  # ET_IMPLICIT_BWD_CHUNK: rows whose gradient terms one workgroup adds, in row order


class ImplicitCell(C.Structure):
    """Mirror of ``et_implicit_cell``: device pointers to one Social-Zone cell's tensors (order: include/eigentraj.h)."""
    _fields_ = [("global_t", C.c_void_p * 8), ("local_t", C.c_void_p * 8), ("noise_w", C.c_void_p),
                ("global_w", C.c_void_p), ("local_w", C.c_void_p)]


class ImplicitParams(C.Structure):
    """Mirror of ``et_implicit_params``."""
    _fields_ = [("spatial_input", C.c_int), ("spatial_output", C.c_int), ("temporal_input", C.c_int),
                ("temporal_output", C.c_int), ("n_bins", C.c_int), ("bins", C.c_float * IMPLICIT_MAX_BINS),
                ("cells", ImplicitCell * IMPLICIT_MAX_BINS)]


MLP_MAX_LAYERS = 5    # ET_MLP_MAX_LAYERS
MLP_MAX_WIDTH = 1024  # ET_MLP_MAX_WIDTH
MLP_MAX_POOLS = 8     # ET_MLP_MAX_POOLS
MLP_MAX_RANGE = 4096  # ET_MLP_MAX_RANGE


class MLPChain(C.Structure):
    """Mirror of ``et_mlp_chain``: one chain of Linear + ReLU, device pointers to its weights and biases."""
    _fields_ = [("n_layers", C.c_int), ("widths", C.c_int * (MLP_MAX_LAYERS + 1)), ("w", C.c_void_p * MLP_MAX_LAYERS),
                ("b", C.c_void_p * MLP_MAX_LAYERS)]


class MLPParams(C.Structure):
    """Mirror of ``et_mlp_params`` (PECNet and LBEBM)."""
    _fields_ = [("fdim", C.c_int), ("nonlocal_pools", C.c_int), ("non_local_dim", C.c_int), ("out_width", C.c_int),
                ("pos_width", C.c_int)] + [(name, MLPChain) for name in (
                    "encoder_past", "encoder_dest", "non_local_theta", "non_local_phi", "non_local_g", "predictor")]


AGENTFORMER_MAX_LAYERS = 4     # ET_AGENTFORMER_MAX_LAYERS
AGENTFORMER_MAX_SCENE_N = 128  # ET_AGENTFORMER_MAX_SCENE_N


class MLPChainGrads(C.Structure):
    """Mirror of ``et_mlp_chain_grads``: where one chain's weight and bias gradients go (device pointers)."""
    _fields_ = [("dw", C.c_void_p * MLP_MAX_LAYERS), ("db", C.c_void_p * MLP_MAX_LAYERS)]


class LBEBMGrads(C.Structure):
    """Mirror of ``et_lbebm_grads``."""
    _fields_ = [(name, MLPChainGrads) for name in ("encoder_past", "encoder_dest", "predictor")]


class PECNetGrads(C.Structure):
    """Mirror of ``et_pecnet_grads``."""
    _fields_ = [(name, MLPChainGrads) for name in ("encoder_past", "encoder_dest", "non_local_theta", "non_local_phi",
                                                   "non_local_g", "predictor")]


class AgentFormerAttn(C.Structure):
    """Mirror of ``et_agentformer_attn``: device pointers to one AgentAwareAttention's tensors."""
    _fields_ = [(name, C.c_void_p) for name in ("in_proj_weight", "in_proj_bias", "in_proj_weight_self",
                                                "in_proj_bias_self", "out_proj_weight", "out_proj_bias")]


class AgentFormerLayer(C.Structure):
    """Mirror of ``et_agentformer_layer`` (``multihead_attn`` and the third norm: decoder layers only)."""
    _fields_ = [("self_attn", AgentFormerAttn), ("multihead_attn", AgentFormerAttn), ("linear1_weight", C.c_void_p),
                ("linear1_bias", C.c_void_p), ("linear2_weight", C.c_void_p), ("linear2_bias", C.c_void_p),
                ("norm_weight", C.c_void_p * 3), ("norm_bias", C.c_void_p * 3)]


class AgentFormerEmbed(C.Structure):
    """Mirror of ``et_agentformer_embed``."""
    _fields_ = [(name, C.c_void_p) for name in ("input_fc_weight", "input_fc_bias", "fc_weight", "fc_bias", "pe")]


class AgentFormerParams(C.Structure):
    """Mirror of ``et_agentformer_params``."""
    _fields_ = [(name, C.c_int) for name in ("motion_dim", "model_dim", "ff_dim", "nhead", "forecast_dim", "past_frames",
                                             "future_frames", "n_enc", "n_dec")] + [
        ("enc_embed", AgentFormerEmbed), ("dec_embed", AgentFormerEmbed), ("out_fc_weight", C.c_void_p),
        ("out_fc_bias", C.c_void_p), ("enc", AgentFormerLayer * AGENTFORMER_MAX_LAYERS),
        ("dec", AgentFormerLayer * AGENTFORMER_MAX_LAYERS)]


GRAPHTERN_MAX_EPGCN = 4  # ET_GRAPHTERN_MAX_EPGCN
GRAPHTERN_MAX_EPCNN = 8  # ET_GRAPHTERN_MAX_EPCNN
GRAPHTERN_REL = 4        # relations per time row: [A_abs, A_rel, 1/A_abs, 1/A_rel]
GRAPHTERN_TRAIN_MAX_N = 512          # ET_GRAPHTERN_TRAIN_MAX_N
GRAPHTERN_TRAIN_LAYOUT_FIELDS = 16   # ET_GRAPHTERN_TRAIN_LAYOUT_FIELDS
GRAPHTERN_TRAIN_LAYOUT_NAMES = ("u", "d", "P", "yp", "x0", "tp", "dtp", "dx0", "dy", "arena", "per", "tp_stride", "dtp_stride",
                                "partials", "grads", "total")  # the C enum's order


class GraphTERNLayer(C.Structure):
    """Mirror of ``et_graphtern_layer``: device pointers to one st_mrgcn block's tensors (field order: include/eigentraj.h)."""
    _fields_ = [(name, C.c_void_p) for name in ("gcn_w", "gcn_b", "tcn_prelu", "tcn_w", "tcn_b", "res_w", "res_b", "prelu")]


class GraphTERNEpcnn(C.Structure):
    """Mirror of ``et_graphtern_epcnn``: device pointers to one epcnn block's tensors."""
    _fields_ = [(name, C.c_void_p) for name in ("tpcn_w", "tpcn_b", "tpcn_a", "cpcn_w", "cpcn_b", "cpcn_a", "rest_w",
                                                "rest_b", "resc_w", "resc_b")]


class GraphTERNParams(C.Structure):
    """Mirror of ``et_graphtern_params``."""
    _fields_ = [(name, C.c_int) for name in ("n_epgcn", "n_epcnn", "input_feat", "hidden_feat", "seq_len", "pred_seq_len",
                                             "n_smpl")] + [
        ("tp_mrgcns", GraphTERNLayer * GRAPHTERN_MAX_EPGCN), ("tpcnns", GraphTERNEpcnn * GRAPHTERN_MAX_EPCNN)]


STATE_BYTES = C.sizeof(KMeansState)
_lib = None


class ETLibraryError(RuntimeError):
    pass


def lib():
    """Load libetamd.so (built in-tree by ``__graft_entry__.build()`` / ``make -C eigentrajectory_amd/csrc``)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ETLibraryError(
                f"{LIB_PATH} is missing: build the HIP kernels first (python -c 'import __graft_entry__ as g; "
                "g.build()' or make -C eigentrajectory_amd/csrc).  eigentrajectory_amd has no CPU fallback.")
        l = C.CDLL(LIB_PATH)
        if l.et_abi_version() != ABI_VERSION:
            raise ETLibraryError(f"{LIB_PATH} has ABI version {l.et_abi_version()}, this binding is for {ABI_VERSION}: "
                                 "rebuild the library (make -C eigentrajectory_amd/csrc)")
        for name, (restype, argtypes) in SIGNATURES.items():
            try:
                fn = getattr(l, name)
            except AttributeError:
                raise ETLibraryError(f"{LIB_PATH} does not export {name}, which include/eigentraj.h declares: rebuild the "
                                     "library (make -C eigentrajectory_amd/csrc)") from None
            fn.restype, fn.argtypes = restype, argtypes
        _lib = l
        # the library reads nothing from the environment; ET_OPT_<KEY>=value is forwarded once, here (A/B scripts under tools/)
        # every variable is applied; the ones the library rejects are named in ONE warning (never an exception out of
        # whichever unrelated call happened to load the library)
        rejected = []
        for name, value in sorted(os.environ.items()):
            if name.startswith("ET_OPT_") and l.et_set_option(name[len("ET_OPT_"):].lower().encode(), value.encode()) != ET_OK:
                rejected.append(f"{name}={value}")
        if rejected:
            import warnings
            warnings.warn("eigentrajectory_amd: et_set_option rejected " + ", ".join(rejected) +
                          " (unknown key or value; the other ET_OPT_ variables were applied)", RuntimeWarning, stacklevel=2)
    return _lib


def set_option(key: str, value) -> None:
    """et_set_option (include/eigentraj.h, "tuning switches"): measurement aids / test levers; never needed for results."""
    rc = lib().et_set_option(str(key).encode(), str(value).encode())
    if rc != ET_OK:
        raise ValueError(f"et_set_option({key!r}, {value!r}): unknown key or value")


def get_option(key: str) -> str:
    buf = C.create_string_buffer(64)
    if lib().et_get_option(str(key).encode(), buf, 64) != ET_OK:
        raise ValueError(f"et_get_option({key!r}): unknown key")
    return buf.value.decode()


class option:
    """``with option("kmeans_packed", 0): ...`` -- set a switch for a block and put the old value back."""

    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        self.old = get_option(self.key)
        set_option(self.key, self.value)
        return self

    def __exit__(self, *exc):
        set_option(self.key, self.old)
        return False


def check(rc: int, what: str):
    if rc != ET_OK:
        msg = lib().et_status_string(rc).decode()
        if rc in (1, ET_ERR_BAD_DATA):
            raise ValueError(f"{what}: {msg}")
        raise ETLibraryError(f"{what}: {msg} (status {rc})")


def call(name: str, *args):
    """Call the status-returning entry point ``name`` and raise what :func:`check` raises for its status."""
    check(getattr(lib(), name)(*args), name)


def require_device(*tensors):
    """Return the HIP device the call runs on; raise when there is none (no CPU path)."""
    for t in tensors:
        if t is not None and t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise ETLibraryError("eigentrajectory_amd needs a HIP device (MI355X); no CPU fallback is provided")
    return torch.device("cuda", torch.cuda.current_device())


def on_device(t, device, dtype=torch.float32):
    """Contiguous ``dtype`` copy/view of ``t`` on ``device`` (None passes through)."""
    if t is None:
        return None
    t = t.detach()
    if t.device != device or t.dtype != dtype:
        t = t.to(device=device, dtype=dtype)
    return t.contiguous()


def ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _p(t):
    """A module tensor's address for a ``c_void_p`` field of the params mirrors: a plain int, which costs less than
    :func:`ptr`'s ``c_void_p`` object on the per-scene path (a module's tensor is never None)."""
    return t.data_ptr()


def module_device(who, *modules, buffers=False, device=None):
    """-> the ONE HIP device every parameter of ``modules`` (with ``buffers`` also every floating-point buffer) lives on as
    a contiguous float32 tensor: the placement check every predictor's ``et_params()`` opens with (``who``: its class
    name).  ``device``: a device already established (GP-Graph's base model) that they must share."""
    tensors = [t for m in modules for t in m.parameters()]
    if buffers:
        tensors += [b for m in modules for b in m.buffers() if b.is_floating_point()]
    dev = tensors[0].device if device is None else device
    if dev.type != "cuda" or any(t.device != dev or t.dtype != torch.float32 or not t.is_contiguous() for t in tensors):
        raise ETLibraryError(f"{who}: every parameter{' and buffer' if buffers else ''} must be a contiguous float32 tensor "
                             "on ONE HIP device (model.cuda()); there is no CPU path")
    return dev


def stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def i64(v):
    return C.c_int64(int(v))


def f32(v):
    return C.c_float(float(v))


try:
    _raw_stream = torch._C._cuda_getCurrentRawStream  # the current stream's hipStream_t as an int, ~0.2 us
except AttributeError:  # pragma: no cover - older / newer torch without the private accessor
    def _raw_stream(device_index):
        return torch.cuda.current_stream(device_index).cuda_stream


def raw_stream(device_index):
    return _raw_stream(device_index)
