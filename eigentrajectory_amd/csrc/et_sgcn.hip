// et_sgcn.hip -- SGCN inference (baseline/sgcn: bridge.py pre-hook, model.py TrajectoryModel.forward in eval mode with
// dropout 0, bridge.py post-hook) for the ET configuration family (include/eigentraj.h "SGCN predictor").
//
// Layered form.  The dense stacks of a scene are (T,4,n,n) floats -- 416 KB at the largest ETH/UCY test scene (n = 57),
// more than a workgroup's LDS -- and spa_fusion mixes all T slices of an entry while the asymmetric convolutions need the
// neighbours within a slice, so the stacks live in two ping-pong buffers of the caller's workspace and every layer is one
// launch over all scenes (grid: scene x chunk).  Per call, for any number of scenes:
//   prep    1 workgroup     the attention collapsed: with one input channel q_i = x_i aq + cq and k_j = x_j ak + ck, so
//                           q_i . k_j = x_j (x_i aq.ak + cq.ak) + (terms constant along the softmax axis); per head the
//                           two scalars alpha = aq.ak / 8 and beta = cq.ak / 8 are formed in fp64
//   input   per scene       v = [C_obs; obs_ori] (or the given graph), the scene's offset into the stacks, and per
//                           softmax row its maximum and its sum (the dense attention is never stored: an entry is
//                           exp(t_i x_j - max_i) / sum_i wherever it is needed)
//   fuse    per entry       spa_fusion over T + PReLU + shortcut -> spatial stack; the temporal stack is the attention
//   asym    x layers        PReLU(conv(1x3) + conv(3x1)) + x on both stacks; the last layer's output are the logits
//   tadj    per row         temporal mask, ZeroSoftmax -> A_t (n,4,T,T); temporal_spatial gcn 0
//   sadj    per row         spatial mask, ZeroSoftmax folded into the two products that use A_s (A_s itself is never
//                           stored): spatial_temporal gcn 0 and temporal_spatial gcn 1
//   tail    per pedestrian  spatial_temporal gcn 1, fusion_, the tcns and the output layer in one wavefront's LDS
// Every sum runs in a fixed order inside one lane, so results do not depend on the launch geometry or on the other scenes.
// The kernels themselves are in et_sgcn_core.inl, which et_gpgraph.hip (GP-Graph-SGCN) shares.  Training (the kept-layout
// forward and the backward pass to every parameter) is et_sgcn_train.inl.
#include "et_common.h"

namespace et {
namespace {

#include "et_sgcn_core.inl"

static int run(const et_sgcn_params &p, const float *gv, const Ident &I, const float *C_obs, const float *nrm, int64_t N,
               const int32_t *off, int n_scenes, int64_t sum_n2, int64_t max_n, float *out, float *logit_s,
               float *logit_t, void *workspace, size_t workspace_bytes, hipStream_t st) {
    const int T = p.obs_len;
    Ctx c;
    c.off = off;
    c.N = N;
    c.n2cap = sum_n2;
    c.S = n_scenes;
    c.T = T;
    c.ws = (float *)workspace;
    c.L = lay_of(T, N, sum_n2, n_scenes);
    c.Nr = N;
    c.Sr = n_scenes;
    if (!workspace || workspace_bytes < (size_t)c.L.total * 4) return ET_ERR_WORKSPACE;
    hipLaunchKernelGGL(sgcn_prep<false>, dim3(1), dim3(kSnThreads), 0, st, p, c.ws);
    run_layers<false>(p, c, gv, I, C_obs, nrm, max_n, out, logit_s, logit_t, st);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

#include "et_sgcn_train.inl"

}  // namespace
}  // namespace et

using namespace et;

extern "C" size_t et_sgcn_workspace_bytes(const et_sgcn_params *params, int64_t N, int64_t sum_n2, int n_scenes) {
    if (check_params(params) != ET_OK || N <= 0 || sum_n2 < 0 || n_scenes < 0) return 0;
    return (size_t)lay_of(params->obs_len, N, sum_n2, n_scenes).total * 4;
}

extern "C" int et_sgcn_forward_scenes(const et_sgcn_params *params, const float *C_obs, const float *nrm, int64_t N,
                                      const int32_t *scene_offsets, int n_scenes, int64_t sum_n2, int64_t max_scene_n,
                                      float *C_pred_refine, float *logit_s, float *logit_t, void *workspace,
                                      size_t workspace_bytes, et_stream_t stream) {
    const int rc = check_params(params);
    if (rc != ET_OK) return rc;
    if (sum_n2 < 0 || max_scene_n < 0) return ET_ERR_INVALID_ARG;
    const int early = scene_args_status(N, INT32_MAX, scene_offsets, n_scenes, ET_SGCN_MAX_N);
    if (early != kSceneArgsGo) return early;
    if (!C_obs || !nrm || !C_pred_refine) return ET_ERR_INVALID_ARG;
    if (!scene_offsets) {
        n_scenes = 1;
        sum_n2 = N * N;
        max_scene_n = N;
    }
    if (max_scene_n > ET_SGCN_MAX_N) max_scene_n = ET_SGCN_MAX_N;  // larger scenes are not computed
    const Ident I{nullptr, nullptr, 1, 1};
    return run(*params, nullptr, I, C_obs, nrm, N, scene_offsets, n_scenes, sum_n2, max_scene_n, C_pred_refine, logit_s,
               logit_t, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int et_sgcn_forward_graph(const et_sgcn_params *params, const float *v, const float *identity_s, int id_s_t,
                                     const float *identity_t, int id_t_t, int64_t N, float *out, float *logit_s,
                                     float *logit_t, void *workspace, size_t workspace_bytes, et_stream_t stream) {
    const int rc = check_params(params);
    if (rc != ET_OK) return rc;
    if (N < 0 || N > ET_SGCN_MAX_N) return ET_ERR_INVALID_ARG;
    if (N == 0) return ET_OK;
    const int T = params->obs_len;
    if (!v || !identity_s || !identity_t || !out || (id_s_t != 1 && id_s_t != T) || (id_t_t != 1 && id_t_t != T))
        return ET_ERR_INVALID_ARG;
    const Ident I{identity_s, identity_t, id_s_t, id_t_t};
    return run(*params, v, I, nullptr, nullptr, N, nullptr, 1, N * N, N, out, logit_s, logit_t, workspace, workspace_bytes,
               (hipStream_t)stream);
}

// ---- training (et_sgcn_train.inl)
extern "C" size_t et_sgcn_train_workspace_bytes(const et_sgcn_params *params, int64_t N, int64_t sum_n2, int n_scenes) {
    if (check_params(params) != ET_OK || N <= 0 || sum_n2 < 0 || n_scenes < 0) return 0;
    return (size_t)tlay_of(*params, N, sum_n2, n_scenes).total * 4;
}

extern "C" int et_sgcn_train_layout(const et_sgcn_params *params, int64_t N, int64_t sum_n2, int n_scenes, int64_t *offsets,
                                    int n_offsets) {
    const int rc = check_params(params);
    if (rc != ET_OK) return rc;
    if (N <= 0 || sum_n2 < 0 || n_scenes < 0 || !offsets || n_offsets != ET_SGCN_TRAIN_LAYOUT_FIELDS) return ET_ERR_INVALID_ARG;
    const TLay t = tlay_of(*params, N, sum_n2, n_scenes);
    const int64_t f[ET_SGCN_TRAIN_LAYOUT_FIELDS] = {t.L.v, t.L.rs_s, t.L.rs_t, t.xs, t.xs_stride, t.xt, t.xt_stride, t.L.at, t.L.f2,
                                                    t.L.f1, t.L.ts, t.keep, tail_keep_floats(*params), t.dat, t.df1, t.dts, t.df2,
                                                    t.rrec, t.gs, t.gt, t.dir_s, t.dir_t, t.dd_s, t.total};
    for (int i = 0; i < ET_SGCN_TRAIN_LAYOUT_FIELDS; ++i) offsets[i] = f[i];
    return ET_OK;
}

extern "C" int64_t et_sgcn_grad_floats(const et_sgcn_params *params) {
    if (check_params(params) != ET_OK) return 0;
    return glay_of(*params).total;
}

extern "C" int et_sgcn_train_forward_scenes(const et_sgcn_params *params, const float *C_obs, const float *nrm, int64_t N,
                                            const int32_t *scene_offsets, int n_scenes, int64_t sum_n2, int64_t max_scene_n,
                                            float *C_pred_refine, float *logit_s, float *logit_t, void *workspace,
                                            size_t workspace_bytes, et_stream_t stream) {
    const int rc = check_params(params);
    if (rc != ET_OK) return rc;
    if (sum_n2 < 0 || max_scene_n < 0) return ET_ERR_INVALID_ARG;
    const int early = scene_args_status(N, INT32_MAX, scene_offsets, n_scenes, ET_SGCN_MAX_N);
    if (early != kSceneArgsGo) return early;
    if (!C_obs || !nrm || !C_pred_refine) return ET_ERR_INVALID_ARG;
    if (!scene_offsets) {
        n_scenes = 1;
        sum_n2 = N * N;
        max_scene_n = N;
    }
    if (max_scene_n > ET_SGCN_MAX_N) max_scene_n = ET_SGCN_MAX_N;
    const Ident I{nullptr, nullptr, 1, 1};
    return run_train(*params, nullptr, I, C_obs, nrm, N, scene_offsets, n_scenes, sum_n2, max_scene_n, C_pred_refine, logit_s,
                     logit_t, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int et_sgcn_train_forward_graph(const et_sgcn_params *params, const float *v, const float *identity_s, int id_s_t,
                                           const float *identity_t, int id_t_t, int64_t N, float *out, float *logit_s,
                                           float *logit_t, void *workspace, size_t workspace_bytes, et_stream_t stream) {
    const int rc = check_params(params);
    if (rc != ET_OK) return rc;
    if (N < 0 || N > ET_SGCN_MAX_N) return ET_ERR_INVALID_ARG;
    if (N == 0) return ET_OK;
    const int T = params->obs_len;
    if (!v || !identity_s || !identity_t || !out || (id_s_t != 1 && id_s_t != T) || (id_t_t != 1 && id_t_t != T))
        return ET_ERR_INVALID_ARG;
    const Ident I{identity_s, identity_t, id_s_t, id_t_t};
    return run_train(*params, v, I, nullptr, nullptr, N, nullptr, 1, N * N, N, out, logit_s, logit_t, workspace,
                     workspace_bytes, (hipStream_t)stream);
}

extern "C" int et_sgcn_backward_scenes(const et_sgcn_params *params, int64_t N, const int32_t *scene_offsets, int n_scenes,
                                       int64_t sum_n2, int64_t max_scene_n, const float *d_out, float *grads,
                                       int64_t grads_floats, void *workspace, size_t workspace_bytes, et_stream_t stream) {
    const int rc = check_params(params);
    if (rc != ET_OK) return rc;
    if (sum_n2 < 0 || max_scene_n < 0 || !grads || grads_floats < glay_of(*params).total) return ET_ERR_INVALID_ARG;
    if (N < 0 || N > INT32_MAX || n_scenes < 0 || (scene_offsets && n_scenes == 0 && N != 0) ||
        (!scene_offsets && N > ET_SGCN_MAX_N) || (N > 0 && !d_out))
        return ET_ERR_INVALID_ARG;
    if (!scene_offsets) {
        n_scenes = 1;
        sum_n2 = N * N;
        max_scene_n = N;
    }
    if (max_scene_n > ET_SGCN_MAX_N) max_scene_n = ET_SGCN_MAX_N;
    if (N == 0) {  // no scene: every gradient is zero
        if (hipMemsetAsync(grads, 0, (size_t)glay_of(*params).total * 4, (hipStream_t)stream) != hipSuccess) return ET_ERR_HIP;
        return ET_OK;
    }
    const Ident I{nullptr, nullptr, 1, 1};
    return run_backward(*params, I, N, scene_offsets, n_scenes, sum_n2, max_scene_n, d_out, grads, workspace, workspace_bytes,
                        (hipStream_t)stream);
}

extern "C" int et_sgcn_backward_graph(const et_sgcn_params *params, const float *identity_s, int id_s_t,
                                      const float *identity_t, int id_t_t, int64_t N, const float *d_out, float *grads,
                                      int64_t grads_floats, void *workspace, size_t workspace_bytes, et_stream_t stream) {
    const int rc = check_params(params);
    if (rc != ET_OK) return rc;
    const int T = params->obs_len;
    if (N <= 0 || N > ET_SGCN_MAX_N || !identity_s || !identity_t || !d_out || !grads ||
        grads_floats < glay_of(*params).total || (id_s_t != 1 && id_s_t != T) || (id_t_t != 1 && id_t_t != T))
        return ET_ERR_INVALID_ARG;
    const Ident I{identity_s, identity_t, id_s_t, id_t_t};
    return run_backward(*params, I, N, nullptr, 1, N * N, N, d_out, grads, workspace, workspace_bytes, (hipStream_t)stream);
}
