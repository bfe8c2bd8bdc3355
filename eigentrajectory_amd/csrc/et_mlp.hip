// et_mlp.hip -- PECNet / LBEBM inference (baseline/pecnet, baseline/lbebm: the bridges' hooks and the two predict bodies;
// include/eigentraj.h "PECNet / LBEBM predictors").  Two kernels:
//
// mlp_chain_kernel   (et_mlp_chain.inl, shared with et_mlp_train.hip; here its MlLaunch form) a workgroup takes kMlRows = 16
//   rows through ALL layers of one chain of Linear + ReLU.  The activations
//   ping-pong between two LDS images of (16, kMlStride) floats; the weights W (out, in) are read in place from global memory
//   (L2: every workgroup reads the same tensors).  A wavefront owns 16-column blocks of a layer's output, two at a time (two
//   independent accumulators hide the MFMA's dependent latency), and forms them with v_mfma_f32_16x16x4_f32: A = the
//   activations (lane l: row l & 15, k = k0 + (l >> 4)), B = W^T (lane l: k = k0 + (l >> 4), column l & 15), D row
//   4 (l >> 4) + r, column l & 15.  The instruction is a k-ordered fp32 fmaf chain, the loop runs k0 ascending from a zero
//   accumulator and the bias is added last, so an output element's value depends on its input row and the layer's shape
//   only -- not on the row's place in the tile, the tile, or the number of rows.  Rows past N, the columns in .. up4(in) of
//   every image and the weights read for them are written / taken as zeros, and a block's columns past `out` are stored
//   as zeros, so nothing uninitialised is ever multiplied.  blockIdx.y picks one of up to three chains of the launch; the
//   first layer gathers its input from up to three sources side by side (element (row, c) at p[row rs + c cs]).
//   In the scene form the encoder_dest chain's workgroups form their rows' obs_ori themselves (the scene's mean in
//   scene_v's summation order), use it as their input and store it for the later launches and the caller.
// nonlocal_pool_kernel   (et_mlp_chain.inl as well; here its AtLaunch form) one wavefront per row: the row's logits against every phi row of its range (fp32 fmaf, ascending),
//   softmax over the whole range, times the mask, / max(sum |w|, 1e-12), times g, + feat.  The range is the row's scene
//   (or all N rows in the module form); a range longer than ET_MLP_MAX_RANGE is not computed: its rows are NaN.
#include "et_common.h"

namespace et {
namespace {

#include "et_scene_helpers.inl"  // scene_of_row, up4, kSnThreads

#include "et_mlp_chain.inl"  // the launch structures, both kernels, the parameter checks (shared with et_mlp_train.hip)

// the workspace, in floats: every block starts on a multiple of 4
struct MlWs {
    int64_t ftraj, dfeat, pos, theta, phi, g, feat[2], total;
};

static MlWs ml_workspace(const et_mlp_params &p, int64_t N) {
    MlWs w{};
    int64_t at = 0;
    auto take = [&](int64_t width) {
        const int64_t here = at;
        at += up4(N * width);
        return here;
    };
    const int F = feat_width(p);
    w.ftraj = take(p.fdim);
    w.dfeat = take(p.fdim);
    w.pos = take(2);
    if (p.nonlocal_pools > 0) {
        w.theta = take(p.non_local_dim);
        w.phi = take(p.non_local_dim);
        w.g = take(F);
        w.feat[0] = take(F);
        w.feat[1] = take(F);
    }
    w.total = at;
    return w;
}

static int lds_attributes() {
    static PerDevice<bool> lds_set;
    bool &ok = lds_set.current();
    if (ok) return ET_OK;
    ET_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(mlp_chain_kernel<MlLaunch>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, kMlLdsBytes));
    ET_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(nonlocal_pool_kernel<AtLaunch>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, kAtLdsBytes));
    ok = true;
    return ET_OK;
}

// Both predictors, both forms.  Module form: past / dest / pos given (nrm null).  Scene form: C_obs, nrm (past, dest, pos
// null); out is then C_pred_refine.  1 + 2 nonlocal_pools + 1 launches.
static int ml_run(const et_mlp_params &p, const float *past, const float *dest, const float *pos, const float *mask,
                  const float *C_obs, const float *nrm, const int32_t *off, int n_scenes, int64_t N, float *out,
                  float *gin, void *workspace, size_t workspace_bytes, hipStream_t stream) {
    const MlWs W = ml_workspace(p, N);
    if (!workspace || workspace_bytes < (size_t)W.total * 4) return ET_ERR_WORKSPACE;
    const int rc = lds_attributes();
    if (rc != ET_OK) return rc;
    float *ws = (float *)workspace;
    const int F = feat_width(p), kp = p.encoder_past.widths[0], kd = p.encoder_dest.widths[0];
    const unsigned tiles = (unsigned)((N + kMlRows - 1) / kMlRows);
    const bool scenes = nrm != nullptr;

    MlLaunch L{};
    L.N = N;
    job_of(L.job[0], p.encoder_past, ws + W.ftraj, p.fdim);
    job_of(L.job[1], p.encoder_dest, ws + W.dfeat, p.fdim);
    L.job[0].n_src = L.job[1].n_src = 1;
    if (scenes) {
        L.job[0].src[0] = MlSrc{C_obs, kp, 1, N};  // past = C_obs^T
        L.sc = MlScene{C_obs, nrm, off, n_scenes, kp, ws + W.pos, gin};
        pos = ws + W.pos;
    } else {
        L.job[0].src[0] = rows_of(past, kp);
        L.job[1].src[0] = rows_of(dest, kd);
    }
    hipLaunchKernelGGL(mlp_chain_kernel<MlLaunch>, dim3(tiles, 2), dim3(kMlThreads), kMlLdsBytes, stream, L);
    ET_LAUNCH_CHECK();

    MlSrc feat[3] = {rows_of(ws + W.ftraj, p.fdim), rows_of(ws + W.dfeat, p.fdim), rows_of(pos, p.pos_width)};
    int n_feat = p.pos_width ? 3 : 2;
    for (int r = 0; r < p.nonlocal_pools; ++r) {
        MlLaunch Q{};
        Q.N = N;
        job_of(Q.job[0], p.non_local_theta, ws + W.theta, p.non_local_dim);
        job_of(Q.job[1], p.non_local_phi, ws + W.phi, p.non_local_dim);
        job_of(Q.job[2], p.non_local_g, ws + W.g, F);
        for (int j = 0; j < 3; ++j) {
            Q.job[j].n_src = n_feat;
            for (int s = 0; s < n_feat; ++s) Q.job[j].src[s] = feat[s];
        }
        hipLaunchKernelGGL(mlp_chain_kernel<MlLaunch>, dim3(tiles, 3), dim3(kMlThreads), kMlLdsBytes, stream, Q);
        ET_LAUNCH_CHECK();
        AtLaunch A{};
        A.theta = ws + W.theta, A.phi = ws + W.phi, A.g = ws + W.g;
        A.D = p.non_local_dim, A.F = F, A.n_src = n_feat;
        for (int s = 0; s < n_feat; ++s) A.src[s] = feat[s];
        A.mask = mask, A.off = off, A.n_scenes = n_scenes, A.N = N;
        A.out = ws + W.feat[r & 1];
        hipLaunchKernelGGL(nonlocal_pool_kernel<AtLaunch>, dim3((unsigned)((N + kAtRows - 1) / kAtRows)), dim3(kMlThreads),
                           kAtLdsBytes, stream, A);
        ET_LAUNCH_CHECK();
        feat[0] = rows_of(A.out, F);
        n_feat = 1;
    }

    MlLaunch P{};
    P.N = N;
    job_of(P.job[0], p.predictor, out, scenes ? p.out_width / kp : p.out_width);
    P.job[0].n_src = n_feat;
    for (int s = 0; s < n_feat; ++s) P.job[0].src[s] = feat[s];
    hipLaunchKernelGGL(mlp_chain_kernel<MlLaunch>, dim3(tiles, 1), dim3(kMlThreads), kMlLdsBytes, stream, P);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

static size_t ml_workspace_bytes(const et_mlp_params *p, bool pecnet, int64_t N) {
    if (ml_check_params(p, pecnet) != ET_OK || N < 0) return 0;
    return (size_t)ml_workspace(*p, N).total * 4;
}

static int ml_predict(const et_mlp_params *p, bool pecnet, const float *past, const float *dest, const float *mask,
                      const float *pos, int64_t N, float *out, void *workspace, size_t workspace_bytes, et_stream_t stream) {
    const int rc = ml_check_params(p, pecnet);
    if (rc != ET_OK) return rc;
    if (N < 0 || N > INT32_MAX) return ET_ERR_INVALID_ARG;
    if (p->nonlocal_pools > 0 && N > ET_MLP_MAX_RANGE) return ET_ERR_UNSUPPORTED;
    if (N == 0) return ET_OK;
    if (!past || !dest || !out || (pecnet && !pos)) return ET_ERR_INVALID_ARG;
    return ml_run(*p, past, dest, pos, mask, nullptr, nullptr, nullptr, 0, N, out, nullptr, workspace, workspace_bytes,
                  (hipStream_t)stream);
}

static int ml_scenes(const et_mlp_params *p, bool pecnet, const float *C_obs, const float *nrm, int64_t N,
                     const int32_t *off, int n_scenes, float *out, float *gin, void *workspace, size_t workspace_bytes,
                     et_stream_t stream) {
    const int rc = ml_check_params(p, pecnet);
    if (rc != ET_OK) return rc;
    if (p->encoder_dest.widths[0] != 2 || p->out_width % p->encoder_past.widths[0] != 0) return ET_ERR_UNSUPPORTED;
    const int early = scene_args_status(N, INT32_MAX, off, n_scenes, ET_SCENE_MAX_N);
    if (early != kSceneArgsGo) return early;
    if (!C_obs || !nrm || !out) return ET_ERR_INVALID_ARG;
    return ml_run(*p, nullptr, nullptr, nullptr, nullptr, C_obs, nrm, off, n_scenes, N, out, gin, workspace,
                  workspace_bytes, (hipStream_t)stream);
}

}  // namespace
}  // namespace et

using namespace et;

extern "C" size_t et_pecnet_workspace_bytes(const et_mlp_params *params, int64_t N) {
    return ml_workspace_bytes(params, true, N);
}

extern "C" int et_pecnet_predict(const et_mlp_params *params, const float *past, const float *dest, const float *mask,
                                 const float *initial_pos, int64_t N, float *out, void *workspace, size_t workspace_bytes,
                                 et_stream_t stream) {
    return ml_predict(params, true, past, dest, mask, initial_pos, N, out, workspace, workspace_bytes, stream);
}

extern "C" int et_pecnet_forward_scenes(const et_mlp_params *params, const float *C_obs, const float *nrm, int64_t N,
                                        const int32_t *scene_offsets, int n_scenes, float *C_pred_refine, float *net_inputs,
                                        void *workspace, size_t workspace_bytes, et_stream_t stream) {
    return ml_scenes(params, true, C_obs, nrm, N, scene_offsets, n_scenes, C_pred_refine, net_inputs, workspace,
                     workspace_bytes, stream);
}

extern "C" size_t et_lbebm_workspace_bytes(const et_mlp_params *params, int64_t N) {
    return ml_workspace_bytes(params, false, N);
}

extern "C" int et_lbebm_predict(const et_mlp_params *params, const float *past, const float *dest, int64_t N, float *out,
                                void *workspace, size_t workspace_bytes, et_stream_t stream) {
    return ml_predict(params, false, past, dest, nullptr, nullptr, N, out, workspace, workspace_bytes, stream);
}

extern "C" int et_lbebm_forward_scenes(const et_mlp_params *params, const float *C_obs, const float *nrm, int64_t N,
                                       const int32_t *scene_offsets, int n_scenes, float *C_pred_refine, float *net_inputs,
                                       void *workspace, size_t workspace_bytes, et_stream_t stream) {
    return ml_scenes(params, false, C_obs, nrm, N, scene_offsets, n_scenes, C_pred_refine, net_inputs, workspace,
                     workspace_bytes, stream);
}
