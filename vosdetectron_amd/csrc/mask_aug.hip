// Mask test-time augmentation: the combination of the per-view soft masks.
//
// Reference: im_detect_mask_aug, lib/core/test.py:405-476.  masks_ts holds one
// [M, R, R] class-selected sigmoid output per view, a flipped view's already
// inverted (masks_hf[:, :, :, ::-1], :491); TEST.MASK_AUG.HEUR combines them:
//   SOFT_AVG   np.mean(masks_ts, axis=0)  = the float32 sum in view order / float32(T)
//   SOFT_MAX   np.amax(masks_ts, axis=0)  = the running maximum
//   LOGIT_AVG  1 / (1 + exp(-mean(logit(y)))), logit(y) = -1 * log((1 - y) / max(y, 1e-20)),
//              all in float32
// vd_mask_aug_accumulate folds one view into acc (reading a flipped view with
// its last axis reversed), vd_mask_aug_finish turns the sums into the result.
#include "vosdet_internal.hpp"

namespace vd {

__global__ __launch_bounds__(256) void mask_aug_accumulate_kernel(float *__restrict__ acc,
                                                                  const float *__restrict__ masks,
                                                                  int64_t n, int R, int hflip,
                                                                  int heur, int first) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % R);
    const float y = masks[hflip ? i - x + (R - 1 - x) : i];
    float v = y;
    if (heur == VD_MASK_AUG_LOGIT_AVG) v = -1.0f * logf((1.0f - y) / fmaxf(y, 1e-20f));
    if (!first) {
        const float a = acc[i];
        v = heur == VD_MASK_AUG_SOFT_MAX ? fmaxf(a, v) : a + v;
    }
    acc[i] = v;
}

__global__ __launch_bounds__(256) void mask_aug_finish_kernel(float *__restrict__ acc, int64_t n,
                                                              float T, int heur) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float m = acc[i] / T;
    acc[i] = heur == VD_MASK_AUG_LOGIT_AVG ? 1.0f / (1.0f + expf(-m)) : m;
}

int launch_mask_aug_accumulate(float *acc, const float *masks, int M, int R, int hflip, int heur,
                               int first, hipStream_t s) {
    if (M < 0 || R < 1 || heur < VD_MASK_AUG_SOFT_AVG || heur > VD_MASK_AUG_LOGIT_AVG)
        return VD_ERR_ARG;
    if (M == 0) return VD_OK;
    const int64_t n = (int64_t)M * R * R;
    hipLaunchKernelGGL(mask_aug_accumulate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       s, acc, masks, n, R, hflip ? 1 : 0, heur, first ? 1 : 0);
    return hipGetLastError() == hipSuccess ? VD_OK : VD_ERR_LAUNCH;
}

int launch_mask_aug_finish(float *acc, int M, int R, int T, int heur, hipStream_t s) {
    if (M < 0 || R < 1 || T < 1 || heur < VD_MASK_AUG_SOFT_AVG || heur > VD_MASK_AUG_LOGIT_AVG)
        return VD_ERR_ARG;
    if (M == 0 || heur == VD_MASK_AUG_SOFT_MAX) return VD_OK;
    const int64_t n = (int64_t)M * R * R;
    hipLaunchKernelGGL(mask_aug_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                       acc, n, (float)T, heur);
    return hipGetLastError() == hipSuccess ? VD_OK : VD_ERR_LAUNCH;
}

}  // namespace vd
