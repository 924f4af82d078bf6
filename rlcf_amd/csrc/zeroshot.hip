// Ensemble cosine logits of the zero-shot classifiers (TPT/clip/custom_clip.py:555-566, CLIPCLS_TTA_Multiple.forward; with one model
// :423-432, CLIPCLS_TTA.forward):
//   logits[b, c] = (1 / M) * sum_{m < M} s_m * <img_m[b, :D_m], txt_m[c, :D_m]>,   s_m = exp(logit_scale_m), M = 1 .. 5
// Every model has its own width D_m and row strides; the rows arrive L2-normalised.  One launch covers all models; a latency kernel
// (the hot path of a zero-shot batch is the image towers), no throughput claim.
// The grid is tiled over (class tile, row tile) = (ZS_TC, ZS_TR) outputs; a workgroup stages both operand tiles of a model through LDS
// in chunks of ZS_DK elements of D with 16-byte global loads, so a text row is read from global memory once per ROW TILE
// (ceil(n / ZS_TR) times), not once per image row as group_logits_kernel reads it.
// House rule of kd.hip / tpt.hip / cocoop.hip: the dot products, the scale, the sum over the models (in model order) and the 1 / M in
// double, rounded to float once at the store.  One thread owns an output and walks D serially in index order: no atomics, no MFMA, no
// cross-lane reduction; two calls give the same bits, and a row gives the same bits alone as inside a batch (its sums never see n).
#include "common.h"
#include "kernels.h"

#define ZS_THREADS 256      // 4 waves: lane = class of the tile, wave = 4 consecutive rows of the tile
#define ZS_TR 16            // rows per tile
#define ZS_TC 64            // classes per tile
#define ZS_DK 64            // elements of D per LDS chunk
#define ZS_LD (ZS_DK + 4)   // LDS row stride in floats: 17 16-byte slots, so the 64 lanes' ds_read_b128 of one column fall on distinct slots mod 16

__global__ void __launch_bounds__(ZS_THREADS)
ensemble_logits_kernel(const rlcf_ens_desc desc, int n, int C, float* __restrict__ logits, int ld_logits) {
    __shared__ __attribute__((aligned(16))) float s_img[ZS_TR * ZS_LD];
    __shared__ __attribute__((aligned(16))) float s_txt[ZS_TC * ZS_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = blockIdx.x * ZS_TC, b0 = blockIdx.y * ZS_TR;
    const int sr = tid >> 4, sq = (tid & 15) * 4;          // staging: row sr (+ 16 k) of a tile, floats sq .. sq + 3 of the chunk
    double total[4] = {0.0, 0.0, 0.0, 0.0};
    for (int m = 0; m < desc.M; ++m) {
        const float* __restrict__ img = desc.m[m].img;
        const float* __restrict__ txt = desc.m[m].txt;
        const int ld_img = desc.m[m].ld_img, ld_txt = desc.m[m].ld_txt, D = desc.m[m].D;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int d0 = 0; d0 < D; d0 += ZS_DK) {
            const bool d_in = d0 + sq < D;                 // D % 4 == 0: a 16-byte group lies inside the row or outside it
            {
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (d_in && b0 + sr < n) v = *(const f32x4*)(img + (size_t)(b0 + sr) * ld_img + d0 + sq);
                *(f32x4*)(s_img + sr * ZS_LD + sq) = v;
            }
#pragma unroll
            for (int k = 0; k < ZS_TC / 16; ++k) {
                const int r = sr + 16 * k;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (d_in && c0 + r < C) v = *(const f32x4*)(txt + (size_t)(c0 + r) * ld_txt + d0 + sq);
                *(f32x4*)(s_txt + r * ZS_LD + sq) = v;
            }
            __syncthreads();
            // (rows, classes and elements past the end were staged as zeros: they add exact zeros, in the same places for every n)
#pragma unroll 4
            for (int d = 0; d < ZS_DK; d += 4) {
                const f32x4 t = *(const f32x4*)(s_txt + lane * ZS_LD + d);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f32x4 a = *(const f32x4*)(s_img + (wave * 4 + i) * ZS_LD + d);      // one address per wave: a broadcast
                    acc[i] += (double)a.x * (double)t.x;
                    acc[i] += (double)a.y * (double)t.y;
                    acc[i] += (double)a.z * (double)t.z;
                    acc[i] += (double)a.w * (double)t.w;
                }
            }
            __syncthreads();
        }
        const double s = (double)desc.m[m].scale;
#pragma unroll
        for (int i = 0; i < 4; ++i) total[i] += s * acc[i];
    }
    const int c = c0 + lane;
    if (c >= C) return;
    const double Md = (double)desc.M;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = b0 + wave * 4 + i;
        if (b < n) logits[(size_t)b * ld_logits + c] = (float)(total[i] / Md);
    }
}

int launch_ensemble_logits(const rlcf_ens_desc* desc, int n, int C, float* logits, int ld_logits, hipStream_t st) {
    if (!desc || !logits) { rlcf_set_error("ensemble_logits: null pointer (the descriptor and logits are required)"); return RLCF_ERR_ARG; }
    if (desc->M < 1 || desc->M > RLCF_ENS_MAX_MODELS || n < 1 || C < 1 || ld_logits < C) {
        rlcf_set_error("ensemble_logits: M = %d models, n = %d rows, C = %d classes, ld_logits = %d (need 1 <= M <= %d, n >= 1, C >= 1, "
                       "ld_logits >= C)", desc->M, n, C, ld_logits, RLCF_ENS_MAX_MODELS);
        return RLCF_ERR_ARG;
    }
    for (int m = 0; m < desc->M; ++m) {
        const rlcf_ens_model& d = desc->m[m];
        if (!d.img || !d.txt || ((uintptr_t)d.img & 15) || ((uintptr_t)d.txt & 15)) {
            rlcf_set_error("ensemble_logits: model %d: img / txt must be non-NULL and 16-byte aligned (the rows are read by 16-byte loads)", m);
            return RLCF_ERR_ARG;
        }
        if (d.D < 4 || d.D % 4 || d.ld_img < d.D || d.ld_img % 4 || d.ld_txt < d.D || d.ld_txt % 4) {
            rlcf_set_error("ensemble_logits: model %d: D = %d, ld_img = %d, ld_txt = %d (need D >= 4, D %% 4 == 0, both strides >= D and "
                           "multiples of 4)", m, d.D, d.ld_img, d.ld_txt);
            return RLCF_ERR_ARG;
        }
    }
    const int row_tiles = (n + ZS_TR - 1) / ZS_TR;
    if (row_tiles > 65535) {           // grid.y (launch_group_logits holds its grid.y to the same limit)
        rlcf_set_error("ensemble_logits: n = %d rows make %d row tiles (at most 65535)", n, row_tiles);
        return RLCF_ERR_ARG;
    }
    ensemble_logits_kernel<<<dim3((C + ZS_TC - 1) / ZS_TC, row_tiles), dim3(ZS_THREADS), 0, st>>>(*desc, n, C, logits, ld_logits);
    RLCF_LAUNCH_CHECK();
    return RLCF_OK;
}
