// The loss of the TPT baseline (TPT/tpt_cls.py:40-46,66, TPT/tune_cls_tpt.py:49): avg_entropy of the selected views' logits rows and
// its dense gradient, stand-alone (no reward model, no sampled classes).  `groups` independent test samples of n consecutive rows:
//   p_ic = softmax(x_i)_c,  a_c = log((1/n) sum_i p_ic)  (clamped below at float32's finfo.min, as the reference clamps it),
//   L = -sum_c a_c e^{a_c},  dL/dx_id = (p_id / n) * (sum_c p_ic a_c - a_d)
// (the form reward_stage_b_kernel uses for its RLCF_F_MIN_ENTROPY regulariser, tta.hip).  Everything is evaluated in double, as kd.hip
// evaluates the distillation losses, and rounded to float once; every reduction is a fixed-order wave-shuffle + LDS tree or a serial
// sum, no atomics: two calls give the same bits, and a group computes the same bits alone as inside a grouped call.
// Three launches, a_c parked in the caller's workspace (no LDS table: C up to RLCF_KD_MAX_CLASSES):
//   rows     one workgroup per row: the row's log-sum-exp                                        -> ws lse[groups * n]
//   classes  grid (chunks of TPT_THREADS classes, groups): a_c over the group's n rows, and the
//            chunk's partial of sum_c a_c e^{a_c}                                                -> ws a[groups * C], part[groups * chunks]
//   grad     one workgroup per row: sum_c p_ic a_c, the row of dlogits; the first row of a group
//            adds the group's partials in chunk order                                            -> dlogits, loss[groups]
// A NaN or an infinity in a row reaches the loss and every gradient of its group (x - lse is NaN), so the GradScaler step skip fires.
#include "kernels.h"

#define TPT_THREADS 256
#define TPT_MIN_REAL (-3.4028234663852886e38)      // torch.finfo(torch.float32).min

static int tpt_chunks(int C) { return (C + TPT_THREADS - 1) / TPT_THREADS; }
size_t tpt_ws_bytes(int groups, int n, int C) {
    return ((size_t)groups * n + (size_t)groups * C + (size_t)groups * tpt_chunks(C)) * sizeof(double);
}

__global__ __launch_bounds__(TPT_THREADS) void tpt_rows_kernel(const float* __restrict__ logits, int ld, int C, double* __restrict__ lse) {
    __shared__ double red[TPT_THREADS / 64];
    const float* x = logits + (size_t)blockIdx.x * ld;
    double mx = -INFINITY;
    for (int c = threadIdx.x; c < C; c += TPT_THREADS) mx = fmax(mx, (double)x[c]);
    mx = block_max<TPT_THREADS>(mx, red);
    double s = 0.0;
    for (int c = threadIdx.x; c < C; c += TPT_THREADS) s += exp((double)x[c] - mx);       // (a NaN the max skipped lands here)
    s = block_sum<TPT_THREADS>(s, red);
    if (threadIdx.x == 0) lse[blockIdx.x] = mx + log(s);
}

__global__ __launch_bounds__(TPT_THREADS) void tpt_classes_kernel(const float* __restrict__ logits, int ld, int n, int C,
                                                                  const double* __restrict__ lse, double* __restrict__ a_out,
                                                                  double* __restrict__ part) {
    __shared__ double red[TPT_THREADS / 64];
    const int g = blockIdx.y, c = blockIdx.x * TPT_THREADS + threadIdx.x;
    const float* x = logits + (size_t)g * n * ld;
    const double* l = lse + (size_t)g * n;
    double h = 0.0;
    if (c < C) {
        double mx = -INFINITY;
        for (int i = 0; i < n; ++i) mx = fmax(mx, (double)x[(size_t)i * ld + c] - l[i]);
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += exp((double)x[(size_t)i * ld + c] - l[i] - mx);
        double a = mx + log(s) - log((double)n);          // (the device's log on both sides: one class gives exactly 0)
        a = a < TPT_MIN_REAL ? TPT_MIN_REAL : a;          // torch.clamp(min=finfo.min): a NaN stays a NaN
        a_out[(size_t)g * C + c] = a;
        h = a * exp(a);
    }
    h = block_sum<TPT_THREADS>(h, red);
    if (threadIdx.x == 0) part[(size_t)g * gridDim.x + blockIdx.x] = h;
}

__global__ __launch_bounds__(TPT_THREADS) void tpt_grad_kernel(const float* __restrict__ logits, int ld, int n, int C, int chunks,
                                                               const double* __restrict__ lse, const double* __restrict__ a_all,
                                                               const double* __restrict__ part, float* __restrict__ loss,
                                                               float* __restrict__ dlogits) {
    __shared__ double red[TPT_THREADS / 64];
    const int i = blockIdx.x, g = i / n;
    const float* x = logits + (size_t)i * ld;
    const double* a = a_all + (size_t)g * C;
    const double l = lse[i];
    if (loss && i == g * n && threadIdx.x == 0) {
        double h = 0.0;
        for (int k = 0; k < chunks; ++k) h += part[(size_t)g * chunks + k];
        loss[g] = (float)(-h);
    }
    if (!dlogits) return;
    double dot = 0.0;
    for (int c = threadIdx.x; c < C; c += TPT_THREADS) dot += exp((double)x[c] - l) * a[c];
    dot = block_sum<TPT_THREADS>(dot, red);
    const double inv_n = 1.0 / n;
    float* d = dlogits + (size_t)i * C;
    for (int c = threadIdx.x; c < C; c += TPT_THREADS) d[c] = (float)(exp((double)x[c] - l) * inv_n * (dot - a[c]));
}

int launch_tpt_loss(const float* logits, int ld, int groups, int n, int C, float* loss, float* dlogits, double* ws, hipStream_t st) {
    RLCF_ARG_CHECK(logits && ws && (loss || dlogits));
    if (groups <= 0 || groups > 65535 || n <= 0 || C <= 0 || C > RLCF_KD_MAX_CLASSES || ld < C || (int64_t)groups * n > 0x7fffffff) {
        rlcf_set_error("tpt_loss: %d groups of n = %d rows of C = %d classes, row stride %d (need 1 <= groups <= 65535, n >= 1, 1 <= C <= %d, ld >= C)",
                       groups, n, C, ld, RLCF_KD_MAX_CLASSES);
        return RLCF_ERR_ARG;
    }
    const int rows = groups * n, chunks = tpt_chunks(C);
    double *lse = ws, *a = ws + rows, *part = a + (size_t)groups * C;
    tpt_rows_kernel<<<dim3(rows), dim3(TPT_THREADS), 0, st>>>(logits, ld, C, lse);
    RLCF_LAUNCH_CHECK();
    tpt_classes_kernel<<<dim3(chunks, groups), dim3(TPT_THREADS), 0, st>>>(logits, ld, n, C, lse, a, part);
    RLCF_LAUNCH_CHECK();
    tpt_grad_kernel<<<dim3(rows), dim3(TPT_THREADS), 0, st>>>(logits, ld, n, C, chunks, lse, a, part, loss, dlogits);
    RLCF_LAUNCH_CHECK();
    return RLCF_OK;
}
