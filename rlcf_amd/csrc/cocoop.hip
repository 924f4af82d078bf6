// The CoCoOp prompt generator (TPT/clip/cocoop.py:52-56,118-127): out[r] = ctx + meta_net(f_r), the meta-net's output broadcast over
// the n_ctx context rows, with meta_net = Linear(D, H) -> ReLU -> Linear(H, W).  One launch; a latency kernel (H * D + W * H
// multiply-adds per prompt), no throughput claim.
//   rows form: one prompt per feature row;  mean form: the n rows are averaged first (gen_ctx(aug=False), cocoop.py:179), one prompt.
// House rule of tpt.hip / kd.hip: every sum in double, rounded to float once at the store; fixed-order reductions (the wave's
// xor-shuffle tree, serial loops), no atomics: two calls give the same bits, and a row gives the same bits alone as inside a batch
// (a workgroup reads its own feature row and nothing else of the batch).
#include "common.h"
#include "kernels.h"

#define COCOOP_THREADS 256          // 4 waves; also the slice of W one workgroup writes
#define COCOOP_MAX_LDS_DOUBLES 8000 // D + H doubles of dynamic LDS (64 KB is the default limit)

// grid (ceil(W / COCOOP_THREADS), rows_out).  Every workgroup recomputes the hidden vector of its prompt into LDS (a wave per hidden
// unit, strided over the waves), then each thread owns one output column of the slice.
__global__ void __launch_bounds__(COCOOP_THREADS)
cocoop_ctx_kernel(const float* __restrict__ feats, int ld, int n, int mean, const float* __restrict__ ctx, int n_ctx,
                  const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                  int D, int H, int W, float* __restrict__ out) {
    extern __shared__ double lds[];
    double* f = lds;                 // [D] the feature row (or the mean row)
    double* h = lds + D;             // [H] relu(W1 f + b1)
    const int r = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int d = tid; d < D; d += COCOOP_THREADS) {
        double v;
        if (mean) {
            v = 0.0;
            for (int i = 0; i < n; ++i) v += (double)feats[(size_t)i * ld + d];      // rows in index order
            v /= (double)n;
        } else {
            v = (double)feats[(size_t)r * ld + d];
        }
        f[d] = v;
    }
    __syncthreads();
    for (int j = wave; j < H; j += COCOOP_THREADS / 64) {
        const float* wr = w1 + (size_t)j * D;
        double acc = 0.0;
        for (int d = lane; d < D; d += 64) acc += (double)wr[d] * f[d];
        acc = wave_sum(acc);
        if (lane == 0) { acc += (double)b1[j]; h[j] = acc > 0.0 ? acc : 0.0; }
    }
    __syncthreads();
    const int w = blockIdx.x * COCOOP_THREADS + tid;
    if (w >= W) return;
    const float* wr = w2 + (size_t)w * H;
    double bias = (double)b2[w];
    for (int j = 0; j < H; ++j) bias += (double)wr[j] * h[j];
    float* o = out + (size_t)r * n_ctx * W;
    for (int i = 0; i < n_ctx; ++i) o[(size_t)i * W + w] = (float)((double)ctx[(size_t)i * W + w] + bias);
}

int launch_cocoop_ctx(const float* feats, int ld, int n, int mean, const float* ctx, int n_ctx, const float* w1, const float* b1,
                      const float* w2, const float* b2, int D, int H, int W, float* out, hipStream_t st) {
    if (!feats || !ctx || !w1 || !b1 || !w2 || !b2 || !out) {
        rlcf_set_error("cocoop_ctx: null pointer (features, ctx, the four meta-net tensors and out are all required)");
        return RLCF_ERR_ARG;
    }
    if (H < 1 || n < 1 || n > 65535 || D < 1 || W < 1 || n_ctx < 1 || ld < D || D + H > COCOOP_MAX_LDS_DOUBLES) {
        rlcf_set_error("cocoop_ctx: n = %d feature rows of D = %d (row stride %d), H = %d hidden units, n_ctx = %d rows of W = %d "
                       "(need 1 <= n <= 65535, H >= 1, D >= 1, W >= 1, n_ctx >= 1, ld >= D, D + H <= %d)", n, D, ld, H, n_ctx, W,
                       COCOOP_MAX_LDS_DOUBLES);
        return RLCF_ERR_ARG;
    }
    const int rows_out = mean ? 1 : n;
    cocoop_ctx_kernel<<<dim3((W + COCOOP_THREADS - 1) / COCOOP_THREADS, rows_out), dim3(COCOOP_THREADS), (size_t)(D + H) * sizeof(double), st>>>(
        feats, ld, n, mean ? 1 : 0, ctx, n_ctx, w1, b1, w2, b2, D, H, W, out);
    RLCF_LAUNCH_CHECK();
    return RLCF_OK;
}
