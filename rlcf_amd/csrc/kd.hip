// Distillation losses of the KD ablation (TPT/tune_cls_kd.py:34-61): the student's logits rows against the reward model's
// (teacher) logits rows, the loss and its dense gradient d loss / d student.  Three losses, called as tune_cls_kd.py calls them:
//   KD   kd_distill_loss_v2 (TPT/utils/KD.py:19-29)    row = -T_s^2 * sum_c pt_c * log_softmax(s / T_s)_c,  pt = softmax(t / T_t)
//   DKD  dkd_distill_loss   (TPT/utils/DKD.py:13-37)   row = T^2 * (alpha * TCKD + beta * NCKD), target g = teacher argmax
//   ATKD atkd_distill_loss  (TPT/utils/ATKD.py:12-42)  version 1, see the note on its statistics below
// loss = mean over rows.  One workgroup per row, every reduction a fixed-order wave-shuffle + LDS tree, the row mean a serial
// sum: two calls give bit-identical results (no atomics).  The row arithmetic runs in double (n_sel x C = 6 x 1000 elements
// on the tuning path: the cost is nil), so the float results are the float64 values rounded once.
//
// Gradients (derived by hand, z = the row as the loss normalises it, ps = softmax(z_s), pt = the teacher's distribution;
// sum(pt) is kept literal, as the autograd of log_softmax keeps it):
//   KD:   d/ds_c = T_s^2 * (1/T_s) * (ps_c * sum(pt) - pt_c) / n = T_s * (ps_c * sum(pt) - pt_c) / n
//   ATKD: z_s = (s - a) * k with k = multiplier / (b + eps) and the statistics a, b held constant (no_grad), row scaled by b^2:
//         d/ds_c = b^2 * k * (ps_c * sum(pt) - pt_c) / n
//   DKD:  TCKD = KL([pt_g, pt_o] || [ps_g, ps_o]) with ps_o = sum_{c != g} ps_c (summed, not 1 - ps_g, as cat_mask sums it):
//           dTCKD/dz_g = ps_g * (pt_g + pt_o) - pt_g
//           dTCKD/dz_c = ps_c * (pt_g + pt_o) - pt_o * qs_c           (c != g; ps_c / ps_o = qs_c, the NCKD softmax below)
//         NCKD = KL(qt || qs), q = softmax over the classes c != g: the reference pushes the target logit down by 1000, whose
//         exp underflows to exactly 0 for CLIP-range logits, so the target class is excluded here outright:
//           dNCKD/dz_c = qs_c * sum(qt) - qt_c  (c != g),  0 at c = g
//         d/ds_c = T * (alpha * dTCKD/dz_c + beta * dNCKD/dz_c) / n
//         torch.log of the merged pair is -inf when ps_g or ps_o is 0 in float32 (the reference's precision): that row then
//         gets loss +inf and NaN gradients, as the reference's autograd gives them, and the GradScaler step skip follows.
#include "kernels.h"

#define KD_THREADS 256

// torch.argmax: first maximum, NaN ranks highest
__device__ __forceinline__ bool kd_better(float a, int ia, float b, int ib) {
    if (a != a) return b == b || ia < ib;
    if (b != b) return false;
    return a > b || (a == b && ia < ib);
}
__device__ int kd_block_argmax(const float* x, int C, float* redv, int* redi) {
    float v = -INFINITY;
    int i = C;
    for (int c = threadIdx.x; c < C; c += KD_THREADS)
        if (kd_better(x[c], c, v, i)) { v = x[c]; i = c; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(i, o);
        if (kd_better(ov, oi, v, i)) { v = ov; i = oi; }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { redv[threadIdx.x >> 6] = v; redi[threadIdx.x >> 6] = i; }
    __syncthreads();
    v = redv[0]; i = redi[0];
    for (int w = 1; w < KD_THREADS / 64; ++w)
        if (kd_better(redv[w], redi[w], v, i)) { v = redv[w]; i = redi[w]; }
    return i;
}
// population mean and standard deviation of a row (torch.std_mean(unbiased=False)), two passes
__device__ void kd_row_stats(const float* x, int C, double* red, double& mean, double& std) {
    double s = 0.0;
    for (int c = threadIdx.x; c < C; c += KD_THREADS) s += (double)x[c];
    mean = block_sum<KD_THREADS>(s, red) / C;
    double q = 0.0;
    for (int c = threadIdx.x; c < C; c += KD_THREADS) { const double d = (double)x[c] - mean; q += d * d; }
    std = sqrt(block_sum<KD_THREADS>(q, red) / C);
}
// p * (log p - lq) with torch.kl_div's convention 0 * log 0 = 0
__device__ __forceinline__ double kd_kl_term(double p, double lp, double lq) { return p > 0.0 ? p * (lp - lq) : 0.0; }

__global__ __launch_bounds__(KD_THREADS) void kd_rows_kernel(const float* __restrict__ stu, int ld_s, const float* __restrict__ tea, int ld_t,
                                                             int C, int mode, const int32_t* __restrict__ target, rlcf_kd_params p, double inv_n,
                                                             double* __restrict__ row_acc, float* __restrict__ row_loss, float* __restrict__ dlogits) {
    __shared__ double red[KD_THREADS / 64];
    __shared__ float redv[KD_THREADS / 64];
    __shared__ int redi[KD_THREADS / 64];
    const int i = blockIdx.x;
    const float* x = stu + (size_t)i * ld_s;
    const float* y = tea + (size_t)i * ld_t;
    float* d = dlogits ? dlogits + (size_t)i * C : nullptr;
    // z = (v - shift) * scale for both rows
    double ks = 1.0, kt = 1.0, as = 0.0, at = 0.0, out_scale = 1.0, grad_scale = 1.0;
    if (mode == RLCF_KD_KD) {
        ks = 1.0 / (double)p.T_stu; kt = 1.0 / (double)p.T_tea;
        out_scale = (double)p.T_stu * (double)p.T_stu;
        grad_scale = out_scale * ks;
    } else if (mode == RLCF_KD_DKD) {
        ks = kt = 1.0 / (double)p.temperature;
        out_scale = (double)p.temperature * (double)p.temperature;
        grad_scale = out_scale * ks;
    } else {
        // ATKD version 1.  utils/ATKD.py:21-22 unpack torch.std_mean (which returns (std, mean)) as `s_mu, s_std`: the row is
        // normalised as (z - std(z)) / (mean(z) + eps) * multiplier and the KL is scaled by mean(z)^2.  Reproduced literally.
        double ms, ss, mt, sd;
        kd_row_stats(x, C, red, ms, ss);
        kd_row_stats(y, C, red, mt, sd);
        as = ss; ks = (double)p.multiplier / (ms + (double)p.eps);
        at = sd; kt = (double)p.multiplier / (mt + (double)p.eps);
        out_scale = ms * ms;
        grad_scale = out_scale * ks;
    }
    int g = -1;
    if (mode == RLCF_KD_DKD) {
        g = target ? target[i] : kd_block_argmax(y, C, redv, redi);
        if (g < 0 || g >= C) {                               // out-of-range target: NaN row (nothing is read outside the row)
            if (threadIdx.x == 0) { row_acc[i] = NAN; if (row_loss) row_loss[i] = NAN; }
            if (d) for (int c = threadIdx.x; c < C; c += KD_THREADS) d[c] = NAN;
            return;
        }
    }
    // maxima (DKD: also over the non-target classes, the shift of the NCKD softmaxes)
    double mxs = -INFINITY, mxt = -INFINITY, mxs_n = -INFINITY, mxt_n = -INFINITY;
    for (int c = threadIdx.x; c < C; c += KD_THREADS) {
        const double zs = ((double)x[c] - as) * ks, zt = ((double)y[c] - at) * kt;
        mxs = fmax(mxs, zs); mxt = fmax(mxt, zt);
        if (c != g) { mxs_n = fmax(mxs_n, zs); mxt_n = fmax(mxt_n, zt); }
    }
    mxs = block_max<KD_THREADS>(mxs, red); mxt = block_max<KD_THREADS>(mxt, red);
    if (mode == RLCF_KD_DKD) { mxs_n = block_max<KD_THREADS>(mxs_n, red); mxt_n = block_max<KD_THREADS>(mxt_n, red); }
    double ss = 0.0, st = 0.0, ss_n = 0.0, st_n = 0.0;
    for (int c = threadIdx.x; c < C; c += KD_THREADS) {
        const double zs = ((double)x[c] - as) * ks, zt = ((double)y[c] - at) * kt;
        ss += exp(zs - mxs); st += exp(zt - mxt);
        if (mode == RLCF_KD_DKD && c != g) { ss_n += exp(zs - mxs_n); st_n += exp(zt - mxt_n); }
    }
    ss = block_sum<KD_THREADS>(ss, red); st = block_sum<KD_THREADS>(st, red);
    const double lss = log(ss), lst = log(st);
    if (mode == RLCF_KD_DKD) { ss_n = block_sum<KD_THREADS>(ss_n, red); st_n = block_sum<KD_THREADS>(st_n, red); }
    const double lss_n = log(ss_n), lst_n = log(st_n);
    if (mode != RLCF_KD_DKD) {
        // KD: -sum pt * log ps;  ATKD: sum pt * (log pt - log ps)
        double l = 0.0, spt = 0.0;
        for (int c = threadIdx.x; c < C; c += KD_THREADS) {
            const double zs = ((double)x[c] - as) * ks, zt = ((double)y[c] - at) * kt;
            const double lps = zs - mxs - lss, lpt = zt - mxt - lst, pt = exp(lpt);
            l += mode == RLCF_KD_KD ? -pt * lps : kd_kl_term(pt, lpt, lps);
            spt += pt;
        }
        l = block_sum<KD_THREADS>(l, red) * out_scale;
        spt = block_sum<KD_THREADS>(spt, red);
        if (threadIdx.x == 0) { row_acc[i] = l; if (row_loss) row_loss[i] = (float)l; }
        if (d) {
            const double gs = grad_scale * inv_n;
            for (int c = threadIdx.x; c < C; c += KD_THREADS) {
                const double zs = ((double)x[c] - as) * ks, zt = ((double)y[c] - at) * kt;
                d[c] = (float)(gs * (exp(zs - mxs - lss) * spt - exp(zt - mxt - lst)));
            }
        }
        return;
    }
    // DKD: the merged pair [p_g, p_other] of both rows; p_other summed over the non-target probabilities (cat_mask)
    double ps_o = 0.0, pt_o = 0.0, nckd = 0.0, sqt = 0.0;
    for (int c = threadIdx.x; c < C; c += KD_THREADS) {
        if (c == g) continue;
        const double zs = ((double)x[c] - as) * ks, zt = ((double)y[c] - at) * kt;
        ps_o += exp(zs - mxs - lss); pt_o += exp(zt - mxt - lst);
        const double lqs = zs - mxs_n - lss_n, lqt = zt - mxt_n - lst_n, qt = exp(lqt);
        nckd += kd_kl_term(qt, lqt, lqs);
        sqt += qt;
    }
    ps_o = block_sum<KD_THREADS>(ps_o, red); pt_o = block_sum<KD_THREADS>(pt_o, red);
    nckd = block_sum<KD_THREADS>(nckd, red); sqt = block_sum<KD_THREADS>(sqt, red);
    const double zsg = ((double)x[g] - as) * ks, ztg = ((double)y[g] - at) * kt;
    const double lps_g = zsg - mxs - lss, lpt_g = ztg - mxt - lst, ps_g = exp(lps_g), pt_g = exp(lpt_g);
    // torch.log(pred_student) of the reference (float32): -inf when either merged probability is 0 there
    const bool dead = (float)ps_g == 0.f || (float)ps_o == 0.f;
    const double tckd = kd_kl_term(pt_g, lpt_g, lps_g) + kd_kl_term(pt_o, log(pt_o), log(ps_o));
    const double l = dead ? INFINITY : out_scale * ((double)p.alpha * tckd + (double)p.beta * nckd);
    if (threadIdx.x == 0) { row_acc[i] = l; if (row_loss) row_loss[i] = (float)l; }
    if (d) {
        const double gs = grad_scale * inv_n, a = (double)p.alpha, b = (double)p.beta, sum_t = pt_g + pt_o;
        for (int c = threadIdx.x; c < C; c += KD_THREADS) {
            double v;
            if (c == g) {
                v = a * (ps_g * sum_t - pt_g);
            } else {
                const double zs = ((double)x[c] - as) * ks, zt = ((double)y[c] - at) * kt;
                const double qs = exp(zs - mxs_n - lss_n), qt = exp(zt - mxt_n - lst_n);
                v = a * (exp(zs - mxs - lss) * sum_t - pt_o * qs) + b * (qs * sqt - qt);
            }
            d[c] = dead ? NAN : (float)(gs * v);
        }
    }
}

// loss = sum of the row losses / n, summed in row order by one thread
__global__ void kd_mean_kernel(const double* __restrict__ row_acc, int n, float* __restrict__ loss) {
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += row_acc[i];
    loss[0] = (float)(s / n);
}

rlcf_kd_params kd_default_params(void) {
    rlcf_kd_params p;
    p.T_stu = 1.f; p.T_tea = 1.f;                       // kd_distill_loss_v2
    p.alpha = 1.f; p.beta = 0.5f; p.temperature = 1.f;  // dkd_distill_loss
    p.multiplier = 2.f; p.eps = 1e-5f;                  // atkd_distill_loss
    return p;
}

int launch_kd_loss(const float* student, int ld_s, const float* teacher, int ld_t, int n, int C, int mode, const int32_t* target,
                   const rlcf_kd_params* params, float* loss, float* row_loss, float* dlogits, double* row_acc, hipStream_t st) {
    RLCF_ARG_CHECK(student && teacher && row_acc && (loss || row_loss || dlogits));
    if (mode != RLCF_KD_KD && mode != RLCF_KD_DKD && mode != RLCF_KD_ATKD) {
        rlcf_set_error("kd_loss: mode %d is not RLCF_KD_KD / RLCF_KD_DKD / RLCF_KD_ATKD", mode);
        return RLCF_ERR_ARG;
    }
    if (n <= 0 || C <= 0 || C > RLCF_KD_MAX_CLASSES) {
        rlcf_set_error("kd_loss: n = %d rows of C = %d classes (need n >= 1, 1 <= C <= %d)", n, C, RLCF_KD_MAX_CLASSES);
        return RLCF_ERR_ARG;
    }
    RLCF_ARG_CHECK(ld_s >= C && ld_t >= C);
    const rlcf_kd_params p = params ? *params : kd_default_params();
    if (mode == RLCF_KD_KD) RLCF_ARG_CHECK(p.T_stu > 0.f && p.T_tea > 0.f);
    if (mode == RLCF_KD_DKD) RLCF_ARG_CHECK(p.temperature > 0.f);
    kd_rows_kernel<<<dim3(n), dim3(KD_THREADS), 0, st>>>(student, ld_s, teacher, ld_t, C, mode, target, p, 1.0 / n, row_acc, row_loss, dlogits);
    RLCF_LAUNCH_CHECK();
    if (loss) {
        kd_mean_kernel<<<dim3(1), dim3(64), 0, st>>>(row_acc, n, loss);
        RLCF_LAUNCH_CHECK();
    }
    return RLCF_OK;
}

// ------------------------------------------------------------------ split-row form of the KD loss (retrieval: few, long rows)
// retrieval/clip_ret_kd.py:50-92 distils ONE query row of 5 000 (images) or 25 010 (captions) logits per step: one workgroup per row
// leaves 255 of 256 CUs idle on the critical path of every tuning step.  Here a row is cut into chunks of KD_SPLIT_CHUNK elements
// (a compile-time constant: the partition, and with it every bit of the result, is the same on every device) and the chunks run on
// different workgroups, grid = (chunks, rows):
//   pass A  each workgroup reduces its chunk of z_s = s / T_s and z_t = t / T_t to (max, sum of exp(z - max)), in double;
//   pass B  every workgroup of a row folds the row's chunk partials in chunk order (the same arithmetic in each of them: one wave
//           rescales the <= 64 partials, one thread adds them in order) into
//           the row's maxima, log-sum-exps and sum(pt), writes dlogits of its chunk and its partial row loss, and the partial
//           <dlogits, s> the text direction turns into d logit_scale (logits = exp(logit_scale) * <feat, bank>);
//   final   one workgroup sums the partials per row in chunk order and the rows in row order.
// No atomics, no cooperative launch, each element read into registers once per pass; float results are the double values rounded once.
// Gradient as in the one-workgroup kernel: d/ds_c = T_s * (ps_c * sum(pt) - pt_c) / n, sum(pt) = sum over chunks of the chunk's
// share st_k * exp(mt_k - mxt - lst) (kept literal; 1 to within rounding).
#define KD_SPLIT_CHUNK 1024
#define KD_SPLIT_PER (KD_SPLIT_CHUNK / KD_THREADS)
#define KD_SPLIT_WS 8          // doubles of workspace per (row, chunk): A {ms, ss, mt, st}, B {loss, dot}
static_assert(KD_SPLIT_CHUNK % KD_THREADS == 0, "a chunk is a whole number of elements per thread");
static_assert(RLCF_KD_MAX_CLASSES <= 64 * KD_SPLIT_CHUNK, "pass B folds a row's chunk partials on the 64 lanes of one wave");

int kd_split_chunks(int C) { return (C + KD_SPLIT_CHUNK - 1) / KD_SPLIT_CHUNK; }
size_t kd_split_ws_bytes(int n, int C) { return ((size_t)n * kd_split_chunks(C) * KD_SPLIT_WS + (size_t)n) * sizeof(double); }

__global__ __launch_bounds__(KD_THREADS) void kd_split_a_kernel(const float* __restrict__ stu, int ld_s, const float* __restrict__ tea, int ld_t,
                                                                int C, double ks, double kt, double* __restrict__ ws) {
    __shared__ double red[KD_THREADS / 64];
    const int k = blockIdx.x, i = blockIdx.y, c0 = k * KD_SPLIT_CHUNK;
    const float* x = stu + (size_t)i * ld_s;
    const float* y = tea + (size_t)i * ld_t;
    double zs[KD_SPLIT_PER], zt[KD_SPLIT_PER];
    double ms = -INFINITY, mt = -INFINITY;
#pragma unroll
    for (int u = 0; u < KD_SPLIT_PER; ++u) {
        const int c = c0 + u * KD_THREADS + threadIdx.x;
        const bool in = c < C;
        zs[u] = in ? (double)x[c] * ks : -INFINITY;
        zt[u] = in ? (double)y[c] * kt : -INFINITY;
        ms = fmax(ms, zs[u]); mt = fmax(mt, zt[u]);
    }
    ms = block_max<KD_THREADS>(ms, red); mt = block_max<KD_THREADS>(mt, red);
    double ss = 0.0, st = 0.0;
#pragma unroll
    for (int u = 0; u < KD_SPLIT_PER; ++u) {
        const int c = c0 + u * KD_THREADS + threadIdx.x;
        if (c < C) { ss += exp(zs[u] - ms); st += exp(zt[u] - mt); }
    }
    ss = block_sum<KD_THREADS>(ss, red); st = block_sum<KD_THREADS>(st, red);
    if (threadIdx.x == 0) {
        double* w = ws + ((size_t)i * gridDim.x + k) * KD_SPLIT_WS;
        w[0] = ms; w[1] = ss; w[2] = mt; w[3] = st;
    }
}

__global__ __launch_bounds__(KD_THREADS) void kd_split_b_kernel(const float* __restrict__ stu, int ld_s, const float* __restrict__ tea, int ld_t,
                                                                int C, double ks, double kt, double gs, double* __restrict__ ws,
                                                                float* __restrict__ dlogits) {
    __shared__ double red[KD_THREADS / 64];
    const int k = blockIdx.x, i = blockIdx.y, nch = gridDim.x, c0 = k * KD_SPLIT_CHUNK;
    const float* x = stu + (size_t)i * ld_s;
    const float* y = tea + (size_t)i * ld_t;
    double* wrow = ws + (size_t)i * nch * KD_SPLIT_WS;
    // the row's statistics from its chunk partials (identical arithmetic in every workgroup of the row): lane j of the first wave
    // rescales chunk j's sums (one exp each, nch <= 64 lanes), thread 0 adds the terms in chunk order, LDS hands the results round
    __shared__ double term_s[64], term_t[64], stat[5];
    const int t = threadIdx.x;
    double cms = -INFINITY, css = 0.0, cmt = -INFINITY, cst = 0.0, wmt = 0.0;
    if (t < 64) {
        if (t < nch) { cms = wrow[t * KD_SPLIT_WS]; css = wrow[t * KD_SPLIT_WS + 1]; cmt = wrow[t * KD_SPLIT_WS + 2]; cst = wrow[t * KD_SPLIT_WS + 3]; }
        const double wms = wave_max(cms);
        wmt = wave_max(cmt);
        term_s[t] = t < nch ? css * exp(cms - wms) : 0.0;
        term_t[t] = t < nch ? cst * exp(cmt - wmt) : 0.0;
        if (t == 0) { stat[0] = wms; stat[1] = wmt; }
    }
    __syncthreads();
    if (t == 0) {
        double a = 0.0, b = 0.0;
        for (int j = 0; j < nch; ++j) { a += term_s[j]; b += term_t[j]; }
        stat[2] = log(a); stat[3] = log(b);
    }
    __syncthreads();
    if (t < 64) term_t[t] = t < nch ? cst * exp(cmt - wmt - stat[3]) : 0.0;          // the chunk's share of sum(pt)
    __syncthreads();
    if (t == 0) {
        double a = 0.0;
        for (int j = 0; j < nch; ++j) a += term_t[j];
        stat[4] = a;
    }
    __syncthreads();
    const double mxs = stat[0], mxt = stat[1], lss = stat[2], lst = stat[3], spt = stat[4];
    float* d = dlogits ? dlogits + (size_t)i * C : nullptr;
    double l = 0.0, dot = 0.0;
#pragma unroll
    for (int u = 0; u < KD_SPLIT_PER; ++u) {
        const int c = c0 + u * KD_THREADS + threadIdx.x;
        if (c < C) {
            const float xs = x[c];
            const double lps = (double)xs * ks - mxs - lss, pt = exp((double)y[c] * kt - mxt - lst);
            l += -pt * lps;
            const float g = (float)(gs * (exp(lps) * spt - pt));
            if (d) d[c] = g;
            dot += (double)g * (double)xs;
        }
    }
    l = block_sum<KD_THREADS>(l, red); dot = block_sum<KD_THREADS>(dot, red);
    if (threadIdx.x == 0) { wrow[k * KD_SPLIT_WS + 4] = l; wrow[k * KD_SPLIT_WS + 5] = dot; }
}

// row i: loss_i = out_scale * sum_k partial (chunk order);  loss = sum_i loss_i / n (row order);  dot = sum_i sum_k <dlogits, s> partials
__global__ __launch_bounds__(KD_THREADS) void kd_split_final_kernel(double* __restrict__ ws, int n, int nch, double out_scale,
                                                                    float* __restrict__ loss, float* __restrict__ row_loss, float* __restrict__ dot) {
    double* row_acc = ws + (size_t)n * nch * KD_SPLIT_WS;
    __shared__ double sdot[KD_THREADS];
    double dsum = 0.0;
    for (int i = threadIdx.x; i < n; i += KD_THREADS) {
        const double* w = ws + (size_t)i * nch * KD_SPLIT_WS;
        double l = 0.0, dd = 0.0;
        for (int k = 0; k < nch; ++k) { l += w[k * KD_SPLIT_WS + 4]; dd += w[k * KD_SPLIT_WS + 5]; }
        l *= out_scale;
        row_acc[i] = l;
        if (row_loss) row_loss[i] = (float)l;
        dsum += dd;
    }
    sdot[threadIdx.x] = dsum;
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (loss) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += row_acc[i];
        loss[0] = (float)(s / n);
    }
    if (dot) {
        double s = 0.0;
        for (int t = 0; t < KD_THREADS && t < n; ++t) s += sdot[t];
        dot[0] = (float)s;
    }
}

// KD only (RLCF_KD_KD).  ws: kd_split_ws_bytes(n, C) bytes.  dot (optional): sum_i <dlogits_i, student_i>, one float.
int launch_kd_loss_split(const float* student, int ld_s, const float* teacher, int ld_t, int n, int C, const rlcf_kd_params* params, float* loss,
                         float* row_loss, float* dlogits, float* dot, double* ws, hipStream_t st) {
    RLCF_ARG_CHECK(student && teacher && ws && (loss || row_loss || dlogits || dot));
    if (n <= 0 || n > RLCF_KD_SPLIT_MAX_ROWS || C <= 0 || C > RLCF_KD_MAX_CLASSES) {          // (rows are the grid's y dimension)
        rlcf_set_error("kd_loss_split: n = %d rows of C = %d classes (need 1 <= n <= %d, 1 <= C <= %d)", n, C, RLCF_KD_SPLIT_MAX_ROWS,
                       RLCF_KD_MAX_CLASSES);
        return RLCF_ERR_ARG;
    }
    RLCF_ARG_CHECK(ld_s >= C && ld_t >= C);
    const rlcf_kd_params p = params ? *params : kd_default_params();
    RLCF_ARG_CHECK(p.T_stu > 0.f && p.T_tea > 0.f);
    const double ks = 1.0 / (double)p.T_stu, kt = 1.0 / (double)p.T_tea, out_scale = (double)p.T_stu * (double)p.T_stu;
    const int nch = kd_split_chunks(C);
    const dim3 grid(nch, n);
    kd_split_a_kernel<<<grid, dim3(KD_THREADS), 0, st>>>(student, ld_s, teacher, ld_t, C, ks, kt, ws);
    RLCF_LAUNCH_CHECK();
    kd_split_b_kernel<<<grid, dim3(KD_THREADS), 0, st>>>(student, ld_s, teacher, ld_t, C, ks, kt, out_scale * ks / n, ws, dlogits);
    RLCF_LAUNCH_CHECK();
    kd_split_final_kernel<<<dim3(1), dim3(KD_THREADS), 0, st>>>(ws, n, nch, out_scale, loss, row_loss, dot);
    RLCF_LAUNCH_CHECK();
    return RLCF_OK;
}

// ------------------------------------------------------------------ recall ranks (LAVIS RetrievalTask._report_metrics)
// rank of a score row = the number of columns that score STRICTLY higher than the best-scoring ground-truth column; one workgroup
// per row.  Ground truth: gt_off != NULL: CSR (row r owns gt_idx[gt_off[r] .. gt_off[r + 1])), image -> text;  gt_off == NULL: one
// index per row, text -> image.  The reference ranks with np.argsort(...)[::-1], whose order among exactly equal scores is
// unspecified: here a column that ties with the ground-truth score does not outrank it (ties count in its favour).
// A row with no ground truth or an index outside [0, cols) gets rank -1.
__global__ __launch_bounds__(KD_THREADS) void retrieval_ranks_kernel(const float* __restrict__ scores, int ld, int cols,
                                                                     const int32_t* __restrict__ gt_off, const int32_t* __restrict__ gt_idx,
                                                                     int32_t* __restrict__ ranks) {
    __shared__ int redc[KD_THREADS / 64];
    const int r = blockIdx.x;
    const float* s = scores + (size_t)r * ld;
    const int b = gt_off ? gt_off[r] : r, e = gt_off ? gt_off[r + 1] : r + 1;
    bool ok = e > b;
    float best = -INFINITY;
    for (int j = b; j < e; ++j) {                     // a handful of captions per image: every thread walks them
        const int g = gt_idx[j];
        if (g < 0 || g >= cols) { ok = false; break; }
        best = fmaxf(best, s[g]);
    }
    if (!ok) { if (threadIdx.x == 0) ranks[r] = -1; return; }
    int cnt = 0;
    for (int c = threadIdx.x; c < cols; c += KD_THREADS) cnt += s[c] > best ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((threadIdx.x & 63) == 0) redc[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < KD_THREADS / 64; ++w) t += redc[w];
        ranks[r] = t;
    }
}

int launch_retrieval_ranks(const float* scores, int ld, int rows, int cols, const int32_t* gt_off, const int32_t* gt_idx, int32_t* ranks,
                           hipStream_t st) {
    RLCF_ARG_CHECK(scores && gt_idx && ranks && rows > 0 && cols > 0 && ld >= cols);
    retrieval_ranks_kernel<<<dim3(rows), dim3(KD_THREADS), 0, st>>>(scores, ld, cols, gt_off, gt_idx, ranks);
    RLCF_LAUNCH_CHECK();
    return RLCF_OK;
}
