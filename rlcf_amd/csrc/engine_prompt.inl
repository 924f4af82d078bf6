// Part of engine.hip (one translation unit: #include'd there): the prompt-tuning step — sparse class passes, one test sample
// (engine_tta_sample: TPT/tpt_cls_rl.py:47-79 + the harness body :251-268), B test samples per tower pass (engine_tta_batch).
// Sparse backward layout for n_e = n_sel*K sampled (view, class) pairs.
static int sparse_ensure(rlcf_engine* e, int n_e_per_group, hipStream_t st, int groups = 1) {
    if (n_e_per_group <= e->sp_max_e && groups <= e->sp_groups) return RLCF_OK;
    ClipModel& m = e->model[RLCF_STUDENT];
    const TextLayout& L = e->lay[0];
    const int Wt = m.cfg.text_width, D = m.cfg.embed_dim;
    groups = std::max(groups, e->sp_groups);
    n_e_per_group = std::max(n_e_per_group, e->sp_max_e);
    const int T = groups * (L.pre_rows + n_e_per_group * L.lmax);
    const int n_e = groups * n_e_per_group;
    TRY(e->sp_seqs.ensure((size_t)(n_e + groups) * sizeof(rlcf_seq))); TRY(e->sp_eot_rows.ensure(n_e * sizeof(int32_t)));
    TRY(e->sp_row_src.ensure((size_t)T * sizeof(int32_t)));
    std::vector<int32_t> list;
    if (L.pre_rows > 0) for (int j = 0; j < L.n_ctx; ++j) list.push_back(1 + j);
    else for (int k = 0; k < n_e_per_group; ++k) for (int j = 0; j < L.n_ctx; ++j) list.push_back(k * L.lmax + 1 + j);
    TRY(upload(e->sp_ctx_rows_list, list, st));
    TRY(e->sp_dtxt.ensure((size_t)n_e * D * sizeof(float))); TRY(e->sp_txt.ensure((size_t)n_e * D * sizeof(float)));
    TRY(e->sp_inv_norm.ensure(n_e * sizeof(float))); TRY(e->sp_eot_x.ensure((size_t)n_e * Wt * sizeof(float)));
    TRY(e->sp_eot_ln.ensure((size_t)n_e * Wt * sizeof(float))); TRY(e->sp_u.ensure((size_t)n_e * D * sizeof(float)));
    TRY(e->sp_du.ensure((size_t)std::max(n_e, L.C) * D * sizeof(float))); TRY(e->sp_dxe.ensure((size_t)std::max(n_e, L.C) * Wt * sizeof(float)));
    TRY(tower_ensure(e->st, T, Wt, st));
    TRY(tower_ensure_saved(e->st, T, Wt, m.cfg.text_layers, st));
    TRY(bwd_ensure(e, T, Wt));
    e->sp_max_e = n_e_per_group; e->sp_T = T; e->sp_groups = groups;
    return RLCF_OK;
}

// the two halves of the sparse pass: the forward over the sampled (view, class) pairs needs only their class indices (top-K of the
// student's own logits) — the one-image call runs it next to the reward models' tower pass —, the backward needs the rewards
static TextPassIO sparse_io(rlcf_engine* e, int n_e) {
    const TextLayout& L = e->lay[0];
    TextPassIO io{};
    io.seqs = e->sp_seqs.as<rlcf_seq>(); io.n_seq = n_e + (L.pre_rows > 0 ? 1 : 0); io.max_q_len = L.max_q_len; io.T = L.pre_rows + n_e * L.lmax;
    io.n_cls = n_e;
    io.attn_pairs = (long)(n_e * (L.mean_len * (L.pre_rows + (L.mean_len + 1) * 0.5)));
    io.eot_rows = e->sp_eot_rows.as<int32_t>(); io.row_src = e->sp_row_src.as<int32_t>();
    io.eot_x = e->sp_eot_x.as<float>(); io.eot_ln = e->sp_eot_ln.as<float>(); io.u = e->sp_u.as<float>();
    io.inv_norm = e->sp_inv_norm.as<float>(); io.txt = e->sp_txt.as<float>();
    io.ctx_row_tab = L.ctx_general ? L.ctx_row.as<int32_t>() : nullptr;
    return io;
}
static int sparse_forward(rlcf_engine* e, const float* ctx, const int32_t* cls, int n_e, hipStream_t st) {
    ClipModel& m = e->model[RLCF_STUDENT];
    const TextLayout& L = e->lay[0];
    TRY(launch_build_sparse_layout(cls, 1, n_e, L.class_start.as<int32_t>(), L.class_len.as<int32_t>(), L.class_eot_off.as<int32_t>(),
                                   L.lmax, L.pre_rows, e->sp_seqs.as<rlcf_seq>(), e->sp_eot_rows.as<int32_t>(),
                                   e->sp_row_src.as<int32_t>(), st));
    return text_forward(e, m, L, e->st, ctx, sparse_io(e, n_e), true, st);
}
static int sparse_backward_only(rlcf_engine* e, const float* sel_feat, const int32_t* cls, int n_e, int K, const float* dlogits, float* dctx,
                                hipStream_t st) {
    ClipModel& m = e->model[RLCF_STUDENT];
    const TextLayout& L = e->lay[0];
    const int D = m.cfg.embed_dim;
    TRY(launch_dtxt_sparse(dlogits, cls, sel_feat, n_e, K, L.C, D, m.logit_scale_exp, e->sp_dtxt.as<float>(), st));
    return text_backward(e, m, e->st, sparse_io(e, n_e), L.max_keys, e->sp_dtxt.as<float>(), e->sp_du.as<float>(), e->sp_dxe.as<float>(),
                         e->sp_ctx_rows_list.as<int32_t>(), L.pre_rows > 0 ? 1 : n_e, L.n_ctx, dctx, st);
}
static int sparse_backward(rlcf_engine* e, const float* ctx, const float* sel_feat, const int32_t* cls, int n_e, int K,
                           const float* dlogits, float* dctx, hipStream_t st) {
    TRY(sparse_forward(e, ctx, cls, n_e, st));
    return sparse_backward_only(e, sel_feat, cls, n_e, K, dlogits, dctx, st);
}

// ------------------------------------------------------------------ one test sample
// set_image_features of every reward model on the selected views (clip_reward.py:59-61,130-137,259-270); the optional
// output is the per-model blocks [rows, Dr_m] one after another.
static int reward_encode(rlcf_engine* e, int rows, int in_res, float* out_concat, hipStream_t st) {
    for (int m = 0; m < e->n_rewards; ++m) {
        const int Dr = e->model[RLCF_REWARD + m].cfg.embed_dim;
        TRY(engine_encode_image(e, RLCF_REWARD + m, e->views_sel.as<float>(), rows, e->rimg[m].as<float>(), st, in_res));
        if (out_concat) {
            RLCF_HIP_CHECK(hipMemcpyAsync(out_concat, e->rimg[m].p, (size_t)rows * Dr * sizeof(float), hipMemcpyDeviceToDevice, st));
            out_concat += (size_t)rows * Dr;
        }
    }
    return RLCF_OK;
}
static RewardBank reward_bank(const rlcf_engine* e) {
    RewardBank b{};
    b.n = e->n_rewards;
    for (int m = 0; m < e->n_rewards; ++m) {
        b.class_feat[m] = e->reward_cls[m].as<float>(); b.reward_img[m] = e->rimg[m].as<float>();
        b.Dr[m] = e->model[RLCF_REWARD + m].cfg.embed_dim;
        b.mix[m] = e->reward_mean ? 1.f : e->reward_mix[m];
    }
    b.post_div = e->reward_mean ? (float)e->n_rewards : 1.f;
    return b;
}

// ------------------------------------------------------------------ what every tuning entry shares: the check, the loss, the optimizer
// One rule set for all entries (api.hip calls it once per call, before anything is launched; the engine functions below trust it).
// kinds: LOSS_BIT()s of the losses the entry has a form of; what: TTA_* traits.  RLCF_ERR_ARG for what the arguments ask, RLCF_ERR_STATE
// for what the engine lacks; the argument rules come first.
int tta_args_check(const rlcf_engine* e, const rlcf_tta_args* a, const char* entry, unsigned kinds, unsigned what) {
    static const char* const name[] = {"the reward loss", "the distillation loss RLCF_F_KD", "the distillation loss RLCF_F_DKD",
                                       "the distillation loss RLCF_F_ATKD", "the TPT loss RLCF_F_TPT"};
    LossKind k = loss_kind(a);
    if ((what & TTA_DISTILS) && k == LOSS_RL) k = LOSS_KD;
    if (!(kinds & LOSS_BIT(k))) {
        // tune_cls_kd.py has no prompt, batched, lane or policy form, clip_ret_kd.py no DKD / ATKD form; TPT/tpt_cls.py and tune_cls_tpt.py
        // have no lane and no retrieval form
        rlcf_set_error("%s: %s has no form on this entry (the distillation losses RLCF_F_KD / RLCF_F_DKD / RLCF_F_ATKD run on rlcf_tta_sample_ln / "
                       "rlcf_tta_sample_visual, kd_distill_loss_v2 alone on the two retrieval *_kd entries; RLCF_F_TPT on rlcf_tta_sample / "
                       "rlcf_tta_sample_ln / rlcf_tta_sample_visual / rlcf_tta_batch / rlcf_tta_batch_ln)", entry, name[k]);
        return RLCF_ERR_ARG;
    }
    if (k != LOSS_RL) {
        const int refused = RLCF_F_MIN_ENTROPY | (k == LOSS_TPT ? RLCF_F_KD_MASK : 0) | ((what & TTA_ROWS_IN_ORDER) ? 0 : RLCF_F_NO_SELECTION);
        if (a->flags & refused) {
            rlcf_set_error("%s: %s takes no second loss, no min-entropy regulariser and no retrieval rows (flags 0x%x)", entry, name[k], a->flags);
            return RLCF_ERR_ARG;
        }
    }
    if (loss_distils(k) && e->n_rewards != 1) {      // CLIPRewardsMultiple has no calulate_similarity (clip_reward.py:180-307)
        rlcf_set_error("%s: the distillation losses need exactly one reward model (the engine holds %d)", entry, e->n_rewards);
        return RLCF_ERR_ARG;
    }
    const bool image_bank = (what & TTA_IMAGE_BANK) != 0;
    if (e->C <= 0 || e->image_bank != image_bank || (e->n_rewards <= 0 && k != LOSS_TPT)) {      // (the TPT loss needs no reward model)
        rlcf_set_error("%s: %s bank / reward model not set", entry, image_bank ? "image" : "class");
        return RLCF_ERR_STATE;
    }
    if ((what & TTA_PROMPT) && e->n_ctx <= 0) {
        rlcf_set_error("%s: prompt tuning needs a class bank with learnable context rows (n_ctx > 0)", entry);
        return RLCF_ERR_STATE;
    }
    if (k == LOSS_RL && !(a->sample_k > 0 && a->sample_k <= 32 && a->sample_k <= e->C)) {        // (only the reward loss samples classes)
        rlcf_set_error("%s: sample_k = %d (need 1 <= sample_k <= 32 and <= the bank's %d entries)", entry, a->sample_k, e->C);
        return RLCF_ERR_ARG;
    }
    return RLCF_OK;
}

#define COPY_OUT(dst, src, bytes) do { if (dst) RLCF_HIP_CHECK(hipMemcpyAsync((dst), (src), (bytes), hipMemcpyDeviceToDevice, st)); } while (0)
// out[0] = sum_i a[i] * b[i]  (one block, fixed reduction order)
__global__ void dot_kernel(const float* __restrict__ a, const float* __restrict__ b, int n, float* __restrict__ out) {
    __shared__ float red[256];
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) acc += a[i] * b[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}
// The loss of one step over `groups` samples of n_sel rows of e->sel_logits: dlogits into e->dlogits, the loss [groups] into loss_out
// (optional), and for the reward loss the sampled classes into e->topk_idx (with loss_out: their e->clip_score / e->rewards too).
//   LOSS_RL   top-K sampling, CLIP reward, baseline, reward-weighted CE (tpt_cls_rl.py:63-74)
//   LOSS_KD / DKD / ATKD  against e->kd_teacher (tune_cls_kd.py:48-55).  rkd != NULL: the retrieval form, kd_distill_loss_v2 with these
//             temperatures over rows as long as the bank (clip_ret_kd.py:62,87); the split-row kernels take over from the
//             one-workgroup-per-row kernel where they are faster (profiles/retrieval_kd_notes.md) — a choice by C alone, so a given
//             query computes the same bits on every device
//   LOSS_TPT  avg_entropy of each sample's rows (tpt_cls.py:49-72); no reward pass, no teacher, no top-K stage
// dot (optional, one row) = <dlogits, sel_logits>, one float.
static int loss_step(rlcf_engine* e, const rlcf_tta_args* a, LossKind kind, int groups, int n_sel, const rlcf_kd_params* rkd, float* dot,
                     float* loss_out, hipStream_t st) {
    const int C = e->C;
    const float* rows = e->sel_logits.as<float>();
    float* dlogits = e->dlogits.as<float>();
    if (kind == LOSS_RL) {
        TRY(launch_reward_loss_bank(rows, C, nullptr, groups, n_sel, C, a->sample_k, reward_bank(e), a->clipscore_weight, a->flags,
                                    a->min_entropy_w, e->topk_idx.as<int32_t>(), loss_out ? e->clip_score.as<float>() : nullptr,
                                    loss_out ? e->rewards.as<float>() : nullptr, loss_out, dlogits, e->rl_stats.as<float>(), st));
    } else if (kind == LOSS_TPT) {
        TRY(e->loss_ws.ensure(tpt_ws_bytes(groups, n_sel, C)));
        TRY(launch_tpt_loss(rows, C, groups, n_sel, C, loss_out, dlogits, e->loss_ws.as<double>(), st));
    } else if (rkd && C >= KD_SPLIT_MIN_C) {     // (this kernel hands the dot product over with the gradient row)
        TRY(e->loss_ws.ensure(kd_split_ws_bytes(n_sel, C)));
        return launch_kd_loss_split(rows, C, e->kd_teacher.as<float>(), C, n_sel, C, rkd, loss_out, nullptr, dlogits, dot, e->loss_ws.as<double>(), st);
    } else {
        TRY(e->loss_ws.ensure((size_t)n_sel * sizeof(double)));
        TRY(launch_kd_loss(rows, C, e->kd_teacher.as<float>(), C, n_sel, C, kind, nullptr, rkd, loss_out, nullptr, dlogits, e->loss_ws.as<double>(), st));
    }
    if (dot) {
        RLCF_ARG_CHECK(groups * n_sel == 1);
        dot_kernel<<<dim3(1), dim3(256), 0, st>>>(dlogits, rows, C, dot);
        RLCF_LAUNCH_CHECK();
    }
    return RLCF_OK;
}
// what the first step's loss leaves for the caller (rows = the rows of dlogits, n_e = the sampled (row, class) pairs).  The distillation
// and TPT losses sample no classes: topk_idx / clip_score / rewards stay unwritten.
static int loss_copy_out(rlcf_engine* e, const rlcf_tta_out* out, LossKind kind, int rows, int n_e, hipStream_t st) {
    if (kind == LOSS_RL) {
        COPY_OUT(out->topk_idx, e->topk_idx.p, (size_t)n_e * sizeof(int32_t));
        COPY_OUT(out->clip_score, e->clip_score.p, (size_t)n_e * sizeof(float));
        COPY_OUT(out->rewards, e->rewards.p, (size_t)n_e * sizeof(float));
    }
    COPY_OUT(out->loss, e->loss.p, sizeof(float));
    COPY_OUT(out->dlogits, e->dlogits.p, (size_t)rows * e->C * sizeof(float));
    return RLCF_OK;
}
// scaler.step(optimizer) (tpt_cls_rl.py:78) as AdamW step j + 1 over one or two buffers of one optimizer, `sets` parameter sets each (one
// per test sample of a fused batch): a gradient with an inf / NaN anywhere in a set's buffers skips that set's update (the same inputs
// give the same gradient at the following steps, so the host-side step number never meets an applied step after a skipped one).
// Derived weight forms are the caller's to refresh.
struct OptimBuf { float *params; const float* grad; float *m, *v; int64_t count; };      // count: floats of one set
static int optim_step(rlcf_engine* e, const rlcf_tta_args* a, int j, const OptimBuf* bufs, int n_bufs, int sets, int32_t* step_skipped_out,
                      hipStream_t st) {
    int32_t* skip = e->step_skip.as<int32_t>();
    for (int i = 0; i < n_bufs; ++i) TRY(launch_grad_nonfinite(bufs[i].grad, bufs[i].count, sets, skip, st, i > 0));
    if (step_skipped_out) COPY_OUT(step_skipped_out + j, skip, sizeof(int32_t));
    for (int i = 0; i < n_bufs; ++i)
        TRY(launch_adamw(bufs[i].params, bufs[i].grad, bufs[i].m, bufs[i].v, sets * bufs[i].count, j + 1, a->lr, a->beta1, a->beta2, a->eps,
                         a->weight_decay, st, skip, bufs[i].count));
    return RLCF_OK;
}

// Harness body TPT/tpt_cls_rl.py:251-262 around test_time_tuning (:47-79).  What feeds the step its image features:
//   views != NULL       the student image tower runs over them (rlcf_tta_sample)
//   feats_raw != NULL   the caller's un-normalised features [N, D] are L2-normalised (rlcf_tta_sample_feats; TPT/clip/cocoop.py:208)
//   both NULL           e->img_feat already holds the normalised features of this sample (rlcf_tta_sample_cocoop: the generator's pass)
// Without views there is nothing for a reward model to read: the entries allow those two forms with the TPT loss alone.
static int tta_sample_core(rlcf_engine* e, const float* views, const float* feats_raw, int N, const rlcf_tta_args* a, const rlcf_tta_out* out,
                           hipStream_t st) {
    ClipModel& s = e->model[RLCF_STUDENT];
    RLCF_ARG_CHECK(a && N > 0 && N <= e->max_views && a->tta_steps >= 0);
    const LossKind kind = loss_kind(a);
    const int C = e->C, K = kind == LOSS_TPT ? 1 : a->sample_k, D = s.cfg.embed_dim, Wt = s.cfg.text_width, n_ctx = e->n_ctx;
    const int n_sel = n_selected(a, N);                       // int() truncation, tpt_cls_rl.py:34
    if (a->tta_steps > 0 && n_sel <= 0) { rlcf_set_error("int(N*selection_p) == 0 views selected (N=%d, p=%g)", N, a->selection_p); return RLCF_ERR_ARG; }
    const size_t cb = (size_t)n_ctx * Wt * sizeof(float);
    const size_t img_elems = (size_t)3 * s.cfg.image_resolution * s.cfg.image_resolution;
    const rlcf_tta_out none{};
    if (!out) out = &none;
    const bool sparse_ok = a->sparse_backward && (a->flags & RLCF_F_REWARD_PROCESS) && !(a->flags & RLCF_F_PROCESS_BATCH) &&
                           !(a->flags & RLCF_F_MIN_ENTROPY) && K > 1 && kind == LOSS_RL;      // (the TPT loss is dense over the classes)
    const int n_e = n_sel * K;
    if (a->tta_steps > 0) {
        if (sparse_ok) TRY(sparse_ensure(e, n_e, st));
        else {
            TRY(tower_ensure_saved(e->tt, e->lay[0].T, Wt, s.cfg.text_layers, st));
            TRY(bwd_ensure(e, e->lay[0].T, Wt));
            TRY(e->sp_du.ensure((size_t)C * D * sizeof(float))); TRY(e->sp_dxe.ensure((size_t)C * Wt * sizeof(float)));
        }
    }
    e->last_flops = 0.0;
    float* ctx = e->ctx.as<float>();
    // model.reset() + optimizer.load_state_dict(optim_state): custom_clip.py:161-164, tpt_cls_rl.py:251-255
    RLCF_HIP_CHECK(hipMemcpyAsync(ctx, a->ctx_in ? (const void*)a->ctx_in : e->ctx_init.p, cb, hipMemcpyDeviceToDevice, st));
    RLCF_HIP_CHECK(hipMemsetAsync(e->adam_m.p, 0, cb, st));
    RLCF_HIP_CHECK(hipMemsetAsync(e->adam_v.p, 0, cb, st));
    // student image features of all N views: computed once (the image tower is frozen, custom_clip.py:325-327)
    if (views) TRY(engine_encode_image(e, RLCF_STUDENT, views, N, e->img_feat.as<float>(), st));
    else if (feats_raw) TRY(launch_l2norm_rows(feats_raw, e->img_feat.as<float>(), nullptr, N, D, st));
    TextPassIO io = full_io(e, e->lay[0]);
    static int no_overlap = -1;                              // RLCF_NO_OVERLAP=1: everything on the caller's stream (benchmarks)
    if (no_overlap < 0) { const char* ev = getenv("RLCF_NO_OVERLAP"); no_overlap = ev ? atoi(ev) : 0; }
    bool vit_rewards = true;
    for (int m = 0; m < e->n_rewards; ++m) vit_rewards = vit_rewards && !is_resnet(e->model[RLCF_REWARD + m].cfg);
    const bool overlap = sparse_ok && vit_rewards && !no_overlap && !e->no_side && !g_prof.enabled && e->side && prec_x3(e) && !prec_single(e);
    bool fwd_done = false;
    for (int j = 0; j < a->tta_steps; ++j) {
        // step 0 runs on ctx == ctx_init: its text features are the cached txt0 (the dense-backward
        // path still needs this pass for its saved activations)
        const bool cached = (j == 0 && sparse_ok && !a->ctx_in);
        if (!cached) TRY(text_forward(e, s, e->lay[0], e->tt, ctx, io, !sparse_ok, st));
        const float* txt_j = cached ? e->txt0.as<float>() : e->txt.as<float>();
        if (j == 0) {   // tpt_cls_rl.py:57-59
            TRY(engine_logits(e, e->img_feat.as<float>(), N, txt_j, C, e->logits.as<float>(), st));
            TRY(launch_entropy_select(e->logits.as<float>(), N, C, n_sel, e->entropy.as<float>(), e->sel_idx.as<int32_t>(), st));
            TRY(launch_gather_rows(e->img_feat.as<float>(), D, e->sel_idx.as<int32_t>(), e->sel_feat.as<float>(), D, n_sel, D, st));
            if (views) TRY(launch_gather_rows(views, (int)img_elems, e->sel_idx.as<int32_t>(), e->views_sel.as<float>(), (int)img_elems, n_sel, (int)img_elems, st));
            // the reward models' pass over the selected views depends on nothing the student does from here to the loss, and at one
            // image's sizes neither it nor the sparse text forward fills the chip: second stream, joined before the loss kernel
            if (overlap) {
                // the side stream's own A-operand buffer: the patch matrix of the selected views or a <= 512-row token matrix against a
                // W x 4W weight, whichever reward model needs more (the main stream keeps a_hi for the text passes it runs meanwhile)
                size_t need2 = 0;
                for (int m = 0; m < e->n_rewards; ++m) {
                    const ClipModel& rm = e->model[RLCF_REWARD + m];
                    need2 = std::max(need2, (size_t)n_sel * rm.tokens * std::max(rm.Kp, 4 * rm.cfg.vision_width));
                }
                if (need2 > e->a_split2_elems) { TRY(e->a_hi2.ensure(need2 * 4)); e->a_split2_elems = need2; }
                RLCF_HIP_CHECK(hipEventRecord(e->ev_fork, st));
                RLCF_HIP_CHECK(hipStreamWaitEvent(e->side, e->ev_fork, 0));
                e->ws_sel = 1;
                const int rc_side = reward_encode(e, n_sel, s.cfg.image_resolution, out->reward_image_features, e->side);
                e->ws_sel = 0;
                const hipError_t er = hipEventRecord(e->ev_join, e->side);      // (recorded even after an error: the main stream must not run ahead)
                if (rc_side != RLCF_OK || er != hipSuccess) {
                    (void)hipStreamWaitEvent(st, e->ev_join, 0);
                    if (er != hipSuccess) { (void)hipStreamSynchronize(e->side); rlcf_set_error("hipEventRecord(ev_join): %s", hipGetErrorString(er)); return RLCF_ERR_HIP; }
                    return rc_side;
                }
            } else if (kind != LOSS_TPT) {
                TRY(reward_encode(e, n_sel, s.cfg.image_resolution, out->reward_image_features, st));
            }
            TRY(launch_gather_rows(e->logits.as<float>(), C, e->sel_idx.as<int32_t>(), e->sel_logits.as<float>(), C, n_sel, C, st));
            if (overlap) {
                // whatever happens on the main stream, it joins the side stream before this call returns: the side stream writes
                // e->vt, e->rimg and the caller's reward_image_features
                int rc_main = launch_topk_rows(e->sel_logits.as<float>(), C, n_sel, C, K, e->topk_idx.as<int32_t>(), e->rl_stats.as<float>(), st);
                if (rc_main == RLCF_OK) rc_main = sparse_forward(e, ctx, e->topk_idx.as<int32_t>(), n_e, st);
                fwd_done = true;
                const hipError_t ej = hipStreamWaitEvent(st, e->ev_join, 0);
                if (rc_main != RLCF_OK) { if (ej != hipSuccess) (void)hipStreamSynchronize(e->side); return rc_main; }
                if (ej != hipSuccess) { (void)hipStreamSynchronize(e->side); rlcf_set_error("hipStreamWaitEvent(ev_join): %s", hipGetErrorString(ej)); return RLCF_ERR_HIP; }
            }
            COPY_OUT(out->logits, e->logits.p, (size_t)N * C * sizeof(float));
            COPY_OUT(out->entropy, e->entropy.p, N * sizeof(float));
            COPY_OUT(out->selected_idx, e->sel_idx.p, n_sel * sizeof(int32_t));
        } else {        // tpt_cls_rl.py:55 — selected views only; their image features are unchanged
            TRY(engine_logits(e, e->sel_feat.as<float>(), n_sel, txt_j, C, e->sel_logits.as<float>(), st));
        }
        TRY(loss_step(e, a, kind, 1, n_sel, nullptr, nullptr, e->loss.as<float>(), st));
        if (sparse_ok && fwd_done) {
            TRY(sparse_backward_only(e, e->sel_feat.as<float>(), e->topk_idx.as<int32_t>(), n_e, K, e->dlogits.as<float>(), e->ctx_grad.as<float>(), st));
            fwd_done = false;
        } else if (sparse_ok) {
            TRY(sparse_backward(e, ctx, e->sel_feat.as<float>(), e->topk_idx.as<int32_t>(), n_e, K, e->dlogits.as<float>(),
                                e->ctx_grad.as<float>(), st));
        } else {
            TRY(launch_dtxt_dense(e->dlogits.as<float>(), e->sel_feat.as<float>(), n_sel, C, D, s.logit_scale_exp, e->dtxt_dense.as<float>(), st));
            TRY(text_backward(e, s, e->tt, io, e->lay[0].max_keys, e->dtxt_dense.as<float>(), e->sp_du.as<float>(), e->sp_dxe.as<float>(),
                              e->lay[0].ctx_rows_list.as<int32_t>(), e->lay[0].n_copies, n_ctx, e->ctx_grad.as<float>(), st));
        }
        if (j == 0) {
            TRY(loss_copy_out(e, out, kind, n_sel, n_e, st));
            COPY_OUT(out->ctx_grad, e->ctx_grad.p, cb);
        }
        const OptimBuf ob{ctx, e->ctx_grad.as<float>(), e->adam_m.as<float>(), e->adam_v.as<float>(), (int64_t)n_ctx * Wt};
        TRY(optim_step(e, a, j, &ob, 1, 1, out->step_skipped, st));
    }
    // final inference on the clean view (views[0]) with the adapted prompt, tpt_cls_rl.py:260-262;
    // its image feature is row 0 of img_feat (frozen image tower: identical to re-encoding it).
    COPY_OUT(out->ctx_after, ctx, cb);
    if (a->skip_final) return RLCF_OK;
    TRY(text_forward(e, s, e->lay[0], e->tt, ctx, io, false, st));
    TRY(engine_logits(e, e->img_feat.as<float>(), 1, e->txt.as<float>(), C, e->final_logits.as<float>(), st));
    TRY(launch_top5(e->final_logits.as<float>(), C, e->top5.as<int32_t>(), st));
    COPY_OUT(out->final_logits, e->final_logits.p, (size_t)C * sizeof(float));
    COPY_OUT(out->top5, e->top5.p, 5 * sizeof(int32_t));
    return RLCF_OK;
}
int engine_tta_sample(rlcf_engine* e, const float* views, int N, const rlcf_tta_args* a, const rlcf_tta_out* out, hipStream_t st) {
    return tta_sample_core(e, views, nullptr, N, a, out, st);
}

// ------------------------------------------------------------------ CoCoOp (TPT/clip/cocoop.py, the --cocoop branch of TPT/tpt_cls.py)
// The generator's ctx parameter is the class bank's ctx_init (cocoop.py:51); the meta-net is the student's (:52-56).
int engine_set_meta_net(rlcf_engine* e, const float* w1, const float* b1, const float* w2, const float* b2, int H, hipStream_t st) {
    const rlcf_clip_cfg& c = e->model[RLCF_STUDENT].cfg;
    const size_t D = (size_t)c.embed_dim, W = (size_t)c.text_width, h = (size_t)H;
    TRY(e->mn_w1.ensure(h * D * sizeof(float))); TRY(e->mn_b1.ensure(h * sizeof(float)));
    TRY(e->mn_w2.ensure(W * h * sizeof(float))); TRY(e->mn_b2.ensure(W * sizeof(float)));
    RLCF_HIP_CHECK(hipMemcpyAsync(e->mn_w1.p, w1, h * D * sizeof(float), hipMemcpyDeviceToDevice, st));
    RLCF_HIP_CHECK(hipMemcpyAsync(e->mn_b1.p, b1, h * sizeof(float), hipMemcpyDeviceToDevice, st));
    RLCF_HIP_CHECK(hipMemcpyAsync(e->mn_w2.p, w2, W * h * sizeof(float), hipMemcpyDeviceToDevice, st));
    RLCF_HIP_CHECK(hipMemcpyAsync(e->mn_b2.p, b2, W * sizeof(float), hipMemcpyDeviceToDevice, st));
    e->mn_H = H;
    return RLCF_OK;
}
// what a generator pass needs of the engine: a meta-net and a class bank with learnable context rows
static int cocoop_state_check(const rlcf_engine* e, const char* entry) {
    if (e->mn_H <= 0) { rlcf_set_error("%s: no meta-net set (rlcf_engine_set_meta_net)", entry); return RLCF_ERR_STATE; }
    if (e->C <= 0 || e->image_bank || e->n_ctx <= 0) {
        rlcf_set_error("%s: needs a class bank with learnable context rows (rlcf_engine_set_class_bank, n_ctx > 0): its ctx_init is the generator's ctx", entry);
        return RLCF_ERR_STATE;
    }
    return RLCF_OK;
}
// CoCoOpCLIP.gen_ctx (cocoop.py:172-182): one student image pass; the meta-net reads the UN-normalised features — row 0 (aug) or the
// mean over the rows.  The normalised features stay in e->img_feat, the raw ones in e->cocoop_raw, the prompt in e->cocoop_ctx.
int engine_cocoop_gen_ctx(rlcf_engine* e, const float* views, int N, int aug, float* feats_raw_out, float* ctx_out, hipStream_t st) {
    TRY(cocoop_state_check(e, "rlcf_cocoop_gen_ctx"));
    ClipModel& s = e->model[RLCF_STUDENT];
    RLCF_ARG_CHECK(N > 0 && N <= e->max_views);
    const int D = s.cfg.embed_dim, Wt = s.cfg.text_width, n_ctx = e->n_ctx;
    TRY(e->cocoop_raw.ensure((size_t)e->max_views * D * sizeof(float)));
    TRY(e->cocoop_ctx.ensure((size_t)n_ctx * Wt * sizeof(float)));
    float* raw = e->cocoop_raw.as<float>();
    TRY(engine_encode_image(e, RLCF_STUDENT, views, N, e->img_feat.as<float>(), st, 0, raw));
    TRY(launch_cocoop_ctx(raw, D, aug ? 1 : N, aug ? 0 : 1, e->ctx_init.as<float>(), n_ctx, e->mn_w1.as<float>(), e->mn_b1.as<float>(),
                          e->mn_w2.as<float>(), e->mn_b2.as<float>(), D, e->mn_H, Wt, e->cocoop_ctx.as<float>(), st));
    COPY_OUT(feats_raw_out, raw, (size_t)N * D * sizeof(float));
    COPY_OUT(ctx_out, e->cocoop_ctx.p, (size_t)n_ctx * Wt * sizeof(float));
    return RLCF_OK;
}
// test_time_tuning on (image_feature, pgen_ctx) + the final call (TPT/tpt_cls.py:49-78,285-295): the prompt step from given features
int engine_tta_sample_feats(rlcf_engine* e, const float* feats_raw, int N, const rlcf_tta_args* a, const rlcf_tta_out* out, hipStream_t st) {
    return tta_sample_core(e, nullptr, feats_raw, N, a, out, st);
}
// The loop body TPT/tpt_cls.py:280-297 with args.cocoop and args.tpt: gen_ctx(aug = True), the step, the final logits — one image
// pass.  The step is tta_sample_core on the features the generator's pass left in e->img_feat: the kernels, shapes and order of
// rlcf_cocoop_gen_ctx followed by rlcf_tta_sample_feats (whose L2 normalisation of the raw rows is the image pass's own kernel on the
// same rows), so the two forms give the same bits.
int engine_tta_sample_cocoop(rlcf_engine* e, const float* views, int N, const rlcf_tta_args* a, const rlcf_tta_out* out, float* feats_raw_out,
                             float* ctx_gen_out, hipStream_t st) {
    TRY(engine_cocoop_gen_ctx(e, views, N, 1, feats_raw_out, ctx_gen_out, st));
    rlcf_tta_args b = *a;
    b.ctx_in = e->cocoop_ctx.as<float>();
    return tta_sample_core(e, nullptr, nullptr, N, &b, out, st);
}

// ------------------------------------------------------------------ B test samples per pass
// Same arithmetic per sample as engine_tta_sample (default RLCF configuration: one tuning step, sparse class backward),
// but every tower pass runs once for the whole batch: B*N views through the student image tower, B*n_sel views through
// the reward tower, B*n_sel*K class prompts through the sparse forward/backward (each sample with its own copy of the
// prompt prefix), B adapted prompts through one replicated final text pass.  Samples stay independent (no cross-sample
// arithmetic); larger M per GEMM is what fills 256 CUs.
static int batch_ensure(rlcf_engine* e, int B, hipStream_t st) {
    if (B <= e->b_cap) return RLCF_OK;
    ClipModel& s = e->model[RLCF_STUDENT];
    const TextLayout& L = e->lay[0];
    const int Wt = s.cfg.text_width, D = s.cfg.embed_dim, C = L.C;
    TRY(e->b_seqs_rep.ensure((size_t)B * L.n_seq * sizeof(rlcf_seq))); TRY(e->b_eot_rep.ensure((size_t)B * C * sizeof(int32_t)));
    TRY(launch_replicate_layout(L.seqs.as<rlcf_seq>(), L.n_seq, L.eot_rows.as<int32_t>(), C, L.T, B, e->b_seqs_rep.as<rlcf_seq>(),
                                e->b_eot_rep.as<int32_t>(), st));
    if (L.n_pk > 0) {        // packed runs: the descriptors shift like the sequences, the per-row sequence starts like row ids
        TRY(e->b_pk_rep.ensure((size_t)B * L.n_pk * sizeof(rlcf_seq))); TRY(e->b_rss_rep.ensure((size_t)B * L.T * sizeof(int32_t)));
        TRY(launch_replicate_layout(L.pk_seqs.as<rlcf_seq>(), L.n_pk, L.pk_rss.as<int32_t>(), L.T, L.T, B, e->b_pk_rep.as<rlcf_seq>(),
                                    e->b_rss_rep.as<int32_t>(), st));
    }
    const size_t cb = (size_t)B * e->n_ctx * Wt * sizeof(float);
    TRY(e->b_ctx.ensure(cb)); TRY(e->b_m.ensure(cb)); TRY(e->b_v.ensure(cb)); TRY(e->b_grad.ensure(cb));
    TRY(e->b_txt.ensure((size_t)B * C * D * sizeof(float))); TRY(e->b_u.ensure((size_t)B * C * D * sizeof(float)));
    TRY(e->b_eot_x.ensure((size_t)B * C * Wt * sizeof(float))); TRY(e->b_eot_ln.ensure((size_t)B * C * Wt * sizeof(float)));
    TRY(e->b_inv.ensure((size_t)B * C * sizeof(float))); TRY(e->b_logits.ensure((size_t)B * C * sizeof(float)));
    TRY(tower_ensure(e->tt, B * L.T, Wt, st));
    if (prec_x3(e) && (size_t)B * L.T * Wt * 4 > e->a_split_elems) {
        e->a_split_elems = (size_t)B * L.T * Wt * 4;
        TRY(e->a_hi.ensure(e->a_split_elems * 4));
    }
    RLCF_HIP_CHECK(hipStreamSynchronize(st));
    e->b_cap = B;
    return RLCF_OK;
}

// img_feat: the student image features [B*N, D] of these views — nullptr: computed here (the whole pass on one stream); else they
// were produced by the caller (tta_batch_pipelined: the tower of this part ran on the other stream) and only the rest of the pass runs
static int tta_batch_fused(rlcf_engine* e, const float* views, int B, int N, const rlcf_tta_args* a, float* final_logits, int32_t* top5,
                           hipStream_t st, const float* img_feat = nullptr) {
    ClipModel& s = e->model[RLCF_STUDENT];
    const TextLayout& L = e->lay[0];
    const int C = e->C, K = a->sample_k, D = s.cfg.embed_dim, Wt = s.cfg.text_width, n_ctx = e->n_ctx;
    const int n_sel = n_selected(a, N), n_e = n_sel * K, BN = B * N, BS = B * n_sel;
    const size_t img_elems = (size_t)3 * s.cfg.image_resolution * s.cfg.image_resolution;
    if (!img_feat) {
        TRY(batch_ensure(e, B, st));
        TRY(sparse_ensure(e, n_e, st, B));
        e->last_flops = 0.0;
        // 1. student image features of all B*N views
        TRY(engine_encode_image(e, RLCF_STUDENT, views, BN, e->img_feat.as<float>(), st));
        img_feat = e->img_feat.as<float>();
    }
    // first-step logits against the cached pristine-prompt text features
    TRY(engine_logits(e, img_feat, BN, e->txt0.as<float>(), C, e->logits.as<float>(), st));
    // 2. per-sample confidence selection (global row ids), gathers, reward features of the selected views
    TRY(launch_entropy_select_batched(e->logits.as<float>(), B, N, C, n_sel, e->entropy.as<float>(), e->sel_idx.as<int32_t>(), st));
    TRY(launch_gather_rows(img_feat, D, e->sel_idx.as<int32_t>(), e->sel_feat.as<float>(), D, BS, D, st));
    TRY(launch_gather_rows(views, (int)img_elems, e->sel_idx.as<int32_t>(), e->views_sel.as<float>(), (int)img_elems, BS, (int)img_elems, st));
    TRY(reward_encode(e, BS, s.cfg.image_resolution, nullptr, st));
    TRY(launch_gather_rows(e->logits.as<float>(), C, e->sel_idx.as<int32_t>(), e->sel_logits.as<float>(), C, BS, C, st));
    const int gT = L.pre_rows + n_e * L.lmax, T = B * gT, nE = B * n_e;
    const int64_t np = (int64_t)n_ctx * Wt;
    // reset state of every sample: ctx = ctx_init, Adam moments zero (custom_clip.py:161-164, tpt_cls_rl.py:251-255)
    TRY(launch_broadcast_rows(e->ctx_init.as<float>(), e->b_ctx.as<float>(), (int)np, B, st));
    RLCF_HIP_CHECK(hipMemsetAsync(e->b_m.p, 0, (size_t)B * np * sizeof(float), st));
    RLCF_HIP_CHECK(hipMemsetAsync(e->b_v.p, 0, (size_t)B * np * sizeof(float), st));
    TextPassIO fo{};                 // full class bank, one replica (and one prompt) per sample
    fo.seqs = e->b_seqs_rep.as<rlcf_seq>(); fo.n_seq = B * L.n_seq; fo.max_q_len = L.max_q_len; fo.T = B * L.T; fo.n_cls = B * C;
    fo.attn_pairs = (long)B * L.attn_pairs; fo.eot_rows = e->b_eot_rep.as<int32_t>(); fo.row_src = nullptr;
    fo.eot_x = e->b_eot_x.as<float>(); fo.eot_ln = e->b_eot_ln.as<float>(); fo.u = e->b_u.as<float>(); fo.inv_norm = e->b_inv.as<float>();
    fo.txt = e->b_txt.as<float>(); fo.rep_rows = L.T; fo.ctx_stride = (int)np;
    if (L.n_pk > 0) { fo.pk_seqs = e->b_pk_rep.as<rlcf_seq>(); fo.n_pk = B * L.n_pk; fo.pk_rss = e->b_rss_rep.as<int32_t>(); }
    for (int j = 0; j < a->tta_steps; ++j) {
        if (j > 0) {
            // tpt_cls_rl.py:55: logits of the selected views under each sample's current prompt
            TRY(text_forward(e, s, L, e->tt, e->b_ctx.as<float>(), fo, false, st));
            TRY(launch_group_logits(e->sel_feat.as<float>(), n_sel, e->b_txt.as<float>(), B, C, D, s.logit_scale_exp, e->sel_logits.as<float>(), st));
            e->last_flops += 2.0 * BS * C * D;
        }
        // 3. top-K sampling, CLIP reward, baseline, reward-weighted CE and dlogits, grouped per sample
        TRY(loss_step(e, a, LOSS_RL, B, n_sel, nullptr, nullptr, nullptr, st));
        // 4. sparse backward of all B*n_e sampled (view, class) pairs; each sample owns a copy of the prompt prefix
        TRY(launch_build_sparse_layout(e->topk_idx.as<int32_t>(), B, n_e, L.class_start.as<int32_t>(), L.class_len.as<int32_t>(),
                                       L.class_eot_off.as<int32_t>(), L.lmax, L.pre_rows, e->sp_seqs.as<rlcf_seq>(), e->sp_eot_rows.as<int32_t>(),
                                       e->sp_row_src.as<int32_t>(), st));
        TextPassIO io{};
        io.seqs = e->sp_seqs.as<rlcf_seq>(); io.n_seq = B * (n_e + (L.pre_rows > 0 ? 1 : 0)); io.max_q_len = L.max_q_len; io.T = T; io.n_cls = nE;
        io.attn_pairs = (long)(nE * (L.mean_len * (L.pre_rows + (L.mean_len + 1) * 0.5)));
        io.eot_rows = e->sp_eot_rows.as<int32_t>(); io.row_src = e->sp_row_src.as<int32_t>();
        io.eot_x = e->sp_eot_x.as<float>(); io.eot_ln = e->sp_eot_ln.as<float>(); io.u = e->sp_u.as<float>();
        io.inv_norm = e->sp_inv_norm.as<float>(); io.txt = e->sp_txt.as<float>();
        io.rep_rows = gT; io.ctx_stride = (int)np;                  // group b of gT rows reads prompt b
        TRY(text_forward(e, s, L, e->st, e->b_ctx.as<float>(), io, true, st));
        TRY(launch_dtxt_sparse(e->dlogits.as<float>(), e->topk_idx.as<int32_t>(), e->sel_feat.as<float>(), nE, K, C, D, s.logit_scale_exp,
                               e->sp_dtxt.as<float>(), st));
        {   // text_backward with the per-sample (grouped) ctx-gradient reduction
            TRY(launch_l2norm_bwd(io.txt, e->sp_dtxt.as<float>(), io.inv_norm, e->sp_du.as<float>(), nE, D, st));
            TRY(gemm(e, e->sp_du.as<float>(), D, s.tproj, D, nullptr, nullptr, 0, nullptr, 0, e->sp_dxe.as<float>(), Wt, nE, Wt, D, 1.f, RLCF_EPI_NONE, st));
            TRY(launch_layernorm_bwd(io.eot_x, s.lnf_w, e->sp_dxe.as<float>(), nullptr, e->sp_dxe.as<float>(), nullptr, nullptr, nE, Wt, st));
            RLCF_HIP_CHECK(hipMemsetAsync(e->dX.p, 0, (size_t)T * Wt * sizeof(float), st));
            TRY(launch_scatter_rows(e->sp_dxe.as<float>(), io.eot_rows, e->dX.as<float>(), nE, Wt, st));
            TRY(transformer_backward(e, s.txt, e->st, io.seqs, io.n_seq, L.max_keys, io.attn_pairs, 1, T, st));
            if (L.ctx_general)
                TRY(launch_ctx_grad_scan(e->dX.as<float>(), io.row_src, L.ctx_row.as<int32_t>(), B, gT, n_ctx, Wt, e->b_grad.as<float>(), st));
            else
                TRY(launch_ctx_grad_grouped(e->dX.as<float>(), e->sp_ctx_rows_list.as<int32_t>(), L.pre_rows > 0 ? 1 : n_e, n_ctx, Wt, B, gT,
                                            e->b_grad.as<float>(), st));
        }
        // 5. AdamW step j+1 of every sample (tpt_cls_rl.py:76-79)
        const OptimBuf ob{e->b_ctx.as<float>(), e->b_grad.as<float>(), e->b_m.as<float>(), e->b_v.as<float>(), np};
        TRY(optim_step(e, a, j, &ob, 1, B, nullptr, st));
    }
    // 6. final clean-view inference: B adapted prompts through one replicated text pass
    TRY(text_forward(e, s, L, e->tt, e->b_ctx.as<float>(), fo, false, st));
    float* fl = final_logits ? final_logits : e->b_logits.as<float>();
    TRY(launch_final_logits_batched(img_feat, N, e->b_txt.as<float>(), B, C, D, s.logit_scale_exp, fl, st));
    e->last_flops += 2.0 * B * C * D;
    TRY(launch_top5_batched(fl, B, C, top5, st));
    return RLCF_OK;
}

// One pass of B test images in `parts` parts on TWO streams: the student image tower of part k+1 (chip-filling GEMMs) runs on the
// caller's stream while everything behind the tower of part k — reward models' pass over the selected views, loss, sparse text
// forward / backward, AdamW, the replicated final text pass: small launch-bound kernels, ~20 % of a pass — runs on the side stream
// with the side stream's own scratch (ws_sel: A-operand buffer, split-K workspace, image-tower scratch).  Samples are independent, so
// the per-sample results are those of the one-stream pass up to the round-off of the GEMM forms the part sizes select
// (test_batch_pipeline_equals_single_stream).  MEASURED SLOWER than the one-stream pass on BASELINE configs[1] (115.7 images/s
// against 114.1 / 109.3 in 2 / 4 parts: a workgroup of the small kernels blocks a CU for the 139-KB GEMM workgroups of the tower just as
// it does alone, so the two-stream form hides nothing) — built only when RLCF_BATCH_PARTS=n asks for it.
static int tta_batch_pipelined(rlcf_engine* e, const float* views, int B, int N, int parts, const rlcf_tta_args* a, float* final_logits,
                               int32_t* top5, hipStream_t st) {
    ClipModel& s = e->model[RLCF_STUDENT];
    const int D = s.cfg.embed_dim, n_sel = n_selected(a, N), n_e = n_sel * a->sample_k;
    const size_t per = (size_t)N * 3 * s.cfg.image_resolution * s.cfg.image_resolution;
    const int Bp = (B + parts - 1) / parts;
    TRY(batch_ensure(e, Bp, st));
    TRY(sparse_ensure(e, n_e, st, Bp));
    {   // side-stream operand buffer: the text passes of a part and the reward models' patch matrices
        size_t need2 = (size_t)Bp * e->lay[0].T * s.cfg.text_width * 4;
        for (int m = 0; m < e->n_rewards; ++m) {
            const ClipModel& rm = e->model[RLCF_REWARD + m];
            need2 = std::max(need2, (size_t)Bp * n_sel * rm.tokens * std::max(rm.Kp, 4 * rm.cfg.vision_width));
        }
        if (need2 > e->a_split2_elems) { TRY(e->a_hi2.ensure(need2 * 4)); e->a_split2_elems = need2; }
    }
    for (int k = 0; k < parts && k < 8; ++k)
        if (!e->ev_part[k]) RLCF_HIP_CHECK(hipEventCreateWithFlags(&e->ev_part[k], hipEventDisableTiming));
    e->last_flops = 0.0;
    RLCF_HIP_CHECK(hipEventRecord(e->ev_fork, st));
    RLCF_HIP_CHECK(hipStreamWaitEvent(e->side, e->ev_fork, 0));
    int rc = RLCF_OK;
    for (int k = 0, b0 = 0; k < parts && b0 < B && rc == RLCF_OK; ++k, b0 += Bp) {
        const int Bk = std::min(Bp, B - b0);
        float* feat_k = e->img_feat.as<float>() + (size_t)b0 * N * D;
        rc = engine_encode_image(e, RLCF_STUDENT, views + (size_t)b0 * per, Bk * N, feat_k, st);
        if (rc != RLCF_OK) break;
        if (hipEventRecord(e->ev_part[k], st) != hipSuccess || hipStreamWaitEvent(e->side, e->ev_part[k], 0) != hipSuccess) { rc = RLCF_ERR_HIP; break; }
        e->ws_sel = 1;
        rc = tta_batch_fused(e, views + (size_t)b0 * per, Bk, N, a, final_logits ? final_logits + (size_t)b0 * e->C : nullptr, top5 + (size_t)b0 * 5,
                             e->side, feat_k);
        e->ws_sel = 0;
    }
    // the caller's stream joins the side stream whatever happened
    const hipError_t e1 = hipEventRecord(e->ev_join, e->side);
    const hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(st, e->ev_join, 0) : e1;
    if (e2 != hipSuccess) { (void)hipStreamSynchronize(e->side); if (rc == RLCF_OK) { rlcf_set_error("tta_batch_pipelined: join: %s", hipGetErrorString(e2)); rc = RLCF_ERR_HIP; } }
    return rc;
}

int engine_tta_batch(rlcf_engine* e, const float* views, int count, int N, const rlcf_tta_args* a, float* final_logits, int32_t* top5,
                     hipStream_t st) {
    ClipModel& s = e->model[RLCF_STUDENT];
    RLCF_ARG_CHECK(N > 0 && N <= e->max_views);
    const size_t per = (size_t)N * 3 * s.cfg.image_resolution * s.cfg.image_resolution;
    const int n_sel = n_selected(a, N);
    const bool sparse_ok = a->sparse_backward && (a->flags & RLCF_F_REWARD_PROCESS) && !(a->flags & RLCF_F_PROCESS_BATCH) &&
                           !(a->flags & RLCF_F_MIN_ENTROPY) && a->sample_k > 1 && loss_kind(a) == LOSS_RL;      // (RLCF_F_TPT: dense backward, sample by sample)
    const int Bmax = e->max_views / N;
    const bool fused = Bmax >= 2 && a->tta_steps >= 1 && sparse_ok && !a->ctx_in && !a->skip_final && n_sel > 0;
    double flops = 0.0;
    int i = 0;
    while (i < count) {
        const int B = fused ? std::min(Bmax, count - i) : 1;
        if (fused && B >= 2) {
            // parts of a pass on two streams (tta_batch_pipelined): needs the side stream, ViT towers everywhere (the ModifiedResNet
            // pass keeps its scratch in the engine), no per-launch profile (its event pairs serialise), one tuning step
            static int parts_env = -1;
            if (parts_env < 0) { const char* ev = getenv("RLCF_BATCH_PARTS"); parts_env = ev ? atoi(ev) : 0; }
            bool vit_all = !is_resnet(s.cfg);
            for (int m = 0; m < e->n_rewards; ++m) vit_all = vit_all && !is_resnet(e->model[RLCF_REWARD + m].cfg);
            int parts = parts_env > 0 ? parts_env : 1;          // (measured slower than one stream on BASELINE configs[1]: off unless asked for)
            parts = std::min(std::min(parts, 8), B / 2);
            if (parts >= 2 && vit_all && e->side && !g_prof.enabled && prec_x3(e)) {
                TRY(tta_batch_pipelined(e, views + (size_t)i * per, B, N, parts, a, final_logits ? final_logits + (size_t)i * e->C : nullptr,
                                        top5 + (size_t)i * 5, st));
            } else
            TRY(tta_batch_fused(e, views + (size_t)i * per, B, N, a, final_logits ? final_logits + (size_t)i * e->C : nullptr, top5 + (size_t)i * 5, st));
        } else {
            rlcf_tta_out o{};
            o.top5 = top5 + (size_t)i * 5;
            o.final_logits = final_logits ? final_logits + (size_t)i * e->C : nullptr;
            TRY(engine_tta_sample(e, views + (size_t)i * per, N, a, &o, st));
        }
        flops += e->last_flops;
        i += B;
    }
    e->last_flops = flops / count;
    return RLCF_OK;
}

// ------------------------------------------------------------------ zero-shot evaluation
// One batch of the loop TPT/zero_shot.py:139-161: model(image) of CLIPCLS_TTA (custom_clip.py:423-432, ensemble = 0) or of
// CLIPCLS_TTA_Multiple (:555-566, the student and every further slot), the rows' top-5 and the hit counts of accuracy(), as one
// enqueue: a tower pass per model (resampled where the model's resolution differs from in_res, :541-544), ONE ensemble-logits launch,
// top-5, hits.  Writes zs_* and the towers' workspace only.
int engine_zero_shot_batch(rlcf_engine* e, const float* images, int n, int in_res, int ensemble, const int64_t* target, float* logits,
                           int32_t* top5, float* hits, hipStream_t st) {
    if (e->C <= 0 || e->image_bank) { rlcf_set_error("rlcf_zero_shot_batch: class bank not set"); return RLCF_ERR_STATE; }
    if (ensemble && e->n_rewards < 1) {
        rlcf_set_error("rlcf_zero_shot_batch: ensemble asked of an engine without a further model (rlcf_engine_create_ensemble)");
        return RLCF_ERR_STATE;
    }
    const int C = e->C, M = ensemble ? 1 + e->n_rewards : 1;
    rlcf_ens_desc desc{};
    desc.M = M;
    for (int m = 0; m < M; ++m) {
        ClipModel& cm = e->model[m];
        const int D = cm.cfg.embed_dim;
        TRY(e->zs_feat[m].ensure((size_t)e->max_views * D * sizeof(float)));
        TRY(engine_encode_image(e, m, images, n, e->zs_feat[m].as<float>(), st, in_res));
        desc.m[m].img = e->zs_feat[m].as<float>(); desc.m[m].ld_img = D;
        desc.m[m].txt = m == 0 ? e->txt0.as<float>() : e->reward_cls[m - 1].as<float>(); desc.m[m].ld_txt = D;
        desc.m[m].D = D; desc.m[m].scale = cm.logit_scale_exp;
    }
    float* lg = logits;
    if (!lg) { TRY(e->zs_logits.ensure((size_t)e->max_views * C * sizeof(float))); lg = e->zs_logits.as<float>(); }
    TRY(launch_ensemble_logits(&desc, n, C, lg, C, st));
    int32_t* t5 = top5;
    if (!t5) { TRY(e->zs_top5.ensure((size_t)e->max_views * 5 * sizeof(int32_t))); t5 = e->zs_top5.as<int32_t>(); }
    if (C < 5) RLCF_HIP_CHECK(hipMemsetAsync(t5, 0xff, (size_t)n * 5 * sizeof(int32_t), st));      // top5_kernel fills min(C, 5) entries: the rest read -1
    TRY(launch_top5_batched(lg, n, C, t5, st));
    if (target) TRY(launch_top5_hits(t5, target, n, hits, st));
    return RLCF_OK;
}
