"""GPU: which tuning entry takes which loss kind with which flags — the whole matrix in one place (tta_args_check, csrc/engine_prompt.inl).
Every entry x {RL, KD, DKD, ATKD, TPT} x {RLCF_F_MIN_ENTROPY, RLCF_F_NO_SELECTION} set / unset at the tiny geometry of the tpt_tiny_* /
kd_tiny_* fixtures.  A refused call returns its status before anything is launched: the outputs keep their sentinel and the tunable
norm layers their reset state; an accepted call runs one step to a finite loss (the batched and lane entries, which hand no loss
out: finite final logits)."""
import ctypes as C

import pytest
import torch

from rlcf_amd import synth

import tpt_ref as T

pytestmark = pytest.mark.gpu

REWARD, REWARD_SEED = "tiny-r", 23
F_NO_SELECTION = 16                     # RLCF_F_NO_SELECTION (include/rlcf_hip.h)
OK, ARG = 0, -1                         # RLCF_OK, RLCF_ERR_ARG
SENTINEL = -12345.0

# a refusal: (status, a word of rlcf_last_error()); the message also names the entry
KD_ = (ARG, b"distillation")            # a distillation loss where it has no form, or with a flag it refuses
TPT_ = (ARG, b"RLCF_F_TPT")             # the TPT loss where it has no form, or with a flag it refuses
ME_ = (ARG, b"min-entropy")             # retrieval distillation with the min-entropy regulariser
DKD_ = (ARG, b"DKD")                    # retrieval distillation has kd_distill_loss_v2 only (the loss kind speaks before the flags)

# (entry, loss kind) -> the call's outcome with the extra flags (none, MIN_ENTROPY, NO_SELECTION, MIN_ENTROPY | NO_SELECTION).
# include/rlcf_hip.h: RLCF_F_KD / DKD / ATKD run on rlcf_tta_sample_ln / rlcf_tta_sample_visual; RLCF_F_TPT on the three one-image calls
# and the two batched calls, refused with RLCF_F_KD_MASK, RLCF_F_MIN_ENTROPY or RLCF_F_NO_SELECTION and by the lanes and the four
# retrieval entries; the two retrieval *_kd entries distil with KD whatever the kind field says, refuse MIN_ENTROPY, DKD and ATKD, and
# take their rows in order anyway.  The reward loss takes both extra flags everywhere.
EXPECT = {
    ("rlcf_tta_sample", "RL"): (OK, OK, OK, OK),
    ("rlcf_tta_sample", "KD"): (KD_, KD_, KD_, KD_),
    ("rlcf_tta_sample", "DKD"): (KD_, KD_, KD_, KD_),
    ("rlcf_tta_sample", "ATKD"): (KD_, KD_, KD_, KD_),
    ("rlcf_tta_sample", "TPT"): (OK, TPT_, TPT_, TPT_),
    ("rlcf_tta_sample_ln", "RL"): (OK, OK, OK, OK),
    ("rlcf_tta_sample_ln", "KD"): (OK, KD_, KD_, KD_),
    ("rlcf_tta_sample_ln", "DKD"): (OK, KD_, KD_, KD_),
    ("rlcf_tta_sample_ln", "ATKD"): (OK, KD_, KD_, KD_),
    ("rlcf_tta_sample_ln", "TPT"): (OK, TPT_, TPT_, TPT_),
    ("rlcf_tta_sample_visual", "RL"): (OK, OK, OK, OK),
    ("rlcf_tta_sample_visual", "KD"): (OK, KD_, KD_, KD_),
    ("rlcf_tta_sample_visual", "DKD"): (OK, KD_, KD_, KD_),
    ("rlcf_tta_sample_visual", "ATKD"): (OK, KD_, KD_, KD_),
    ("rlcf_tta_sample_visual", "TPT"): (OK, TPT_, TPT_, TPT_),
    ("rlcf_tta_batch", "RL"): (OK, OK, OK, OK),
    ("rlcf_tta_batch", "KD"): (KD_, KD_, KD_, KD_),
    ("rlcf_tta_batch", "DKD"): (KD_, KD_, KD_, KD_),
    ("rlcf_tta_batch", "ATKD"): (KD_, KD_, KD_, KD_),
    ("rlcf_tta_batch", "TPT"): (OK, TPT_, TPT_, TPT_),
    ("rlcf_tta_batch_ln", "RL"): (OK, OK, OK, OK),
    ("rlcf_tta_batch_ln", "KD"): (KD_, KD_, KD_, KD_),
    ("rlcf_tta_batch_ln", "DKD"): (KD_, KD_, KD_, KD_),
    ("rlcf_tta_batch_ln", "ATKD"): (KD_, KD_, KD_, KD_),
    ("rlcf_tta_batch_ln", "TPT"): (OK, TPT_, TPT_, TPT_),
    ("rlcf_tta_retrieval_image", "RL"): (OK, OK, OK, OK),
    ("rlcf_tta_retrieval_image", "KD"): (KD_, KD_, KD_, KD_),
    ("rlcf_tta_retrieval_image", "DKD"): (KD_, KD_, KD_, KD_),
    ("rlcf_tta_retrieval_image", "ATKD"): (KD_, KD_, KD_, KD_),
    ("rlcf_tta_retrieval_image", "TPT"): (TPT_, TPT_, TPT_, TPT_),
    ("rlcf_tta_retrieval_text", "RL"): (OK, OK, OK, OK),
    ("rlcf_tta_retrieval_text", "KD"): (KD_, KD_, KD_, KD_),
    ("rlcf_tta_retrieval_text", "DKD"): (KD_, KD_, KD_, KD_),
    ("rlcf_tta_retrieval_text", "ATKD"): (KD_, KD_, KD_, KD_),
    ("rlcf_tta_retrieval_text", "TPT"): (TPT_, TPT_, TPT_, TPT_),
    ("rlcf_tta_retrieval_image_kd", "RL"): (OK, ME_, OK, ME_),
    ("rlcf_tta_retrieval_image_kd", "KD"): (OK, ME_, OK, ME_),
    ("rlcf_tta_retrieval_image_kd", "DKD"): (DKD_, DKD_, DKD_, DKD_),
    ("rlcf_tta_retrieval_image_kd", "ATKD"): (DKD_, DKD_, DKD_, DKD_),
    ("rlcf_tta_retrieval_image_kd", "TPT"): (TPT_, TPT_, TPT_, TPT_),
    ("rlcf_tta_retrieval_text_kd", "RL"): (OK, ME_, OK, ME_),
    ("rlcf_tta_retrieval_text_kd", "KD"): (OK, ME_, OK, ME_),
    ("rlcf_tta_retrieval_text_kd", "DKD"): (DKD_, DKD_, DKD_, DKD_),
    ("rlcf_tta_retrieval_text_kd", "ATKD"): (DKD_, DKD_, DKD_, DKD_),
    ("rlcf_tta_retrieval_text_kd", "TPT"): (TPT_, TPT_, TPT_, TPT_),
    ("rlcf_lanes_submit", "RL"): (OK, OK, OK, OK),
    ("rlcf_lanes_submit", "KD"): (KD_, KD_, KD_, KD_),
    ("rlcf_lanes_submit", "DKD"): (KD_, KD_, KD_, KD_),
    ("rlcf_lanes_submit", "ATKD"): (KD_, KD_, KD_, KD_),
    ("rlcf_lanes_submit", "TPT"): (TPT_, TPT_, TPT_, TPT_),
}
ENTRIES = sorted({e for e, _ in EXPECT}, key=[e for e, _ in EXPECT].index)
TEXT_ENTRIES = ("rlcf_tta_retrieval_text", "rlcf_tta_retrieval_text_kd")        # a query caption over an image bank
BATCHED = ("rlcf_tta_batch", "rlcf_tta_batch_ln", "rlcf_lanes_submit")          # (final logits, top-5) out, no loss


def st():
    return torch.cuda.current_stream().cuda_stream


class _Rig:
    """two tiny engines (class bank with learnable context; image bank), the inputs, and one sentinel-filled row per output field"""

    def __init__(self, L, dev):
        from rlcf_amd.engine import Engine, TTAConfig
        _, meta = T.load_golden("tpt_tiny_vis_s1")
        self.L, self.lib, self.meta = L, L.lib(), meta
        sg, rg = synth.GEOMETRIES[meta["student"]], synth.GEOMETRIES[REWARD]
        ssd, rsd = synth.make_state_dict(sg, meta["student_seed"], device=dev), synth.make_state_dict(rg, REWARD_SEED, device=dev)
        self.N, self.n_cls = meta["n_views"], meta["n_cls"]
        self.views = synth.make_views(meta["view_seed"], self.N, sg.image_resolution, device=dev)
        self.engines = []
        for _ in range(2):
            eng = Engine(sg, rg, self.N, self.n_cls, 2)
            eng.load_state_dict(L.STUDENT, ssd)
            eng.load_state_dict(L.REWARD, rsd)
            eng.finalize()
            self.engines.append(eng)
        self.cls, self.img = self.engines
        tokens = synth.make_token_bank(sg, self.n_cls, seed=meta["bank_seed"], n_ctx=meta["n_ctx"])
        ctx0 = ssd["token_embedding.weight"][torch.tensor(synth.ctx_token_ids_default(sg, meta["n_ctx"]), device=dev)].clone()
        self.cls.set_class_bank(tokens, meta["n_ctx"], ctx0, L.TEXT_SHARED)
        self.img.set_image_bank(self.img.encode_image(L.STUDENT, self.views), self.img.encode_image(L.REWARD, self.views))
        self.query = tokens[3].to("cpu", torch.int32).contiguous()
        self.cfg = TTAConfig(selection_p=meta["selection_p"], tta_steps=1, lr=meta["lr"], weight_decay=meta["weight_decay"])
        n_vis = int(self.lib.rlcf_engine_visual_param_count(self.cls.h, st()))
        n_txt = int(self.lib.rlcf_engine_text_param_count(self.img.h, None, st()))
        assert n_vis > 0 and n_txt > 0
        width = max(n_vis, n_txt, self.N * self.n_cls, self.N * rg.embed_dim, int(self.lib.rlcf_engine_ln_param_count(self.cls.h)))
        self.pristine = torch.full((len(L.TTA_OUT_FIELDS), width), SENTINEL, device=dev)
        self.arena = self.pristine.clone()
        self.row = {f: self.arena[i] for i, f in enumerate(L.TTA_OUT_FIELDS)}
        self.out = L.TTAOut(**{f: self.row[f].data_ptr() for f in L.TTA_OUT_FIELDS})
        self.kind_flag = {"RL": 0, "KD": L.F_KD, "DKD": L.F_DKD, "ATKD": L.F_ATKD, "TPT": L.F_TPT}

    def call(self, entry, lanes, flags):
        """the entry's status with these flags, on the engine that holds the bank it needs"""
        lib, out = self.lib, C.byref(self.out)
        eng = self.img if entry in TEXT_ENTRIES else self.cls
        a = self.cfg.c_args(1 if entry in TEXT_ENTRIES else self.N)
        a.flags = self.L.F_REWARD_PROCESS | flags
        v, N, fl, top5 = self.views.data_ptr(), self.N, self.row["final_logits"].data_ptr(), self.row["top5"].data_ptr()
        if entry in ("rlcf_tta_sample", "rlcf_tta_sample_ln", "rlcf_tta_sample_visual", "rlcf_tta_retrieval_image"):
            return eng, getattr(lib, entry)(eng.h, v, N, C.byref(a), out, st())
        if entry == "rlcf_tta_retrieval_image_kd":
            return eng, lib.rlcf_tta_retrieval_image_kd(eng.h, v, N, C.byref(a), None, out, st())
        if entry == "rlcf_tta_retrieval_text":
            return eng, lib.rlcf_tta_retrieval_text(eng.h, self.query.data_ptr(), C.byref(a), out, st())
        if entry == "rlcf_tta_retrieval_text_kd":
            return eng, lib.rlcf_tta_retrieval_text_kd(eng.h, self.query.data_ptr(), C.byref(a), None, out, st())
        if entry == "rlcf_lanes_submit":
            rc = lib.rlcf_lanes_submit(lanes, v, 1, N, C.byref(a), fl, top5, 0, st())
            if rc >= 0:
                assert lib.rlcf_lanes_join(lanes, st()) == 0
            return eng, min(rc, 0)                  # (an accepted submit returns its lane's index)
        return eng, getattr(lib, entry)(eng.h, v, 1, N, C.byref(a), fl, top5, st())

    def close(self):
        for eng in self.engines:
            eng.close()


@pytest.fixture(scope="module")
def rig():
    from rlcf_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    r = _Rig(_lib, torch.device("cuda:0"))
    yield r
    r.close()


def test_table_covers_every_entry_and_loss_kind():
    assert len(ENTRIES) == 10 and len(EXPECT) == 10 * 5
    assert all((e, k) in EXPECT and len(EXPECT[e, k]) == 4 for e in ENTRIES for k in ("RL", "KD", "DKD", "ATKD", "TPT"))


@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_takes_and_refuses_what_the_table_says(rig, entry):
    lib, L = rig.lib, rig.L
    lanes = None
    if entry == "rlcf_lanes_submit":
        lanes = lib.rlcf_lanes_create((C.c_void_p * 1)(rig.cls.h), 1)
        assert lanes
    wrong = []
    try:
        for kind in ("RL", "KD", "DKD", "ATKD", "TPT"):
            for extra, want in zip((0, L.F_MIN_ENTROPY, F_NO_SELECTION, L.F_MIN_ENTROPY | F_NO_SELECTION), EXPECT[entry, kind]):
                case = f"{entry} {kind} +0x{extra:x}"
                eng, rc = rig.call(entry, lanes, rig.kind_flag[kind] | extra)
                torch.cuda.synchronize()
                if want == OK:
                    got = rig.row["final_logits" if entry in BATCHED else "loss"][: rig.n_cls if entry in BATCHED else 1]
                    print(f"{case}: status {rc}, {'final logits' if entry in BATCHED else 'loss'} {got.flatten()[:4].tolist()}")
                    if rc != OK:
                        wrong.append(f"{case}: status {rc} ({lib.rlcf_last_error().decode()}), expected RLCF_OK")
                    elif not (torch.isfinite(got).all() and (got != SENTINEL).all()):
                        wrong.append(f"{case}: accepted, but no finite result was written: {got.tolist()}")
                    rig.arena.copy_(rig.pristine)
                    continue
                status, word = want
                msg = lib.rlcf_last_error()
                print(f"{case}: status {rc}: {msg.decode()}")
                if rc != status or word not in msg or entry.encode() not in msg:
                    wrong.append(f"{case}: status {rc} ({msg.decode()}), expected {status} naming {word.decode()!r} and the entry")
                if not torch.equal(rig.arena, rig.pristine):
                    wrong.append(f"{case}: a refused call wrote to its outputs")
                    rig.arena.copy_(rig.pristine)
                if not torch.equal(eng.ln_params(), eng.ln_params(pristine=True)):
                    wrong.append(f"{case}: a refused call moved the tunable norm layers")
    finally:
        if lanes:
            lib.rlcf_lanes_destroy(lanes)
    assert not wrong, "\n".join(wrong)
