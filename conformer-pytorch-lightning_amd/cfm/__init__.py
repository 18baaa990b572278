"""cfm -- ctypes binding of libconformer_gfx950.so (the C ABI declared in include/cfm.h).

This is plumbing only: it turns torch tensors that already live on an MI355X into raw device
pointers + sizes, passes the current HIP stream, and converts negative status codes into
``RuntimeError`` carrying ``cfm_last_error()``.  There is NO CPU fallback and no other backend: if the
shared library is missing, or a tensor is not on a HIP device, every entry point raises.
"""
import ctypes
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "libconformer_gfx950.so")

F32, BF16, F16 = 0, 1, 2
ACT_NONE, ACT_SILU, ACT_RELU, ACT_GLU, ACT_DSILU, ACT_DRELU = 0, 1, 2, 3, 4, 5
TILE_AUTO_TRAIN = -1            # cfm_gemm_desc.tile: automatic choice with the K-group tiles allowed (training paths; cfm.h)

_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}
_TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}

c_p = ctypes.c_void_p
c_i64 = ctypes.c_int64
c_i32 = ctypes.c_int32
c_int = ctypes.c_int
c_f = ctypes.c_float
P = ctypes.POINTER


class GemmDesc(ctypes.Structure):
    _fields_ = [("A", c_p), ("W", c_p), ("W_lo", c_p), ("bias", c_p), ("residual", c_p), ("row_mask", c_p), ("C", c_p),
                ("lda", c_i64), ("ldc", c_i64), ("ldr", c_i64),
                ("M", c_i32), ("N", c_i32), ("K", c_i32),
                ("a_dtype", c_i32), ("w_dtype", c_i32), ("c_dtype", c_i32),
                ("act", c_i32), ("alpha", ctypes.c_float),
                ("conv_C", c_i32), ("conv_T1", c_i32), ("conv_F1", c_i32), ("conv_T2", c_i32), ("conv_F2", c_i32),
                ("tile", c_i32), ("mask_mode", c_i32),
                ("C_pre", c_p), ("ld_pre", c_i64), ("pre_dtype", c_i32), ("aux_dtype", c_i32), ("aux", c_p), ("ld_aux", c_i64),
                ("drop_p", ctypes.c_float), ("drop2_p", ctypes.c_float), ("drop_seed", ctypes.c_uint32), ("drop2_seed", ctypes.c_uint32),
                ("row_len", c_p), ("row_T", c_i32)]


class GemmTnDesc(ctypes.Structure):
    _fields_ = [("A", c_p), ("B", c_p), ("C", c_p), ("colsum", c_p), ("row_mask", c_p),
                ("lda", c_i64), ("ldb", c_i64), ("ldc", c_i64), ("M", c_i32), ("N", c_i32), ("K", c_i32),
                ("a_dtype", c_i32), ("b_dtype", c_i32), ("mma_dtype", c_i32), ("split", c_i32), ("accumulate", c_i32), ("splits", c_i32),
                ("alpha", ctypes.c_float),
                ("conv_C", c_i32), ("conv_T1", c_i32), ("conv_F1", c_i32), ("conv_T2", c_i32), ("conv_F2", c_i32),
                ("row_off", c_p), ("colsum_off", c_p), ("tile", c_i32), ("colsum_off2", c_p)]


class AttnBwdDesc(ctypes.Structure):
    _fields_ = [("q", c_p), ("k", c_p), ("v", c_p), ("mask", c_p), ("out", c_p), ("dout", c_p), ("lse", c_p),
                ("grad_q", c_p), ("grad_k", c_p), ("grad_v", c_p), ("delta", c_p),
                ("q_sb", c_i64), ("q_st", c_i64), ("k_sb", c_i64), ("k_st", c_i64), ("v_sb", c_i64), ("v_st", c_i64), ("m_sb", c_i64), ("m_sq", c_i64),
                ("B", c_i32), ("H", c_i32), ("Tq", c_i32), ("Tk", c_i32), ("dk", c_i32),
                ("io_dtype", c_i32), ("dout_dtype", c_i32), ("mma_dtype", c_i32), ("split", c_i32), ("scale", ctypes.c_float),
                ("drop_p", ctypes.c_float), ("drop_seed", ctypes.c_uint32)]


class AttnDesc(ctypes.Structure):
    _fields_ = [("q", c_p), ("k", c_p), ("v", c_p), ("p", c_p), ("bias_u", c_p), ("bias_v", c_p), ("mask", c_p), ("out", c_p),
                ("q_sb", c_i64), ("q_st", c_i64), ("k_sb", c_i64), ("k_st", c_i64), ("k_sh", c_i64),
                ("v_sb", c_i64), ("v_st", c_i64), ("v_sh", c_i64), ("p_sb", c_i64), ("p_st", c_i64),
                ("m_sb", c_i64), ("m_sq", c_i64),
                ("B", c_i32), ("H", c_i32), ("Tq", c_i32), ("Tk", c_i32), ("dk", c_i32),
                ("q_dtype", c_i32), ("kv_dtype", c_i32), ("p_dtype", c_i32), ("out_dtype", c_i32), ("mma_dtype", c_i32),
                ("split", c_i32), ("scale", ctypes.c_float), ("lse", c_p), ("drop_p", ctypes.c_float), ("drop_seed", ctypes.c_uint32)]


class FfnDesc(ctypes.Structure):
    _fields_ = [("x", c_p), ("ln_g", c_p), ("ln_b", c_p), ("w1f", c_p), ("w2f", c_p), ("b1", c_p), ("b2", c_p),
                ("ln1_g", c_p), ("ln1_b", c_p), ("ln2_g", c_p), ("ln2_b", c_p), ("out_f32", c_p), ("out16", c_p),
                ("M", c_i64), ("D", c_i32), ("FF", c_i32), ("w_dtype", c_i32), ("out16_dtype", c_i32), ("act", c_i32),
                ("add_x", c_i32), ("alpha", ctypes.c_float), ("eps", ctypes.c_float)]


class RowChainDesc(ctypes.Structure):
    _fields_ = [("x", c_p), ("head_a", c_p), ("head_w", c_p), ("head_b", c_p), ("head_res", c_p), ("head_mask", c_p),
                ("ln_g", c_p), ("ln_b", c_p), ("ln_mask", c_p), ("w1f", c_p), ("w2n", c_p), ("b1", c_p), ("b2", c_p),
                ("ln1_g", c_p), ("ln1_b", c_p), ("ln2_g", c_p), ("ln2_b", c_p), ("out_f32", c_p), ("out16", c_p),
                ("tail_w", c_p), ("tail_b", c_p), ("tail_out", c_p), ("M", c_i64), ("D", c_i32), ("FF", c_i32),
                ("tail_N", c_i32), ("tail_glu", c_i32), ("w_dtype", c_i32), ("alpha", ctypes.c_float), ("eps", ctypes.c_float),
                ("out2_f32", c_p), ("dw_w", c_p), ("dw_b", c_p), ("dw_scale", c_p), ("dw_shift", c_p), ("dw_T", c_i32), ("dw_K", c_i32),
                ("s2_ln_g", c_p), ("s2_ln_b", c_p), ("s2_w1f", c_p), ("s2_w2n", c_p), ("s2_b1", c_p), ("s2_b2", c_p), ("s2_out_f32", c_p),
                ("s2_alpha", ctypes.c_float), ("psum_out", c_p), ("psum_in", c_p), ("psum_b2", c_p), ("psum_alpha", ctypes.c_float),
                ("cin_a", c_p), ("cin_w", c_p), ("cin_b", c_p), ("cin_res", c_p), ("cin_out", c_p), ("cin_ln_g", c_p), ("cin_ln_b", c_p), ("cin_mask", c_p),
                ("cin_tail_w", c_p), ("cin_tail_b", c_p), ("tail_pair", c_i32), ("glu_len", c_p), ("glu_T", c_i32)]


_LAYER_W_FIELDS = [
    "ln_ffm_g", "ln_ffm_b", "ln_mha_g", "ln_mha_b", "ln_conv_g", "ln_conv_b", "ln_ff_g", "ln_ff_b", "ln_final_g", "ln_final_b",
    "ffm_w1", "ffm_w1_lo", "ffm_w2", "ffm_w2_lo", "ffm_b1", "ffm_b2",
    "ff_w1", "ff_w1_lo", "ff_w2", "ff_w2_lo", "ff_b1", "ff_b2", "ffm_w1f", "ffm_w2f", "ff_w1f", "ff_w2f", "ffm_w2n", "ff_w2n", "qkv_wf", "out_wf", "pw1_wf", "pw2_wf",
    "qkv_w", "qkv_w_lo", "pos_w", "pos_w_lo", "out_w", "out_w_lo", "qkv_b", "out_b", "bias_u", "bias_v",
    "pw1_w", "pw1_w_lo", "pw2_w", "pw2_w_lo", "pw1_b", "pw2_b", "dw_w", "dw_b", "bn_scale", "bn_shift"]


_TRAIN_W_PTRS = ["ln_ffm_g", "ln_ffm_b", "ln_mha_g", "ln_mha_b", "ln_conv_g", "ln_conv_b", "ln_ff_g", "ln_ff_b", "ln_final_g", "ln_final_b",
                 "ffm_w1", "ffm_w1_lo", "ffm_w2", "ffm_w2_lo", "ffm_w1t", "ffm_w1t_lo", "ffm_w2t", "ffm_w2t_lo", "ffm_b1", "ffm_b2",
                 "ff_w1", "ff_w1_lo", "ff_w2", "ff_w2_lo", "ff_w1t", "ff_w1t_lo", "ff_w2t", "ff_w2t_lo", "ff_b1", "ff_b2",
                 "qkv_w", "qkv_w_lo", "qkv_t", "qkv_t_lo", "out_w", "out_w_lo", "out_t", "out_t_lo", "qkv_b", "out_b",
                 "pw1_w", "pw1_w_lo", "pw1_t", "pw1_t_lo", "pw2_w", "pw2_w_lo", "pw2_t", "pw2_t_lo", "pw1_b", "pw2_b", "dw_w", "dw_b", "bn_gamma", "bn_beta",
                 "bn_running_mean", "bn_running_var"]


class LayerTrainWeights(ctypes.Structure):
    _fields_ = [(n, c_p) for n in _TRAIN_W_PTRS] + [("bn_momentum", ctypes.c_float), ("bn_eps", ctypes.c_float)]


class TrainGroup(ctypes.Structure):
    _fields_ = [("B", c_i32), ("T", c_i32), ("row0", c_i64), ("attn_mask", c_p), ("am_sb", c_i64), ("am_sq", c_i64)]


LAYER_DONE_FN = ctypes.CFUNCTYPE(None, c_i32, c_p)


class LayerTrainIO(ctypes.Structure):
    _fields_ = [("D", c_i32), ("H", c_i32), ("FF", c_i32), ("ktaps", c_i32), ("act_dtype", c_i32), ("w_dtype", c_i32), ("pad_valid", c_p),
                ("p_hidden_m", ctypes.c_float), ("p_hidden", ctypes.c_float), ("p_branch", ctypes.c_float), ("p_attn", ctypes.c_float),
                ("p_attn_out", ctypes.c_float), ("seed", ctypes.c_uint32), ("deterministic", c_i32), ("grads_accumulate", c_i32),
                ("n_groups", c_i32), ("groups", ctypes.POINTER(TrainGroup)), ("defer_wgrad", c_i32)]


_TRAIN_SAVED = ["xn1", "z1", "h1", "xn2", "qkv", "ctx", "xn3", "u", "glu", "s", "xn4", "z2", "h2", "x1", "x2", "x3", "x4", "c", "lse", "stats"]
_TRAIN_SCRATCH = ["dxn", "dz", "dyb", "ds", "dglu", "du", "dctx", "dqkv", "delta", "ln_ws", "dwbn_ws", "dy_ws", "dz2", "dyb2", "dyb3", "dyb4"]
_TRAIN_GRADS = ["slab", "ln_ffm_g", "ln_ffm_b", "ln_mha_g", "ln_mha_b", "ln_conv_g", "ln_conv_b", "ln_ff_g", "ln_ff_b", "ln_final_g", "ln_final_b",
                "ffm_w1", "ffm_b1", "ffm_w2", "ffm_b2", "ff_w1", "ff_b1", "ff_w2", "ff_b2", "out_w", "out_b", "pw2_w", "pw2_b", "dw_w", "dw_b", "bn_g", "bn_b",
                "pos_bias_u", "q_bias", "qkv_row_off", "qkv_bias_off", "pw1_row_off", "pw1_bias_off", "qkv_bias_off2"]


class LayerTrainSaved(ctypes.Structure):
    _fields_ = [(n, c_p) for n in _TRAIN_SAVED]


class LayerTrainScratch(ctypes.Structure):
    _fields_ = [(n, c_p) for n in _TRAIN_SCRATCH]


class LayerTrainGrads(ctypes.Structure):
    _fields_ = [(n, c_p) for n in _TRAIN_GRADS]


class LayerWeights(ctypes.Structure):
    _fields_ = [(n, c_p) for n in _LAYER_W_FIELDS]


class CtcGroup(ctypes.Structure):
    _fields_ = [("logits", c_p), ("ld", c_i64), ("B", c_i32), ("T", c_i32), ("Umax", c_i32), ("enc_lens", c_p), ("labels", c_p), ("label_lens", c_p),
                ("work", c_p), ("alpha", c_p), ("lse", c_p), ("nll", c_p), ("nll_shifted", c_p), ("beta", c_p)]


class RnntDesc(ctypes.Structure):
    _fields_ = [("logits", c_p), ("ld", c_i64), ("logits_dtype", c_i32), ("B", c_i32), ("T", c_i32), ("U1", c_i32), ("V", c_i32), ("blank", c_i32),
                ("targets", c_p), ("logit_lens", c_p), ("target_lens", c_p),
                ("lse", c_p), ("lp_blank", c_p), ("lp_label", c_p), ("alpha", c_p), ("beta", c_p), ("shift", c_p),
                ("nll", c_p), ("nll_shifted", c_p), ("ll_alpha", c_p),
                ("grad", c_p), ("ld_grad", c_i64), ("grad_dtype", c_i32), ("grad_cols", c_i32), ("gscale", ctypes.c_float),
                ("gscale_stride", c_i32), ("gscale_dev", c_p), ("clamp", ctypes.c_float)]


class Lattice(ctypes.Structure):
    _fields_ = [("B", c_i32), ("T_max", c_i32), ("U1_max", c_i32), ("M", c_i64), ("off", c_p), ("T", c_p), ("U", c_p), ("enc_row0", c_p),
                ("pred_row0", c_p), ("n_enc", c_i64), ("n_pred", c_i64), ("blk_off", c_p)]


class RnntPackedDesc(ctypes.Structure):
    _fields_ = [("lat", Lattice), ("logits", c_p), ("ld", c_i64), ("logits_dtype", c_i32), ("V", c_i32), ("blank", c_i32), ("ld_targets", c_i32),
                ("targets", c_p), ("lse", c_p), ("lp_blank", c_p), ("lp_label", c_p), ("alpha", c_p), ("beta", c_p), ("shift", c_p),
                ("nll", c_p), ("nll_shifted", c_p), ("ll_alpha", c_p),
                ("grad", c_p), ("ld_grad", c_i64), ("grad_dtype", c_i32), ("grad_cols", c_i32), ("gscale", ctypes.c_float),
                ("gscale_stride", c_i32), ("gscale_dev", c_p), ("clamp", ctypes.c_float)]


_ALIGN_OUT = [("frame", c_p), ("token_logp", c_p), ("score", c_p), ("scratch", c_p), ("scratch_bytes", c_i64)]


class RnntAlignDesc(ctypes.Structure):
    _fields_ = [("r", RnntDesc)] + _ALIGN_OUT


class RnntPackedAlignDesc(ctypes.Structure):
    _fields_ = [("r", RnntPackedDesc)] + _ALIGN_OUT


class LnBwdDesc(ctypes.Structure):
    _fields_ = [("x", c_p), ("dy", c_p), ("gamma", c_p), ("row_mask", c_p), ("dres", c_p), ("dx", c_p), ("dgamma", c_p), ("dbeta", c_p), ("ws", c_p),
                ("dx2", c_p), ("M", c_i64), ("D", c_i32), ("dy_dtype", c_i32), ("dx2_dtype", c_i32), ("accumulate", c_i32),
                ("eps", ctypes.c_float), ("alpha2", ctypes.c_float), ("p1", ctypes.c_float), ("p2", ctypes.c_float),
                ("seed1", ctypes.c_uint32), ("seed2", ctypes.c_uint32), ("dx2_row_mask", c_p),
                ("chain_x", c_p), ("chain_gamma", c_p), ("chain_dgamma", c_p), ("chain_dbeta", c_p)]


class LstmDesc(ctypes.Structure):
    _c_fields_ = {"in_": "in"}              # Python field -> C member, where `in` cannot be spelled
    _fields_ = [("B", c_i32), ("U", c_i32), ("in_", c_i32), ("H", c_i32), ("layers", c_i32), ("drop_p", c_f), ("seed", ctypes.c_uint32), ("x", c_p),
                ("w_ih", c_p * 4), ("w_hh", c_p * 4), ("b_ih", c_p * 4), ("b_hh", c_p * 4), ("h0", c_p), ("c0", c_p), ("y", c_p), ("hn", c_p), ("cn", c_p),
                ("save", c_p * 4), ("dy", c_p), ("dhn", c_p), ("dcn", c_p), ("dx", c_p), ("dw_ih", c_p * 4), ("dw_hh", c_p * 4), ("db_ih", c_p * 4),
                ("db_hh", c_p * 4), ("dh0", c_p), ("dc0", c_p), ("dg", c_p), ("dyl", c_p)]


class GreedyDesc(ctypes.Structure):
    _fields_ = [("embed", c_p), ("lstm_w", c_p * 4), ("lstm_b", c_p * 4), ("proj_w", c_p), ("proj_b", c_p), ("pf_w", c_p), ("pf_b", c_p), ("out_w", c_p),
                ("out_b", c_p), ("enc_proj", c_p), ("token", c_p), ("t", c_p), ("count", c_p), ("frame_count", c_p), ("hyps", c_p), ("lens", c_p),
                ("h", c_p), ("c", c_p), ("h_new", c_p), ("c_new", c_p), ("pred", c_p), ("act", c_p), ("pmax", c_p), ("pidx", c_p), ("done", c_p),
                ("n_done", c_p), ("hyp_cap", c_i64), ("hyp_ld", c_i64), ("B", c_i32), ("T", c_i32), ("L", c_i32), ("E", c_i32), ("H", c_i32),
                ("P", c_i32), ("J", c_i32), ("Vp", c_i32), ("blank", c_i32), ("n_steps", c_i32)]


class GreedyChunkDesc(ctypes.Structure):
    _fields_ = ([("embed", c_p), ("lstm_w", c_p * 4), ("lstm_b", c_p * 4)] +
                [(n, c_p) for n in ("proj_w", "proj_b", "pf_w", "pf_b", "out_w", "out_b", "ef_w", "ef_b", "enc", "enc_proj", "token", "t", "count", "frame_count",
                                    "hyps", "lens", "h", "c", "h_new", "c_new", "pred", "pp", "act", "pmax", "pidx", "rows", "row_off", "row_cnt", "n_rows",
                                    "steps", "overflow", "done", "n_done")] +
                [("hyp_cap", c_i64), ("hyp_ld", c_i64)] +
                [(n, c_i32) for n in ("B", "chunk", "L", "E", "H", "P", "J", "D", "Vp", "blank", "n_steps", "carry")])


class CtcGreedyDesc(ctypes.Structure):
    _fields_ = ([("idx", c_p), ("logp", c_p), ("ld_k", c_i64)] + [(n, c_p) for n in ("lens", "prev", "frame_base", "hyps", "count", "frames", "token_logp", "overflow")] +
                [("hyp_cap", c_i64), ("hyp_ld", c_i64)] + [(n, c_i32) for n in ("B", "T", "V", "blank")])


class CtcBeamDesc(ctypes.Structure):
    _fields_ = ([(n, c_p) for n in ("idx", "logp", "lens", "nodes")] + [("n_nodes", c_i64)] + [(n, c_p) for n in ("nbest_tokens", "nbest_len", "nbest_score")] +
                [(n, c_i32) for n in ("B", "T", "V", "k", "beam", "blank")])


class CtcAlignDesc(ctypes.Structure):
    _fields_ = ([("logits", c_p), ("ld", c_i64)] + [(n, c_p) for n in ("enc_lens", "labels", "label_lens", "work", "scratch")] + [("scratch_bytes", c_i64)] +
                [(n, c_p) for n in ("path", "score", "start", "end", "token_logp")] + [(n, c_i32) for n in ("B", "T", "V", "Umax")])


class EditDistanceDesc(ctypes.Structure):
    _fields_ = ([(n, c_p) for n in ("hyp", "hyp_lens", "ref", "ref_lens", "ref_index", "dist", "counts", "ops", "ops_len", "scratch")] + [("scratch_bytes", c_i64)] +
                [(n, c_i32) for n in ("P", "R", "Hmax", "Umax")])


class RnntBeamDesc(ctypes.Structure):
    _fields_ = ([("embed", c_p), ("lstm_w", c_p * 4), ("lstm_b", c_p * 4)] +
                [(n, c_p) for n in ("proj_w", "proj_b", "pf_w", "pf_b", "out_w", "out_b", "enc_proj", "lens", "token", "t", "hash", "fc", "len", "node", "parent", "ext",
                                    "live", "score", "h", "c", "h_new", "c_new", "pred", "act", "logits", "topk_idx", "topk_logp", "lse", "nodes")] +
                [("n_nodes", c_i64)] +
                [(n, c_p) for n in ("fin_score", "fin_node", "fin_len", "n_fin", "step", "done", "n_done", "nbest_tokens", "nbest_len", "nbest_score")] +
                [(n, c_i32) for n in ("B", "T", "L", "E", "H", "P", "J", "V", "Vp", "beam", "blank", "max_symbols", "max_len", "len_by_frames", "parity")])


class RnntBeamStreamDesc(ctypes.Structure):
    _fields_ = ([("beam", RnntBeamDesc)] +
                [(n, c_p) for n in ("enc", "ef_w", "ef_b", "chunk_proj", "avail", "final", "paused", "feed_final", "overflow", "best_tokens", "best_len", "stable_len",
                                    "best_score")] +
                [(n, c_i32) for n in ("chunk", "D")])


class FbankDesc(ctypes.Structure):
    _fields_ = ([(n, c_p) for n in ("samples", "lengths", "feats_length", "carry_in", "carry_out", "fresh_in", "pos_in", "fresh_out", "pos_out", "twiddle", "window",
                                    "mel_w", "mel_start", "mel_len", "mel_off", "out")] + [("ld", c_i64)] +
                [(n, c_i32) for n in ("B", "n_cols", "rows", "F", "win", "shift", "padded", "mel_nnz", "samples_i16", "carry_n", "hop")] +
                [("dither", c_f), ("seed", ctypes.c_uint32)] +
                [(n, c_p) for n in ("n_new", "final", "carry_len_in", "carry_len_out", "frame_lens")] + [("carry_cap", c_i32)])


class ResampleDesc(ctypes.Structure):
    _fields_ = ([(n, c_p) for n in ("samples", "lengths", "taps", "tap_first", "tap_off", "out", "out_lens")] + [("ld", c_i64), ("ld_out", c_i64)] +
                [(n, c_i32) for n in ("B", "n_cols", "cap", "samples_i16", "o", "n", "width", "n_live")] +
                [(n, c_p) for n in ("n_new", "final", "tail_in", "tail_out", "counts_in", "counts_out")] + [("tail_cap", c_i32)])


RESAMPLE_MAX_BANKS, SPEC_MAX_MASKS = 8, 32


class ResampleBank(ctypes.Structure):
    _fields_ = [(n, c_i32) for n in ("o", "n", "width", "n_live", "taps_at", "first_at", "off_at", "tile_blocks")]


class ResampleGroupDesc(ctypes.Structure):
    _fields_ = ([(n, c_p) for n in ("samples", "lengths", "bank", "taps", "tap_first", "tap_off", "out", "out_lens")] + [("ld", c_i64), ("ld_out", c_i64)] +
                [(n, c_i32) for n in ("B", "n_cols", "cap", "samples_i16", "G", "n_taps", "n_first", "n_off")] + [("banks", ResampleBank * RESAMPLE_MAX_BANKS)])


class SpecAugmentDesc(ctypes.Structure):
    _fields_ = ([(n, c_p) for n in ("feats", "lengths", "ids", "masks")] + [("item_stride", c_i64), ("row_stride", c_i64)] +
                [(n, c_i32) for n in ("B", "T_max", "F", "num_t_mask", "num_f_mask", "max_t", "max_f")] + [("seed", ctypes.c_uint32)])


class RescorePrepDesc(ctypes.Structure):
    _fields_ = ([(n, c_p) for n in ("tokens", "nlen", "score", "embed", "embed_r", "pe", "x0", "x0_r", "targets", "targets_r", "mask")] +
                [(n, c_i32) for n in ("B", "N", "Lmax", "D", "V", "sos", "eos")])


class TokenLogprobDesc(ctypes.Structure):
    _fields_ = ([(n, c_p) for n in ("X", "W", "bias", "logits", "target", "logp", "lse")] + [("ldx", c_i64), ("ld", c_i64)] +
                [(n, c_i32) for n in ("M", "D", "V", "x_dtype", "w_dtype")])


class LsmLossDesc(ctypes.Structure):
    _fields_ = ([(n, c_p) for n in ("X", "W", "bias", "logits", "target", "loss", "lse")] + [("ldx", c_i64), ("ld", c_i64)] +
                [(n, c_i32) for n in ("M", "D", "V", "x_dtype", "w_dtype")] + [("smoothing", c_f)])


class LsmGradDesc(ctypes.Structure):
    _fields_ = ([(n, c_p) for n in ("X", "W", "bias", "logits", "target", "lse", "g", "dz")] + [("ldx", c_i64), ("ld", c_i64), ("ldz", c_i64)] +
                [(n, c_i32) for n in ("M", "D", "V", "Vk", "x_dtype", "w_dtype", "dz_dtype")] + [("smoothing", c_f)])


class RescoreCombineDesc(ctypes.Structure):
    _fields_ = ([(n, c_p) for n in ("logp", "logp_r", "nlen", "score", "final_score", "left", "right", "order")] + [(n, c_i32) for n in ("B", "N", "Lc")] +
                [("first_pass_weight", c_f), ("reverse_weight", c_f)])


class DecStepAttnDesc(ctypes.Structure):
    _fields_ = ([(n, c_p) for n in ("q", "store", "slot", "klen", "step", "kv_new", "out")] + [(n, c_i64) for n in ("ldq", "ld_new", "ldo", "slots")] +
                [(n, c_i32) for n in ("R", "H", "dk", "cap", "slot_ld", "group", "stride", "klen_group", "io_dtype")])


class DecBeamPruneDesc(ctypes.Structure):
    _fields_ = ([(n, c_p) for n in ("topk_idx", "topk_logp", "embed", "pe", "max_len", "score", "token", "parent", "finished", "hlen", "klen", "tokens", "slots", "x", "step",
                                    "done", "n_done", "all_done", "nbest_tokens", "nbest_len", "nbest_score")] +
                [(n, c_i32) for n in ("B", "K", "k_ld", "Lmax", "D", "V", "eos")])


class CtcPrefixDesc(ctypes.Structure):
    _fields_ = ([(n, c_p) for n in ("x", "state", "psi", "topk_idx", "topk_logp", "token", "hlen", "finished", "step", "done", "lens", "parent", "tokens", "out_idx", "out_logp",
                                    "cand_psi")] +
                [(n, c_i32) for n in ("B", "K", "P", "T", "V", "Lmax", "blank", "eos")] + [("ctc_weight", c_f)])


class FfnSplitDesc(ctypes.Structure):
    _fields_ = [("x", c_p), ("psum", c_p), ("psum_b2", c_p), ("psum_splits", c_i32), ("psum_alpha", c_f), ("ln1_g", c_p), ("ln1_b", c_p), ("ln2_g", c_p),
                ("ln2_b", c_p), ("rows_out", c_p), ("rows2_out", c_p), ("ln_g", c_p), ("ln_b", c_p), ("w1", c_p), ("b1", c_p), ("N1", c_i32), ("act", c_i32),
                ("w2", c_p), ("psum_out", c_p), ("out16", c_p), ("ldo", c_i64), ("M", c_i32), ("D", c_i32), ("mode", c_i32), ("w_dtype", c_i32), ("eps", c_f),
                ("kv_ring", c_p), ("ring_offsets", c_p), ("ring_T", c_i32), ("ring_H", c_i32), ("ring_Tq", c_i32), ("ring_len", c_p)]


class LayerScratch(ctypes.Structure):
    _fields_ = [(n, c_p) for n in ("xn", "hid", "qkv", "pos", "ctx", "glu", "dw")] + [("psum", c_p), ("psum_splits", c_i32)]


class LayerIO(ctypes.Structure):
    _fields_ = [("B", c_i32), ("T", c_i32), ("D", c_i32), ("H", c_i32), ("FF", c_i32), ("ktaps", c_i32),
                ("act_dtype", c_i32), ("w_dtype", c_i32),
                ("attn_mask", c_p), ("am_sb", c_i64), ("am_sq", c_i64),
                ("pad_valid", c_p), ("pos_embed", c_p), ("pos_rows", c_i32),
                ("pos_proj", c_p), ("pos_proj_ld", c_i64),
                ("attn_cache", c_p), ("cache_T", c_i32), ("new_cache", c_p), ("after_g", c_p), ("after_b", c_p), ("after_out", c_p),
                ("kv_ring", c_p), ("stream_offset", c_p), ("ring_T", c_i32), ("causal_conv", c_i32), ("conv_cache", c_p), ("pos_shared", c_i32),
                ("next_w", c_p), ("next_x_out", c_p), ("macaron_done", c_i32), ("utt_len", c_p), ("stream_len", c_p)]


ROUTES = ("GENERAL", "FUSED_FFN", "CHAIN", "CHAIN_NEXT", "CHAIN_NEXT_CIN", "FFSPLIT", "PAIR")     # include/cfm.h cfm_route, by value (cfm_encoder_layer_route)

# The whole binding: every mirror above gets the header's name for it as `_c_name_`, and PROTOTYPES is (name, restype, *argtypes) for every function
# include/cfm.h declares, in the header's order; lib() applies it.  tests/abi_check.py has the compiler check each field and each prototype against the header.
for _c_name, _cls in dict(
        cfm_gemm_desc=GemmDesc, cfm_gemm_tn_desc=GemmTnDesc, cfm_attn_bwd_desc=AttnBwdDesc, cfm_attn_desc=AttnDesc, cfm_ffn_desc=FfnDesc, cfm_rowchain_desc=RowChainDesc,
        cfm_layer_train_weights=LayerTrainWeights, cfm_train_group=TrainGroup, cfm_layer_train_io=LayerTrainIO, cfm_layer_train_saved=LayerTrainSaved,
        cfm_layer_train_scratch=LayerTrainScratch, cfm_layer_train_grads=LayerTrainGrads, cfm_layer_weights=LayerWeights, cfm_ctc_group=CtcGroup,
        cfm_rnnt_desc=RnntDesc, cfm_lattice=Lattice, cfm_rnnt_packed_desc=RnntPackedDesc, cfm_rnnt_align_desc=RnntAlignDesc, cfm_rnnt_packed_align_desc=RnntPackedAlignDesc, cfm_ln_bwd_desc=LnBwdDesc, cfm_lstm_desc=LstmDesc, cfm_greedy_desc=GreedyDesc,
        cfm_greedy_chunk_desc=GreedyChunkDesc, cfm_ctc_greedy_desc=CtcGreedyDesc, cfm_ctc_beam_desc=CtcBeamDesc, cfm_ctc_align_desc=CtcAlignDesc, cfm_edit_distance_desc=EditDistanceDesc, cfm_rnnt_beam_desc=RnntBeamDesc, cfm_rnnt_beam_stream_desc=RnntBeamStreamDesc, cfm_fbank_desc=FbankDesc, cfm_resample_desc=ResampleDesc,
        cfm_resample_bank=ResampleBank, cfm_resample_group_desc=ResampleGroupDesc, cfm_spec_augment_desc=SpecAugmentDesc,
        cfm_rescore_prep_desc=RescorePrepDesc, cfm_token_logprob_desc=TokenLogprobDesc, cfm_rescore_combine_desc=RescoreCombineDesc, cfm_lsm_loss_desc=LsmLossDesc, cfm_lsm_grad_desc=LsmGradDesc,
        cfm_dec_step_attn_desc=DecStepAttnDesc, cfm_dec_beam_prune_desc=DecBeamPruneDesc, cfm_ctc_prefix_desc=CtcPrefixDesc,
        cfm_ffn_split_desc=FfnSplitDesc, cfm_layer_scratch=LayerScratch, cfm_layer_io=LayerIO).items():
    _cls._c_name_ = _c_name
PROTOTYPES = (
    ("cfm_version", c_int),
    ("cfm_last_error", ctypes.c_char_p),
    ("cfm_device_ok", c_int),
    ("cfm_gemm", c_int, P(GemmDesc), c_p),
    ("cfm_gemm_tn", c_int, P(GemmTnDesc), c_p),
    ("cfm_gemm_tn_group", c_int, P(GemmTnDesc), c_i32, c_p),
    ("cfm_ffn_fused", c_int, P(FfnDesc), c_p),
    ("cfm_rowchain", c_int, P(RowChainDesc), c_p),
    ("cfm_rowchain_supported", c_int, c_i32, c_i32),
    ("cfm_rowchain_dw_supported", c_int, c_i32),
    ("cfm_rowchain_pair_supported", c_int, c_i32, c_i32),
    ("cfm_layernorm", c_int, c_p, c_p, c_p, c_p, c_i32, c_p, c_p, c_p, c_i32, c_p, c_f, c_i64, c_i32, c_p),
    ("cfm_attention", c_int, P(AttnDesc), c_p),
    ("cfm_attention_group", c_int, P(AttnDesc), c_i32, c_p),
    ("cfm_kv_cache_pack", c_int, c_p, c_i32, c_p, c_p, c_i32, c_i64, c_i64, c_i64, c_i64, c_p, c_i32, c_i32, c_i32, c_i32, c_p),
    ("cfm_dwconv_bn_silu", c_int, c_p, c_i32, c_p, c_p, c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_p),
    ("cfm_conv1_relu", c_int, c_p, c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_p, c_p, c_p),
    ("cfm_conv1_relu_mma", c_int, c_p, c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_p, c_p, c_p),
    ("cfm_conv12_supported", c_int, c_i32, c_i32),
    ("cfm_conv12_relu", c_int, c_p, c_p, c_p, c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_p, c_p, c_p),
    ("cfm_conv12_plan", c_int, c_i64, c_i32, c_i32, P(c_i32), P(c_i32)),
    ("cfm_set_conv12_tile", c_i32, c_i32),
    ("cfm_valid_mask", c_int, c_p, c_i32, c_p, c_i32, c_i32, c_i32, c_i32, c_p),
    ("cfm_chunk_mask", c_int, c_p, c_i32, c_i32, c_i32, c_p),
    ("cfm_attn_mask", c_int, c_p, c_p, c_p, c_i32, c_i32, c_p),
    ("cfm_stream_prep", c_int, c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_p, c_i32, c_i32, c_p, c_p, c_p, c_p),
    ("cfm_kv_ring_write", c_int, c_p, c_p, c_i32, c_i64, c_i64, c_i64, c_i64, c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_p),
    ("cfm_stream_advance", c_int, c_p, c_p, c_p, c_p, c_i32, c_i32, c_i32, c_p),
    ("cfm_dwconv_causal_bn_silu", c_int, c_p, c_i32, c_p, c_p, c_p, c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_p),
    ("cfm_conv_cache_update", c_int, c_p, c_i32, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_p),
    ("cfm_cast", c_int, c_p, c_i32, c_p, c_i32, c_i64, c_p),
    ("cfm_add_rows", c_int, c_p, c_p, c_i64, c_i32, c_i32, c_p),
    ("cfm_encoder_layer_forward", c_int, P(LayerWeights), P(LayerScratch), P(LayerIO), c_p, c_p, c_i32, c_p, c_p, c_p),
    ("cfm_encoder_layer_route", c_i32, P(LayerWeights), P(LayerScratch), P(LayerIO), c_p, c_p),
    ("cfm_ffsplit_max_rows", c_i32),
    ("cfm_ctc_nll", c_int, c_p, c_i64, c_i32, c_i32, c_i32, c_p, c_p, c_i32, c_p, c_p, c_p, c_p),
    ("cfm_joint_act", c_int, c_p, c_i64, c_p, c_i64, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_p),
    ("cfm_rnnt_nll", c_int, P(RnntDesc), c_p),
    ("cfm_rnnt_grad", c_int, P(RnntDesc), c_p),
    ("cfm_joint_act_bwd_ws", c_i64, c_i32, c_i32, c_i32, c_i32),
    ("cfm_joint_act_bwd", c_int, c_p, c_i64, c_p, c_i64, c_p, c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_p),
    ("cfm_joint_act_packed", c_int, c_p, c_i64, c_p, c_i64, c_p, c_i32, P(Lattice), c_i32, c_p),
    ("cfm_joint_act_packed_bwd", c_int, c_p, c_i64, c_p, c_i64, c_p, c_p, c_p, c_p, P(Lattice), c_i32, c_p),
    ("cfm_rnnt_packed_nll", c_int, P(RnntPackedDesc), c_p),
    ("cfm_rnnt_packed_grad", c_int, P(RnntPackedDesc), c_p),
    ("cfm_rnnt_align_scratch_bytes", c_i64, c_i64),
    ("cfm_rnnt_align", c_int, P(RnntAlignDesc), c_p),
    ("cfm_rnnt_packed_align", c_int, P(RnntPackedAlignDesc), c_p),
    ("cfm_layernorm_bwd_ws", c_i64, c_i64, c_i32),
    ("cfm_layernorm_bwd_fused", c_int, P(LnBwdDesc), c_p),
    ("cfm_glu_bwd", c_int, c_p, c_i32, c_p, c_i32, c_p, c_i32, c_i64, c_i32, c_p),
    ("cfm_dwconv_bn_ws", c_i64, c_i32, c_i32, c_i32),
    ("cfm_dwconv_bn_train_groups", c_int, c_p, c_i32, c_p, c_p, c_p, c_p, c_p, c_p, c_f, c_f, c_p, c_p, c_p, c_i32, c_p, P(TrainGroup), c_i32, c_i32, c_i32, c_p),
    ("cfm_dwconv_bn_train_bwd_groups", c_int, c_p, c_i32, c_p, c_p, c_p, c_i32, c_p, c_p, c_i32, c_p, c_p, c_p, c_p, c_p, c_p, P(TrainGroup), c_i32, c_i32, c_i32, c_i32, c_p, c_p, c_p),
    ("cfm_col2im_relu_bwd", c_int, c_p, c_i32, c_p, c_i32, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_p),
    ("cfm_conv1_wgrad_ws", c_i64, c_i32, c_i32, c_i32),
    ("cfm_conv1_wgrad", c_int, c_p, c_i32, c_p, c_p, c_p, c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_p),
    ("cfm_attention_bwd", c_int, P(AttnBwdDesc), c_p),
    ("cfm_attention_bwd_group", c_int, P(AttnBwdDesc), c_i32, c_p),
    ("cfm_attention_bwd_force_general", None, c_i32),
    ("cfm_set_cin_merge", c_i32, c_i32),
    ("cfm_ffn_split", c_int, P(FfnSplitDesc), c_p),
    ("cfm_ffn_split_supported", c_int, c_i32, c_i32),
    ("cfm_ctc_nll_train_groups", c_int, P(CtcGroup), c_i32, c_i32, c_p),
    ("cfm_ctc_grad", c_int, c_p, c_i64, c_i32, c_i32, c_i32, c_p, c_p, c_i32, c_p, c_p, c_p, c_p, c_p, c_p, c_f, c_p, c_p, c_p),
    ("cfm_dropout_rows", c_int, c_p, c_i32, c_p, c_i32, c_p, c_f, c_f, ctypes.c_uint32, c_f, ctypes.c_uint32, c_i64, c_i32, c_p),
    ("cfm_dropout_mask", c_int, c_p, c_i64, c_f, ctypes.c_uint32, c_p),
    ("cfm_pack_matrices", c_int, c_p, c_i32, c_i64, c_i32, c_i32, c_p),
    ("cfm_pack_vectors", c_int, c_p, c_p, c_p, c_i64, c_p),
    ("cfm_encoder_train_forward", c_int, c_i32, P(LayerTrainWeights), P(LayerTrainIO), P(LayerTrainSaved), P(LayerTrainScratch), P(c_p), c_p),
    ("cfm_encoder_train_backward", c_int, c_i32, P(LayerTrainWeights), P(LayerTrainIO), P(LayerTrainSaved), P(LayerTrainScratch), P(LayerTrainGrads), P(c_p), c_p, c_p, c_p, LAYER_DONE_FN, c_p, P(c_p), c_p),
    ("cfm_adam_step", c_int, c_p, c_p, c_p, c_p, c_i64, c_f, c_f, c_f, c_f, c_f, c_i64, c_p, c_p),
    ("cfm_sumsq", c_int, c_p, c_i64, c_p, c_i32, c_p, c_p),
    ("cfm_adam_clip_step", c_int, c_p, c_p, c_p, c_p, c_i64, c_f, c_f, c_f, c_f, c_f, c_i64, c_p, c_f, c_f, c_i32, c_p, c_p),
    ("cfm_prof_enable", None, c_i32),
    ("cfm_prof_reset", None),
    ("cfm_prof_collect", c_int),
    ("cfm_prof_entry", c_int, c_i32, ctypes.c_char_p, c_i32, P(c_i64), P(ctypes.c_double), P(ctypes.c_double), P(ctypes.c_double)),
    ("cfm_greedy_step", c_int, P(GreedyDesc), c_p),
    ("cfm_greedy_chunk_begin", c_int, P(GreedyChunkDesc), c_p),
    ("cfm_greedy_chunk_step", c_int, P(GreedyChunkDesc), c_p),
    ("cfm_fbank", c_int, P(FbankDesc), c_p),
    ("cfm_fbank_stream", c_int, P(FbankDesc), c_p),
    ("cfm_lstm_save_floats", c_i64, c_i32, c_i32, c_i32),
    ("cfm_lstm_forward", c_int, P(LstmDesc), c_p),
    ("cfm_lstm_backward", c_int, P(LstmDesc), c_p),
    ("cfm_ctc_topk", c_int, c_p, c_i64, c_i32, c_i32, c_i32, c_p, c_i32, c_p, c_p, c_p, c_p),
    ("cfm_ctc_greedy", c_int, P(CtcGreedyDesc), c_p),
    ("cfm_ctc_beam_nodes", c_i64, c_i32, c_i32, c_i32),
    ("cfm_ctc_prefix_beam", c_int, P(CtcBeamDesc), c_p),
    ("cfm_ctc_align_scratch_bytes", c_i64, c_i32, c_i32, c_i32),
    ("cfm_ctc_align", c_int, P(CtcAlignDesc), c_p),
    ("cfm_edit_distance_scratch_bytes", c_i64, c_i32, c_i32, c_i32),
    ("cfm_edit_distance", c_int, P(EditDistanceDesc), c_p),
    ("cfm_rnnt_beam_nodes", c_i64, c_i32, c_i32, c_i32, c_i32),
    ("cfm_rnnt_beam_begin", c_int, P(RnntBeamDesc), c_p),
    ("cfm_rnnt_beam_step", c_int, P(RnntBeamDesc), c_p),
    ("cfm_rnnt_beam_stream_reset", c_int, P(RnntBeamStreamDesc), c_p, c_p),
    ("cfm_rnnt_beam_stream_feed", c_int, P(RnntBeamStreamDesc), c_p),
    ("cfm_rnnt_beam_stream_step", c_int, P(RnntBeamStreamDesc), c_p),
    ("cfm_rnnt_beam_stream_report", c_int, P(RnntBeamStreamDesc), c_p),
    ("cfm_resample", c_int, P(ResampleDesc), c_p),
    ("cfm_resample_stream", c_int, P(ResampleDesc), c_p),
    ("cfm_resample_tile_blocks", c_i32, c_i32, c_i32, c_i32),
    ("cfm_resample_group", c_int, P(ResampleGroupDesc), c_p),
    ("cfm_spec_augment", c_int, P(SpecAugmentDesc), c_p),
    ("cfm_rescore_prep", c_int, P(RescorePrepDesc), c_p),
    ("cfm_token_logprob", c_int, P(TokenLogprobDesc), c_p),
    ("cfm_rescore_combine", c_int, P(RescoreCombineDesc), c_p),
    ("cfm_lsm_loss", c_int, P(LsmLossDesc), c_p),
    ("cfm_lsm_grad", c_int, P(LsmGradDesc), c_p),
    ("cfm_lsm_reduce", c_int, c_p, c_p, c_i32, c_i32, c_p, c_p),
    ("cfm_dec_step_attn", c_int, P(DecStepAttnDesc), c_p),
    ("cfm_dec_beam_prune", c_int, P(DecBeamPruneDesc), c_p),
    ("cfm_ctc_logprob_t", c_int, c_p, c_i64, c_i32, c_i32, c_i32, c_p, c_p, c_p),
    ("cfm_ctc_prefix_score", c_int, P(CtcPrefixDesc), c_p),
    ("cfm_ctc_prefix_advance", c_int, P(CtcPrefixDesc), c_p),
)

_lib = None
_lock = threading.Lock()


def lib():
    """The loaded shared library; raises (loudly) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libconformer_gfx950.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C conformer-pytorch-lightning_amd/csrc`. There is no CPU fallback." % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, restype, *argtypes in PROTOTYPES:
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed (status %d): %s" % (what, rc, lib().cfm_last_error().decode(errors="replace")))


def dt_code(t):
    try:
        return _DT[t.dtype if isinstance(t, torch.Tensor) else t]
    except KeyError:
        raise TypeError("cfm: unsupported dtype %s (float32, bfloat16, float16 only)" % (t.dtype if isinstance(t, torch.Tensor) else t))


def torch_dtype(code):
    return _TORCH_DT[code]


def require_hip(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("cfm: tensor on %s -- this framework runs on MI355X (HIP) only; there is no CPU path" % t.device)


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def call(name, *args):
    """Launch the status-returning entry point `name`(*args, current stream); a non-zero status raises with cfm_last_error()."""
    check(getattr(lib(), name)(*args, stream()), name)


# ----------------------------------------------------------------------------------------------------------------------
# precision modes
# ----------------------------------------------------------------------------------------------------------------------
class Precision:
    """How the dense contractions are evaluated.

    bf16 : bf16 MFMA operands, f32 accumulate, bf16 intermediates, f32 residual stream (BASELINE.json config 2)
    fp16 : same speed, fp16 operands (11-bit mantissa)
    fp32 : "f32-accurate": f32 intermediates, every product as 3 bf16 MFMAs on hi/lo splits (~16 mantissa bits)
    """

    def __init__(self, name):
        if name not in ("bf16", "fp16", "fp32"):
            raise ValueError("precision must be bf16, fp16 or fp32, got %r" % (name,))
        self.name = name
        self.split = name == "fp32"
        self.w_code = F16 if name == "fp16" else BF16
        self.act_code = F32 if self.split else self.w_code
        self.w_dtype = torch_dtype(self.w_code)
        self.act_dtype = torch_dtype(self.act_code)

    def __repr__(self):
        return "Precision(%s)" % self.name


_precision = Precision(os.environ.get("CFM_PRECISION", "bf16"))


def set_precision(name):
    global _precision
    _precision = name if isinstance(name, Precision) else Precision(name)
    return _precision


def get_precision():
    return _precision


def resolve_precision(module=None):
    """The precision a module computes in: its own `precision` attribute when set (a name or a Precision; see
    ConformerEncoder.set_precision), else the process default.  Resolved per call -- two encoders at different precisions can run
    side by side."""
    p = getattr(module, "precision", None) if module is not None else None
    if p is None:
        return _precision
    return p if isinstance(p, Precision) else Precision(p)


_warned = set()


def check_mode(module, what):
    """Shared train / eval gate of the drop-in modules.  Returns True when the module must take its TRAIN path (module.training):
    BatchNorm batch statistics, dropout from the kernels' counter-based generator, autograd Functions.
    In eval mode the forward is inference-only: gradients do not flow (warned once when someone might expect them to)."""
    if module.training:
        return True
    if torch.is_grad_enabled() and what not in _warned and any(q.requires_grad for q in module.parameters()):
        _warned.add(what)
        import warnings
        warnings.warn("%s: eval-mode forward runs inference kernels; its output is detached from the parameters. "
                      "Call .train() for a differentiable forward, or wrap inference in torch.no_grad()." % what)
    return False


from .ops import *  # noqa: E402,F401,F403
