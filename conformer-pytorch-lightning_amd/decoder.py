"""CTC head -- drop-in for the class of the same name in the reference's src/decoder.py:7-23 (forward / loss evaluation only).

    logits = ctc_lo(dropout(encoder_out))                      cfm_gemm, f32 logits, vocabulary padded to a multiple of 4 columns
    loss   = CTCLoss(sum)(log_softmax(logits), labels, enc_lens, label_lens) / labels.size(1)      cfm_ctc_nll + a host-side sum

Same constructor arguments and parameter names (`ctc_lo.weight`, `ctc_lo.bias`) as the reference.  Quirk Q7 is kept: the reference
calls F.dropout with its default training=True, i.e. it drops activations even in eval mode; with dropout > 0 this module does the same
(and is then as random as the reference), parity is defined and tested at dropout = 0.  In train mode `forward` is differentiable
(cfm/autograd.py CTCLossFn, the batch as a window of one micro-batch: the alpha and beta recursions and d loss / d logits in csrc/ctc.hip, the
projection's gradients through cfm_gemm / cfm_gemm_tn); `nll` is loss evaluation only.

Decoding (eval mode only, csrc/ctc_decode.hip; the reference has none): `greedy_search` (best path), `prefix_beam_search` (n-best lists with
scores) and `CTCGreedyStream` (best path chunk by chunk, all state on the device).  They read the same logits as `nll` but apply NO dropout:
Q7 is a quirk of the reference's loss, a decoder that drops activations would only be a worse decoder.

Forced alignment (eval mode only, cfm_ctc_align in csrc/ctc.hip; the reference has none): `forced_align` gives, for a known transcript, each
token's first and last encoder frame and its log-probability along the best single alignment, and that alignment's score.  Blank is 0 as in the
loss, and there is no dropout, for the same reason as in decoding.
"""
import math

import torch
import torch.nn as nn

import cfm
import token_log
from cfm import packing
from greedy import _Search, _nbest_lists


class CTCDecoder(nn.Module):

    def __init__(self, vocab_size, encoder_dim, dropout):
        super().__init__()
        self.ctc_lo = nn.Linear(encoder_dim, vocab_size)
        self.dropout = dropout
        self._pack = packing.PackCache()

    def _weights(self, prec):
        def build():
            V, D = self.ctc_lo.weight.shape
            Vp = (V + 3) // 4 * 4                              # cfm_gemm wants N % 4 == 0; the pad columns are never read by cfm_ctc_nll
            w = torch.zeros((Vp, D), dtype=torch.float32, device=self.ctc_lo.weight.device)
            w[:V] = self.ctc_lo.weight.detach()
            b = torch.zeros((Vp,), dtype=torch.float32, device=w.device)
            b[:V] = self.ctc_lo.bias.detach()
            wm, wlo = packing.matrix(w, prec)
            return packing.Packed(w=wm, w_lo=wlo, b=b, V=V, Vp=Vp)
        return self._pack.get([self.ctc_lo.weight, self.ctc_lo.bias], prec, build)

    @staticmethod
    def _logits(x, pk):
        """f32 logits [B, T, Vp] of x [B, T, D] (columns V..Vp are padding that no consumer reads)."""
        B, T, D = x.shape
        x2 = (x if x.dtype == torch.float32 else x.float()).contiguous().view(B * T, D)
        return cfm.gemm(x2, pk.w, bias=pk.b, w_lo=pk.w_lo, out_dtype=torch.float32).view(B, T, pk.Vp)

    def nll(self, encoder_out, encoder_out_lens, padded_labels, label_lengths):
        """Per-utterance CTC negative log-likelihood, f32 [B] (loss evaluation: not differentiable -- use forward in train mode)."""
        cfm.require_hip(encoder_out)
        prec = cfm.resolve_precision(self)
        pk = self._weights(prec)
        x = nn.functional.dropout(encoder_out, self.dropout)      # training=True by default, as decoder.py:19 (quirk Q7)
        logits = self._logits(x, pk)
        dev = x.device
        i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()
        return cfm.ctc_nll(logits, pk.V, i32(encoder_out_lens), i32(padded_labels), i32(label_lengths))

    def forward(self, encoder_out, encoder_out_lens, padded_labels, label_lengths):
        if self.training:
            # differentiable path (cfm/autograd.py CTCLossFn): the batch's [B*T', D] rows as a window of one micro-batch
            from cfm import autograd as ag
            cfm.require_hip(encoder_out)
            dev = encoder_out.device
            i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()
            x = nn.functional.dropout(encoder_out, self.dropout)          # training=True by default, as decoder.py:19 (quirk Q7); a torch op
            B, T, D = x.shape
            g = (B, T, i32(encoder_out_lens), i32(padded_labels), i32(label_lengths))
            return ag.CTCLossFn.apply(x.reshape(B * T, D), self, cfm.resolve_precision(self), [g], self.ctc_lo.weight, self.ctc_lo.bias).reshape(())
        loss = self.nll(encoder_out, encoder_out_lens, padded_labels, label_lengths).sum()
        return loss / padded_labels.size(1)

    def forward_window(self, rows, groups):
        """Train mode: the CTC losses of an accumulation window in one projection.  rows f32 [sum B_g*T'_g, D]: the encoder outputs of the window's
        micro-batches as ONE row matrix (ConformerEncoder.forward_window(..., return_rows=True)); groups: [(B, T', encoder_out_lens, padded_labels,
        label_lengths)] in row order.  Returns a 1-D tensor of the micro-batches' losses, entry g equal to forward() on micro-batch g alone
        (decoder.py:18-23; the always-on F.dropout of :19 draws one mask over all rows instead of one per micro-batch)."""
        if not self.training:
            raise RuntimeError("CTCDecoder.forward_window is the train-mode path; in eval mode call forward per batch")
        from cfm import autograd as ag
        cfm.require_hip(rows)
        dev = rows.device
        i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()
        x = nn.functional.dropout(rows, self.dropout)                    # training=True by default, as decoder.py:19 (quirk Q7)
        gs = [(int(B), int(T), i32(el), i32(lab), i32(ll)) for B, T, el, lab, ll in groups]
        return ag.CTCLossFn.apply(x, self, cfm.resolve_precision(self), gs, self.ctc_lo.weight, self.ctc_lo.bias)

    # -- decoding (inference only) ------------------------------------------------------------------------------------------------------------
    def _topk(self, encoder_out, encoder_out_lens, k, who):
        """(idx, logp, lse, lens int32 on the device, V) of cfm.ctc_topk on the head's logits: no dropout (see the module docstring)."""
        if self.training:
            raise RuntimeError("CTCDecoder.%s is an eval-mode operation (inference only); in train mode call forward" % who)
        cfm.require_hip(encoder_out)
        if encoder_out.dim() != 3:
            raise ValueError("CTCDecoder.%s: encoder_out must be [B, T, D], got %s" % (who, tuple(encoder_out.shape)))
        pk = self._weights(cfm.resolve_precision(self))
        lens = torch.as_tensor(encoder_out_lens).to(device=encoder_out.device, dtype=torch.int32).contiguous()
        return cfm.ctc_topk(self._logits(encoder_out, pk), pk.V, lens, k) + (lens, pk.V)

    @torch.no_grad()
    def greedy_search(self, encoder_out, encoder_out_lens, blank=0, return_details=False):
        """Best path: per frame the most probable class, repeats collapsed, blanks dropped (cfm_ctc_topk with k = 1, cfm_ctc_greedy).
        encoder_out [B, T, D], encoder_out_lens (B,).  Returns a list of B token lists; return_details=True: (that list, details) with
        details = {"frames": int32 [B, T], "logp": f32 [B, T], "count": int64 [B]} on the device -- per emitted token its frame and its
        log-probability, count[b] of them valid per row."""
        idx, logp, _, lens, V = self._topk(encoder_out, encoder_out_lens, 1, "greedy_search")
        S = cfm.ctc_greedy(idx, logp, lens, V, blank=blank)
        counts = S["count"].tolist()
        hyps = S["hyps"].cpu()
        out = [hyps[b, :counts[b]].tolist() for b in range(len(counts))]
        return (out, {"frames": S["frames"], "logp": S["token_logp"], "count": S["count"]}) if return_details else out

    @torch.no_grad()
    def prefix_beam_search(self, encoder_out, encoder_out_lens, beam=10, blank=0):
        """CTC prefix beam search (cfm_ctc_topk with k = min(beam, V), beam <= 16, cfm_ctc_prefix_beam; include/cfm.h states the algorithm and its ranking
        rule).  Returns per utterance a list of (tokens, score) pairs, best first; score = log of the summed probability of the alignments of
        the token string that the search kept."""
        beam = int(beam)
        idx, logp, _, lens, V = self._topk(encoder_out, encoder_out_lens, max(1, min(beam, self.ctc_lo.out_features)), "prefix_beam_search")
        tokens, nlen, score = cfm.ctc_prefix_beam(idx, logp, lens, V, beam=beam, blank=blank)
        tokens, nlen, score = tokens.cpu(), nlen.tolist(), score.tolist()
        return [[(tokens[b, n, :nlen[b][n]].tolist(), score[b][n]) for n in range(len(nlen[b])) if score[b][n] > float("-inf")] for b in range(len(nlen))]

    @torch.no_grad()
    def forced_align(self, encoder_out, encoder_out_lens, padded_labels, label_lengths, return_path=False):
        """Forced alignment: which frames carry which token of a KNOWN transcript (cfm_ctc_align: the best single alignment, blank 0 as in the loss;
        include/cfm.h states the recursion and its tie rule).  encoder_out [B, T, D], encoder_out_lens (B,), padded_labels [B, Umax] (padding beyond
        label_lengths[b] is ignored), label_lengths (B,).  Returns a list of B entries: None for an utterance that has no alignment (fewer frames than
        labels plus adjacent repeats), else {"score": the path's log-probability, "tokens": [(token, start_frame, end_frame, logp), ...]} with
        inclusive encoder frames and logp the sum of the token's frames' log-probabilities; return_path=True adds "path", the int32 [len] state
        indices 0..2U (odd 2u+1: label u, even: blank) on the host.  One host transfer per call."""
        if self.training:
            raise RuntimeError("CTCDecoder.forced_align is an eval-mode operation (inference only); in train mode call forward")
        cfm.require_hip(encoder_out)
        if encoder_out.dim() != 3:
            raise ValueError("CTCDecoder.forced_align: encoder_out must be [B, T, D], got %s" % (tuple(encoder_out.shape),))
        B, T = encoder_out.shape[:2]
        dev = encoder_out.device
        i32 = lambda t: torch.as_tensor(t).to(device=dev, dtype=torch.int32).contiguous()
        lens, labels, llens = i32(encoder_out_lens), i32(padded_labels), i32(label_lengths)
        if labels.dim() != 2 or labels.shape[0] != B or lens.shape != (B,) or llens.shape != (B,):
            raise ValueError("CTCDecoder.forced_align: %d utterances, but lengths %s, labels %s, label lengths %s" %
                             (B, tuple(lens.shape), tuple(labels.shape), tuple(llens.shape)))
        pk = self._weights(cfm.resolve_precision(self))
        Umax = labels.shape[1]
        if Umax == 0:                                          # cfm_ctc_align wants a label column; an empty transcript aligns all-blank
            labels = torch.zeros((B, 1), dtype=torch.int32, device=dev)
        path, score, start, end, token_logp = cfm.ctc_align(self._logits(encoder_out, pk), pk.V, lens, labels, llens)
        # one transfer: everything as float64 columns (frames, states and lengths are far below 2^53)
        host = torch.cat([t.to(torch.float64).reshape(B, -1) for t in (score, lens.clamp(0, T), llens.clamp(0, Umax), labels, start, end, token_logp, path)], 1).cpu()
        W = labels.shape[1]
        out = []
        for b in range(B):
            row = host[b]
            sc, n, U = float(row[0]), int(row[1]), int(row[2])
            if sc == float("-inf"):
                out.append(None)
                continue
            lab, st, en, lp = (row[3 + k * W:3 + k * W + U].tolist() for k in range(4))
            entry = {"score": sc, "tokens": [(int(lab[u]), int(st[u]), int(en[u]), lp[u]) for u in range(U)]}
            if return_path:
                entry["path"] = row[3 + 4 * W:3 + 4 * W + n].to(torch.int32)
            out.append(entry)
        return out


class CTCGreedyStream:
    """Best-path CTC decoding of `streams` utterances chunk by chunk -- `CTCDecoder.greedy_search` as a streaming step, with the contract of
    greedy.ChunkGreedySearch's decode / hyps / reset.  All state lives on the device: per stream the last frame's class (`prev`: a repeat that
    straddles two chunks collapses), the frames seen so far, the hypothesis buffer, its frames and log-probabilities, and the counts.  A decode
    is three launches (projection, cfm_ctc_topk, cfm_ctc_greedy) and one host read of the counts; a chunk of C frames adds at most C symbols per
    stream, so the buffers are grown BEFORE a chunk that could overflow them (token_log, as ChunkGreedySearch) and the overflow flag stays an error."""

    def __init__(self, ctc, streams, blank=0, max_tokens=None):
        self.ctc, self.B, self.blank = ctc, int(streams), int(blank)
        if self.B < 1:
            raise ValueError("CTCGreedyStream: streams is positive")
        self.dev = ctc.ctc_lo.weight.device
        self.S = cfm.ctc_greedy_state(self.B, max(1, int(max_tokens) if max_tokens is not None else 256), self.dev) if self.dev.type == "cuda" else None
        self._lens = torch.zeros((self.B,), dtype=torch.int32, device=self.dev)         # this chunk's frames per stream, as the kernels read them
        self._log = token_log.TokenLog(self.B)

    def reset(self, streams=None):
        """New utterances on the given streams (all by default): no previous class, frame 0, hypotheses emptied."""
        if self.S is None:
            raise RuntimeError("cfm: CTCGreedyStream on %s -- this framework runs on MI355X (HIP) only; there is no CPU path" % self.dev)
        streams = None if streams is None else list(streams)
        idx = packing.stream_index(streams, self.dev)
        self.S["prev"][idx] = -1
        for k in ("frame_base", "count", "hyps", "frames", "token_logp"):
            self.S[k][idx] = 0
        self._log.reset(streams)

    def hyps(self):
        """Everything emitted per stream since its last reset."""
        return self._log.hyps()

    @torch.no_grad()
    def decode(self, enc_chunk, lens=None):
        """enc_chunk (B, C, D) encoder output of one chunk (any C); lens (B,): how many of its frames belong to each stream (default: all; 0: the
        stream is idle and nothing about it changes).  Returns a list of B lists: the tokens this chunk added."""
        if self.ctc.training:
            raise RuntimeError("CTCGreedyStream.decode is an eval-mode operation (inference only)")
        cfm.require_hip(enc_chunk)
        B = self.B
        if enc_chunk.dim() != 3 or enc_chunk.shape[0] != B or enc_chunk.device != self.dev:
            raise ValueError("CTCGreedyStream.decode wants (%d, C, D) on %s, got %s on %s" % (B, self.dev, tuple(enc_chunk.shape), enc_chunk.device))
        C = enc_chunk.shape[1]
        packing.stream_lens("CTCGreedyStream.decode", "lens", B, lens, C, self._lens)   # clamped to 0 .. C here as the kernels clamp them
        token_log.grow(self.S, ("hyps", "frames", "token_logp"), self._log.most() + C)
        idx, logp, _, lens, V = self.ctc._topk(enc_chunk, self._lens, 1, "greedy_search")
        cfm.ctc_greedy(idx, logp, lens, V, blank=self.blank, state=self.S)
        rep = torch.cat([self.S["count"], self.S["overflow"].to(torch.int64)]).tolist()
        counts, overflow = rep[:B], rep[B]
        if overflow:
            raise RuntimeError("CTCGreedyStream: a stream emitted more symbols than the hypothesis buffer holds")
        return self._log.take(self.S["hyps"], counts)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# Attention decoder (eval mode only) and the rescoring of n-best lists
# ------------------------------------------------------------------------------------------------------------------------------------------------
class TransformerDecoder(nn.Module):
    """Drop-in for the reference's class of the same name (src/decoder.py:26-73): constructor arguments, submodule and parameter names, the
    forward signature and its three return values.  The reference's own decoder cannot run (decoder_layer.py:51 adds a tuple to a tensor), so the
    arithmetic is the pre-norm transformer decoder stated in float64 in tests/attention_decoder_ref.py; eval mode only.

    One deliberate difference from what the reference's lines would do: `embed` stays nn.Sequential(nn.Embedding, PositionalEncoding) -- the
    state_dict keys are the reference's -- but it is NOT called.  PositionalEncoding.forward keeps the reference's quirk of slicing its table by
    the BATCH size (attention.py:119), and a decoder built on that would score the same hypothesis differently depending on its batch slot.  The
    decoder indexes the f32 sinusoid table (attention._sinusoid_table) by POSITION itself and scales the embedding by sqrt(D):
    x_i = E[token_i] * sqrt(D) + pe[i]."""

    def __init__(self, vocab_size, decoder_dim, num_heads, hidden_dim, num_layers, dropout, positional_dropout, self_attention_dropout,
                 src_attention_dropout):
        super().__init__()
        from attention import PositionalEncoding
        from decoder_layer import TransformerDecoderLayer
        self.embed = nn.Sequential(nn.Embedding(vocab_size, decoder_dim), PositionalEncoding(decoder_dim, positional_dropout))
        self.after_norm = nn.LayerNorm(decoder_dim, eps=1e-5)
        self.output_layer = nn.Linear(decoder_dim, vocab_size)
        self.decoders = nn.ModuleList([TransformerDecoderLayer(decoder_dim, num_heads, hidden_dim, dropout, self_attention_dropout, src_attention_dropout)
                                       for _ in range(num_layers)])
        self._pack = packing.PackCache()
        self._pe = None                                        # f32 [max_len, D] on the parameters' device: a plain attribute, not in the state_dict

    def position_table(self, rows):
        from attention import _sinusoid_table
        dev = self.output_layer.weight.device
        if self._pe is None or self._pe.device != dev or self._pe.shape[0] < rows:
            self._pe = _sinusoid_table(max(int(rows), 5000), self.output_layer.in_features)[:, 0].contiguous().to(dev)
        return self._pe

    def _output_pack(self, prec):
        def build():
            V, D = self.output_layer.weight.shape
            Vp = (V + 3) // 4 * 4                              # cfm_gemm wants N % 4 == 0; cfm_token_logprob never reads rows V..Vp
            w = torch.zeros((Vp, D), dtype=torch.float32, device=self.output_layer.weight.device)
            w[:V] = self.output_layer.weight.detach()
            b = torch.zeros((Vp,), dtype=torch.float32, device=w.device)
            b[:V] = self.output_layer.bias.detach()
            wm, wlo = packing.matrix(w, prec)
            return packing.Packed(w=wm, w_lo=wlo, b=b, V=V, Vp=Vp)
        return self._pack.get([self.output_layer.weight, self.output_layer.bias], prec, build)

    def rows_forward(self, x, self_shape, self_mask, memory_rows, src_shape, memory_mask, prec):
        """The layers and after_norm on the f32 row matrix x [R, D] (overwritten): the normalised rows in the activation type, ready for the output
        projection.  The shapes and masks are decoder_layer.layer_rows'."""
        from decoder_layer import _no_training, layer_rows
        _no_training(self)
        for layer in self.decoders:
            layer_rows(layer, x, self_shape, self_mask, memory_rows, src_shape, memory_mask, prec)
        return cfm.layernorm(x, self.after_norm.weight, self.after_norm.bias, out1_dtype=prec.act_dtype)[0]

    @torch.no_grad()
    def forward(self, memory, memory_mask, targets, target_lengths, r_targets=None, reverse_weight=None):
        """memory [B, T, D], memory_mask bool [B, 1, T], targets long [B, L] (sos + labels), target_lengths (B,).  Returns (logits [B, L, V] -- the
        unfused cfm.gemm, because the caller wants logits --, torch.tensor(0.0), targets_mask.sum(dim=1)) as decoder.py:62-73."""
        import math
        from decoder_layer import _no_training
        from utils import make_pad_mask, make_subsequent_mask
        _no_training(self)
        cfm.require_hip(memory, targets)
        prec = cfm.resolve_precision(self)
        B, L = targets.shape
        T, D = memory.shape[1], memory.shape[2]
        dev = memory.device
        lens = torch.as_tensor(target_lengths).to(device=dev, dtype=torch.int32)
        targets_mask = ~make_pad_mask(lens, L).unsqueeze(1)
        targets_mask = targets_mask & make_subsequent_mask(L, dev).unsqueeze(0)                       # [B, L, L]
        E = self.embed[0].weight.detach()
        x = (E[targets.long()].double() * math.sqrt(D) + self.position_table(L)[:L].double()).float().reshape(B * L, D).contiguous()
        mem = memory.detach().to(torch.float32).reshape(B * T, D).contiguous()
        xn = self.rows_forward(x, (B, L), cfm.as_u8_mask(targets_mask), mem, (B, L, T), cfm.as_u8_mask(memory_mask.expand(B, 1, T)), prec)
        pk = self._output_pack(prec)
        logits = cfm.gemm(xn, pk.w, bias=pk.b, w_lo=pk.w_lo, out_dtype=torch.float32)[:, :pk.V].reshape(B, L, pk.V)
        return logits, torch.tensor(0.0), targets_mask.sum(dim=1)


class BiTransformerDecoder(nn.Module):
    """Drop-in for src/decoder.py:76-121: left_decoder and right_decoder (the keys decoder.left_decoder.* / decoder.right_decoder.* of the loadable
    checkpoints), forward as decoder.py:110-121."""

    def __init__(self, vocab_size, decoder_dim, num_heads, hidden_dim, num_layers, r_num_layers, dropout, pos_enc_dropout, self_attention_dropout,
                 src_attention_dropout):
        super().__init__()
        self.left_decoder = TransformerDecoder(vocab_size, decoder_dim, num_heads, hidden_dim, num_layers, dropout, pos_enc_dropout,
                                               self_attention_dropout, src_attention_dropout)
        self.right_decoder = TransformerDecoder(vocab_size, decoder_dim, num_heads, hidden_dim, r_num_layers, dropout, pos_enc_dropout,
                                                self_attention_dropout, src_attention_dropout)

    def forward(self, memory, memory_mask, targets, target_lengths, r_targets, reverse_weight):
        left_outputs, right_outputs, output_lengths = self.left_decoder(memory, memory_mask, targets, target_lengths)
        if reverse_weight > 0.0:
            right_outputs, _, output_lengths = self.right_decoder(memory, memory_mask, r_targets, target_lengths)
        return left_outputs, right_outputs, output_lengths


class AttentionLoss(nn.Module):
    """The attention head's training loss (the reference's commented-out loss_attn, model.py:85): label-smoothed cross entropy of the left decoder
    on (sos + y, y + eos) and, when reverse_weight > 0, of the right decoder on the reversed labels:

        loss_att = (1 - reverse_weight) * loss_left + reverse_weight * loss_right

    forward(encoder_out [B, T, D], encoder_mask bool [B, 1, T], padded_labels [B, U] (ignore_id: padding), label_lengths [B]) returns
    (loss_att, loss_left, loss_right).  Train mode: one cfm.autograd.DecoderLossFn per decoder -- gradients for every decoder parameter and for
    encoder_out.  Eval mode: the same value, nothing saved, no gradient.  The loss is divided by the batch size, or with normalize_length by the
    number of target tokens.  The eval-only entry points of the decoders (forward, AttentionRescorer) are unchanged."""

    def __init__(self, decoder, lsm_weight=0.0, reverse_weight=0.0, sos=None, eos=None, ignore_id=-1, normalize_length=False, fused=False):
        super().__init__()
        if isinstance(decoder, BiTransformerDecoder):
            left, right = decoder.left_decoder, decoder.right_decoder
        elif isinstance(decoder, TransformerDecoder):
            left, right = decoder, None
        else:
            raise TypeError("AttentionLoss: decoder is a TransformerDecoder or a BiTransformerDecoder, got %s" % type(decoder).__name__)
        self.decoder = decoder
        self.lsm_weight, self.reverse_weight = float(lsm_weight), float(reverse_weight)
        if not 0.0 <= self.reverse_weight <= 1.0 or not 0.0 <= self.lsm_weight < 1.0:
            raise ValueError("AttentionLoss: reverse_weight in [0, 1] and lsm_weight in [0, 1), got %r and %r" % (reverse_weight, lsm_weight))
        if self.reverse_weight > 0.0 and right is None:
            raise ValueError("AttentionLoss: reverse_weight > 0 needs a BiTransformerDecoder (a right decoder)")
        V = left.output_layer.out_features
        self.sos = V - 1 if sos is None else int(sos)
        self.eos = V - 1 if eos is None else int(eos)
        self.ignore_id, self.normalize_length, self.fused = int(ignore_id), bool(normalize_length), bool(fused)

    def _one(self, dec, encoder_out, mem_mask8, labels, prec):
        from cfm import autograd as ag
        from utils import add_sos_eos, make_subsequent_mask
        ys_in, ys_out = add_sos_eos(labels, self.sos, self.eos, self.ignore_id)
        B, Lc = ys_in.shape
        valid = ys_out != self.ignore_id                                                      # position i is a real one: i < L + 1
        self_mask = valid.unsqueeze(1) & make_subsequent_mask(Lc, ys_in.device).unsqueeze(0)   # [B, Lc, Lc]: j <= i and j < L + 1
        tgt = torch.where(valid, ys_out, torch.full_like(ys_out, -1)).to(torch.int32)
        args = (dec, ys_in.to(torch.int32), tgt, cfm.as_u8_mask(self_mask), mem_mask8, prec, self.lsm_weight, 0 if self.normalize_length else B)
        if dec.training:
            return ag.DecoderLossFn.apply(encoder_out, *args, ag.draw_seed(), self.fused, *dec.parameters())
        with torch.no_grad():
            return ag.DecoderLossFn.apply(encoder_out.detach(), *args, 0, self.fused)

    def forward(self, encoder_out, encoder_mask, padded_labels, label_lengths):
        from utils import reverse_sequence
        cfm.require_hip(encoder_out, encoder_mask, padded_labels)                             # no CPU path
        prec = cfm.resolve_precision(self.decoder)
        B, T = encoder_out.shape[0], encoder_out.shape[1]
        mem_mask8 = cfm.as_u8_mask(encoder_mask.expand(B, 1, T))
        left = self.decoder.left_decoder if isinstance(self.decoder, BiTransformerDecoder) else self.decoder
        labels = padded_labels.long()
        loss_left = self._one(left, encoder_out, mem_mask8, labels, prec)
        loss_right = torch.zeros((), dtype=torch.float32, device=encoder_out.device)
        if self.reverse_weight > 0.0:
            r = reverse_sequence(labels, label_lengths, self.ignore_id).long()
            loss_right = self._one(self.decoder.right_decoder, encoder_out, mem_mask8, r, prec)
        return (1.0 - self.reverse_weight) * loss_left + self.reverse_weight * loss_right, loss_left, loss_right


class AttentionRescorer:
    """Second pass over n-best lists: every hypothesis is scored by the attention decoder against its utterance's encoder output and the lists are
    re-ranked (the definition: tests/attention_decoder_ref.py; the kernels: csrc/rescore.hip).

        final = (1 - reverse_weight) * s_left + reverse_weight * s_right + first_pass_weight * first_pass_score

    with s(y) = sum_i log_softmax(logits_i)[target_i] over (y_1..y_L, eos); the right decoder scores the reversed hypothesis and runs only when
    reverse_weight > 0 (it needs a BiTransformerDecoder).  No length normalisation.  `sos` / `eos` default to vocab_size - 1, as in model.py.

    A pass per group of utterances: cfm_rescore_prep (inputs, targets and masks from the device n-best buffers), per layer self-attention over
    P = B*N rows of Lc = Lmax + 1 positions and cross-attention as B utterances of N*Lc queries (the memory's keys and values projected once per
    utterance and layer), after_norm, cfm_token_logprob (fused=True: the output projection and the log-softmax gather without the logits;
    fused=False, and always in the fp32 precision mode: cfm_gemm, then the kernel's logits form), cfm_rescore_combine.  One host read at the end.
    Utterances are grouped so that a group has at most MAX_ROWS = 65536 decoder rows (B * N * Lc)."""

    MAX_ROWS = 65536
    DEFAULT_FUSED = True

    def __init__(self, decoder, first_pass_weight=0.5, reverse_weight=0.0, sos=None, eos=None, fused=None):
        if isinstance(decoder, BiTransformerDecoder):
            self.left, self.right = decoder.left_decoder, decoder.right_decoder
        elif isinstance(decoder, TransformerDecoder):
            self.left, self.right = decoder, None
        else:
            raise TypeError("AttentionRescorer: decoder is a TransformerDecoder or a BiTransformerDecoder, got %s" % type(decoder).__name__)
        self.decoder = decoder
        self.first_pass_weight, self.reverse_weight = float(first_pass_weight), float(reverse_weight)
        if not 0.0 <= self.reverse_weight <= 1.0:
            raise ValueError("AttentionRescorer: reverse_weight in [0, 1], got %r" % (reverse_weight,))
        if self.reverse_weight > 0.0 and self.right is None:
            raise ValueError("AttentionRescorer: reverse_weight > 0 needs a BiTransformerDecoder (a right decoder)")
        V = self.left.output_layer.out_features
        self.sos = V - 1 if sos is None else int(sos)
        self.eos = V - 1 if eos is None else int(eos)
        self.fused = self.DEFAULT_FUSED if fused is None else bool(fused)

    def _logp(self, dec, x0, targets, mask, mem, mem_mask, B, N, Lc, T, prec):
        xn = dec.rows_forward(x0, (B * N, Lc), mask, mem, (B, N * Lc, T), mem_mask, prec)
        pk = dec._output_pack(prec)
        D = xn.shape[1]
        if self.fused and not prec.split and D % 8 == 0 and D <= 512:
            return cfm.token_logprob(xn, pk.w, pk.b, targets.view(-1), pk.V)
        logits = cfm.gemm(xn, pk.w, bias=pk.b, w_lo=pk.w_lo, out_dtype=torch.float32)
        return cfm.token_logprob(None, None, None, targets.view(-1), pk.V, logits=logits)

    def scores(self, encoder_out, encoder_out_lens, tokens, nlen, score):
        """The device half: (final, left, right f32 [B, N], order int32 [B, N]) of the device n-best buffers tokens int32 [B, N, Lmax], nlen int32
        [B, N] (-1: unused), score f32 [B, N]; no host synchronisation."""
        if self.decoder.training:
            raise NotImplementedError("AttentionRescorer: eval mode only -- the attention decoder has no backward (cross-attention); call .eval()")
        cfm.require_hip(encoder_out, tokens, nlen, score)
        prec = cfm.resolve_precision(self.decoder)
        B, N, Lmax = tokens.shape
        if encoder_out.dim() != 3 or encoder_out.shape[0] != B:
            raise ValueError("AttentionRescorer: encoder_out %s for %d n-best lists" % (tuple(encoder_out.shape), B))
        if not 1 <= N <= 16 or Lmax + 1 > 1024:
            raise ValueError("AttentionRescorer: N = %d hypotheses of up to %d tokens; 1 <= N <= 16 and at most 1023 tokens" % (N, Lmax))
        Lc, T, D = Lmax + 1, encoder_out.shape[1], encoder_out.shape[2]
        dev = encoder_out.device
        lens = torch.as_tensor(encoder_out_lens).to(device=dev, dtype=torch.int32)
        mem_mask = cfm.as_u8_mask(cfm.valid_mask(lens, T)).view(B, 1, T)
        mem = encoder_out.detach().to(torch.float32).reshape(B * T, D).contiguous()
        pe = self.left.position_table(Lc)
        two = self.reverse_weight > 0.0
        group = max(1, self.MAX_ROWS // (N * Lc))
        outs = []
        with torch.no_grad():
            for b0 in range(0, B, group):
                b1 = min(B, b0 + group)
                tk, nl, sc = tokens[b0:b1].contiguous(), nlen[b0:b1].contiguous(), score[b0:b1].contiguous()
                x0, tg, mask, x0r, tgr = cfm.rescore_prep(tk, nl, sc, self.left.embed[0].weight.detach(), pe, self.sos, self.eos,
                                                          embed_r=self.right.embed[0].weight.detach() if two else None)
                args = (mem[b0 * T:b1 * T], mem_mask[b0:b1], b1 - b0, N, Lc, T, prec)
                lp = self._logp(self.left, x0, tg, mask, *args)
                lpr = self._logp(self.right, x0r, tgr, mask, *args) if two else None
                outs.append(cfm.rescore_combine(lp, nl, sc, self.first_pass_weight, self.reverse_weight, logp_r=lpr))
        return outs[0] if len(outs) == 1 else tuple(torch.cat([o[k] for o in outs], 0) for k in range(4))

    def rescore(self, encoder_out, encoder_out_lens, nbest, return_details=False):
        """nbest: the list of per-utterance lists of (tokens, score) that CTCDecoder.prefix_beam_search and greedy.BeamSearch return, or their device
        triple (tokens int32 [B, N, Lmax], nlen int32 [B, N], score f32 [B, N]).  Returns per utterance the same hypotheses re-ranked, best first,
        as (tokens, final); return_details=True: (tokens, final, {"left", "right", "first_pass"})."""
        dev = encoder_out.device
        if isinstance(nbest, (tuple, list)) and len(nbest) == 3 and all(isinstance(t, torch.Tensor) for t in nbest):
            tokens, nlen, score = (t.to(dev) for t in nbest)
            tokens, nlen, score = tokens.to(torch.int32).contiguous(), nlen.to(torch.int32).contiguous(), score.to(torch.float32).contiguous()
        else:
            B = len(nbest)
            N = max([len(u) for u in nbest] + [1])
            Lmax = max([len(t) for u in nbest for t, _ in u] + [1])
            host = torch.zeros((B, N, Lmax + 2), dtype=torch.float64)           # one upload: tokens | length | score
            host[:, :, Lmax], host[:, :, Lmax + 1] = -1.0, float("-inf")
            for b, u in enumerate(nbest):
                for n, (t, s) in enumerate(u):
                    host[b, n, :len(t)] = torch.tensor(t, dtype=torch.float64)
                    host[b, n, Lmax], host[b, n, Lmax + 1] = len(t), s
            d = host.to(dev)
            tokens, nlen, score = d[:, :, :Lmax].to(torch.int32).contiguous(), d[:, :, Lmax].to(torch.int32).contiguous(), d[:, :, Lmax + 1].to(torch.float32).contiguous()
        B, N, Lmax = tokens.shape
        final, left, right, order = self.scores(encoder_out, encoder_out_lens, tokens, nlen, score)
        host = torch.cat([t.to(torch.float64).reshape(B, N, -1) for t in (final, left, right, order, nlen, score, tokens)], 2).cpu()      # the one host read
        out = []
        for b in range(B):
            rows = []
            for r in range(N):
                n = int(host[b, r, 3])
                f, l, rt, _, ln, sc = host[b, n, :6].tolist()
                if ln < 0 or sc == float("-inf"):
                    continue
                tk = [int(v) for v in host[b, n, 6:6 + int(ln)].tolist()]
                rows.append((tk, f, {"left": l, "right": rt, "first_pass": sc}) if return_details else (tk, f))
            out.append(rows)
        return out


# ------------------------------------------------------------------------------------------------------------------------------------------------
# Autoregressive beam search with the attention decoder: the incremental path (a device K/V cache)
# ------------------------------------------------------------------------------------------------------------------------------------------------
class _DecoderWeights:
    """What greedy._Search asks of a head, for a search that has no predictor and no joint: the identity of the decoder's weights (with the
    precision mode: the packs differ)."""

    def __init__(self, owner, dec):
        self.owner, self.dec = owner, dec

    def weights_key(self):
        return packing.weights_key(list(self.dec.parameters()), cfm.resolve_precision(self.owner).name)


class AttentionBeamSearch(_Search):
    """Decoding with the attention decoder alone: per utterance the `beam` best token strings with their scores s(y) = sum of the token
    log-probabilities, eos included -- the quantity AttentionRescorer's left decoder assigns -- no length normalisation.  Specified in float64,
    without a cache, in tests/attention_search_ref.py; a BiTransformerDecoder searches with its left decoder.  Eval mode only, device only.

    The R = B * beam hypotheses are the rows of one step: per layer cfm.layernorm, the fused q|k|v product, cfm.dec_step_attn over the self-attention
    store (append and attend in one launch), the out-projection with the residual, cfm.layernorm, the q product, cfm.dec_step_attn over the memory's
    keys and values (projected once per utterance and layer before the loop), the out-projection, cfm.layernorm and both feed-forward products; then
    after_norm, the output product, cfm.ctc_topk and cfm.dec_beam_prune.  Position j's K | V is written once, to slot j * R + (the row at step
    j) of a [layers][max_len * R][2 D] store, and never moved: a row carries its ancestry as a table of slots, and pruning reorders only that.
    `steps_per_replay` steps are captured in one HIP graph; the host reads one done flag per replay.  Weight changes, other shapes and another
    precision mode drop the graph (greedy._Search).

    search(encoder_out [B, T, D], encoder_out_lens (B,)) -> per utterance a list of (tokens, score), best first, sos / eos stripped; an utterance
    without frames gives [([], 0.0)].  max_len: the most steps (default: the utterance's frames); a hypothesis cut off there is returned unfinished,
    its score without an eos term.  return_device=True: (that list, (tokens int32 [B, beam, Lmax], lengths int32 [B, beam], scores f32 [B, beam])),
    the triple AttentionRescorer.scores / rescore take.  Limits: 1 <= beam <= 16, beam <= V, B * beam <= 1024, max_len <= 1023, T <= 2048."""

    _SNAP = ("score", "token", "parent", "finished", "hlen", "klen", "tokens", "slots", "x", "step", "done", "n_done", "all_done", "nbest_tokens", "nbest_len",
             "nbest_score")      # what a step changes (packing.capture_step); the self-attention store is written at a position before it is read
    _who = "AttentionBeamSearch"

    def __init__(self, decoder, beam=10, sos=None, eos=None, max_len=None, steps_per_replay=8, use_graph=True):
        if isinstance(decoder, BiTransformerDecoder):
            left = decoder.left_decoder
        elif isinstance(decoder, TransformerDecoder):
            left = decoder
        else:
            raise TypeError("AttentionBeamSearch: decoder is a TransformerDecoder or a BiTransformerDecoder, got %s" % type(decoder).__name__)
        super().__init__(None, None, 0, steps_per_replay, use_graph, head=_DecoderWeights(decoder, left))
        self.decoder, self.left = decoder, left
        V = left.output_layer.out_features
        self.beam, self.max_len = int(beam), None if max_len is None else int(max_len)
        self.sos = V - 1 if sos is None else int(sos)
        self.eos = V - 1 if eos is None else int(eos)
        if not 1 <= self.beam <= 16:
            raise ValueError("AttentionBeamSearch: beam = %d outside 1..16 (the top-k launch returns at most 16 classes)" % self.beam)
        if self.beam > V:
            raise ValueError("AttentionBeamSearch: beam = %d above the vocabulary's %d classes" % (self.beam, V))
        if self.max_len is not None and not 1 <= self.max_len <= 1023:
            raise ValueError("AttentionBeamSearch: max_len = %d outside 1..1023" % self.max_len)
        if not (0 <= self.sos < V and 0 <= self.eos < V) or self.steps_per_replay < 1:
            raise ValueError("AttentionBeamSearch: sos and eos inside the vocabulary, steps_per_replay positive")
        self._S = self._key = None
        self.steps = self.replays = 0

    def _state(self, B, T, Lmax, dev, prec):
        left, K = self.left, self.beam
        R, D, n_layers = B * K, left.output_layer.in_features, len(left.decoders)
        z = lambda dt, *s: torch.zeros(s, dtype=dt, device=dev)
        f32, i32, u8 = torch.float32, torch.int32, torch.uint8
        return dict(lens=z(i32, B), max_len=z(i32, B), score=z(f32, R), token=z(i32, R), parent=z(i32, R), finished=z(u8, R), hlen=z(i32, R), klen=z(i32, R),
                    tokens=z(i32, R, Lmax), slots=z(i32, R, Lmax), x=z(f32, R, D), step=z(i32, B), done=z(u8, B), n_done=z(i32, 1), all_done=z(i32, 1),
                    nbest_tokens=z(i32, B, K, Lmax), nbest_len=z(i32, B, K), nbest_score=z(f32, B, K), rows=torch.full((1,), R, dtype=i32, device=dev),
                    self_kv=z(prec.act_dtype, n_layers, Lmax * R, 2 * D), mem_kv=z(prec.act_dtype, n_layers, B * T, 2 * D))

    def _begin(self, S, lens, Lmax):
        """The live set [sos] at score 0 in the first row of every utterance (the other rows: score -inf), an utterance without frames done."""
        K, dev = self.beam, lens.device
        R, D = S["score"].shape[0], S["x"].shape[1]
        S["score"].fill_(float("-inf"))
        S["score"][::K] = 0.0
        S["token"].fill_(self.sos)
        S["parent"].copy_(torch.arange(R, dtype=torch.int32, device=dev))
        for k in ("finished", "hlen", "tokens", "slots", "step", "nbest_tokens", "nbest_len"):
            S[k].zero_()
        S["klen"].fill_(1)
        S["slots"][:, 0] = S["parent"]
        S["max_len"].copy_(lens.clamp(max=Lmax) if self.max_len is None else torch.where(lens > 0, torch.full_like(lens, Lmax), torch.zeros_like(lens)))
        done = lens <= 0
        S["done"].copy_(done.to(torch.uint8))
        S["n_done"].copy_(done.sum().to(torch.int32).reshape(1))
        S["all_done"].copy_((S["n_done"] >= lens.shape[0]).to(torch.int32))
        S["nbest_score"].fill_(float("-inf"))
        S["nbest_score"][:, 0] = torch.where(done, 0.0, float("-inf"))
        E = self.left.embed[0].weight.detach()
        S["x"].copy_((E[self.sos].double() * math.sqrt(D) + self.left.position_table(Lmax + 1)[0].double()).float().expand(R, D))

    def _prepare(self, S, encoder_out, T):
        """What a subclass derives from the encoder output once per search, before _begin (JointBeamSearch: the CTC head's log-probabilities)."""

    def _step(self):
        S, left, prec = self._S, self.left, self._prec
        K, H = self.beam, left.decoders[0].self_attn.num_heads
        x = S["x"]
        (R, D), dev, adt = x.shape, x.device, prec.act_dtype
        B, T = S["lens"].shape[0], S["mem_kv"].shape[1] // S["lens"].shape[0]
        buf = lambda tag, dt, *shape: cfm.scratch("att_search_" + tag, int(torch.Size(shape).numel()), dt, dev).view(*shape)
        xn, ctx, q = buf("xn", adt, R, D), buf("ctx", adt, R, D), buf("q", adt, R, D)
        qkv = buf("qkv", adt, R, 3 * D)
        for l, layer in enumerate(left.decoders):
            pk = packing.pack_mhsa(layer.self_attn, prec, False)
            cfm.layernorm(x, layer.norm1.weight, layer.norm1.bias, out1=xn)
            cfm.gemm(xn, pk.qkv_w, bias=pk.qkv_b, w_lo=pk.qkv_w_lo, out=qkv)
            cfm.dec_step_attn(qkv[:, :D], S["self_kv"][l], H, klen=S["klen"], slot=S["slots"], kv_new=qkv[:, D:], out=ctx)
            cfm.gemm(ctx, pk.out_w, bias=pk.out_b, w_lo=pk.out_w_lo, residual=x, out=x)
            pk = packing.pack_mhsa(layer.src_attn, prec, False)
            cfm.layernorm(x, layer.norm2.weight, layer.norm2.bias, out1=xn)
            cfm.gemm(xn, pk.q_w, bias=pk.q_b, w_lo=pk.q_w_lo, out=q)
            cfm.dec_step_attn(q, S["mem_kv"][l], H, klen=S["lens"], out=ctx, group=K, stride=T)
            cfm.gemm(ctx, pk.out_w, bias=pk.out_b, w_lo=pk.out_w_lo, residual=x, out=x)
            pf = packing.pack_ffn(layer.feed_forward, prec)
            cfm.layernorm(x, layer.norm3.weight, layer.norm3.bias, out1=xn)
            hid = cfm.gemm(xn, pf.w1, bias=pf.b1, w_lo=pf.w1_lo, act=cfm.ACT_RELU, out=buf("hid", adt, R, pf.w1.shape[0]))
            cfm.gemm(hid, pf.w2, bias=pf.b2, w_lo=pf.w2_lo, residual=x, out=x)
        cfm.layernorm(x, left.after_norm.weight, left.after_norm.bias, out1=xn)
        po = left._output_pack(prec)
        logits = cfm.gemm(xn, po.w, bias=po.b, w_lo=po.w_lo, out=buf("logits", torch.float32, R, po.Vp))
        self._select(logits, po, buf)

    def _select(self, logits, po, buf):
        """The step's f32 logits [R, Vp] to the pruned beam: cfm.ctc_topk and cfm.dec_beam_prune (JointBeamSearch scores the candidates in between)."""
        S, K, R = self._S, self.beam, logits.shape[0]
        top = (buf("topk_idx", torch.int32, 1, R, K), buf("topk_logp", torch.float32, 1, R, K), buf("lse", torch.float32, 1, R))
        cfm.ctc_topk(logits.view(1, R, po.Vp), po.V, S["rows"], K, out=top)                 # the one top-k of the library: B = 1, T = R
        cfm.dec_beam_prune(top[0].view(R, K), top[1].view(R, K), S, self.left.embed[0].weight.detach(), self._pe, self.eos, po.V)

    def _run_steps(self):
        for _ in range(self.steps_per_replay):
            self._step()

    @torch.no_grad()
    def search(self, encoder_out, encoder_out_lens, return_device=False):
        if self.decoder.training:
            raise RuntimeError("%s is an eval-mode operation (the decoder's dropout would be live); call .eval()" % self._who)
        if encoder_out.dim() != 3 or encoder_out.shape[2] != self.left.output_layer.in_features:
            raise ValueError("%s: encoder_out must be [B, T, %d], got %s" % (self._who, self.left.output_layer.in_features, tuple(encoder_out.shape)))
        (B, T, D), K, dev = encoder_out.shape, self.beam, encoder_out.device
        Lmax = max(T, 1) if self.max_len is None else self.max_len
        if B < 1 or B * K > 1024:
            raise ValueError("%s: B * beam = %d * %d rows, one step takes 1..1024" % (self._who, B, K))
        if Lmax > 1023:
            raise ValueError("%s: max_len defaults to the %d encoder frames, above the 1023 steps a search takes; pass max_len" % (self._who, T))
        if T > 2048:
            raise ValueError("%s: %d encoder frames, cfm_dec_step_attn attends to at most 2048 keys" % (self._who, T))
        cfm.require_hip(encoder_out)
        prec = cfm.resolve_precision(self.decoder)
        self._sync_weights()
        key = (B, T, K, Lmax, str(dev), prec.name)
        if self._key != key:                                                            # new buffers: the graph holds their addresses
            self._S, self._key = self._state(B, T, Lmax, dev, prec), key
            self._drop()
        S, self._prec = self._S, prec
        self._pe = self.left.position_table(Lmax + 1)
        lens = torch.as_tensor(encoder_out_lens).to(device=dev, dtype=torch.int32).reshape(B).clamp(0, T)
        S["lens"].copy_(lens)
        if T > 0:
            mem = encoder_out.detach().to(torch.float32).reshape(B * T, D).contiguous()
            for l, layer in enumerate(self.left.decoders):                                  # the memory's keys and values: once per utterance and layer
                pk = packing.pack_mhsa(layer.src_attn, prec, False)
                cfm.gemm(mem, pk.qkv_w[D:], bias=pk.qkv_b[D:], w_lo=None if pk.qkv_w_lo is None else pk.qkv_w_lo[D:], out=S["mem_kv"][l])
        self._prepare(S, encoder_out, T)
        self._begin(S, lens, Lmax)
        self.replays = 0 if bool(S["all_done"]) else self._replay(S, self._SNAP, lambda: bool(S["all_done"]), Lmax // self.steps_per_replay + 2)
        out = _nbest_lists(S["nbest_tokens"], S["nbest_len"], S["nbest_score"], range(B))
        self.steps = int(S["step"].max()) + 1 if self.replays else 0
        return (out, (S["nbest_tokens"].clone(), S["nbest_len"].clone(), S["nbest_score"].clone())) if return_device else out


# ------------------------------------------------------------------------------------------------------------------------------------------------
# Joint CTC/attention decoding: the attention beam search with the CTC head's prefix probabilities (csrc/ctc_prefix.hip)
# ------------------------------------------------------------------------------------------------------------------------------------------------
class _JointWeights(_DecoderWeights):
    """Both heads' weights: a change to the CTC projection drops the graph as a change to the decoder does."""

    def __init__(self, owner, dec, ctc):
        super().__init__(owner, dec)
        self.ctc = ctc

    def weights_key(self):
        return super().weights_key() + packing.weights_key(list(self.ctc.parameters()), cfm.resolve_precision(self.ctc).name)


class JointBeamSearch(AttentionBeamSearch):
    """Joint CTC/attention decoding: AttentionBeamSearch in which every candidate extension is also scored by the CTC head's prefix probability.
    An unfinished hypothesis g offers class c at

        (1 - ctc_weight) * logp_att(c) + ctc_weight * (psi(g.c) - psi(g)),      psi(h) = log P_ctc(the output starts with h),  psi(g.eos) = log P_ctc(g)

    so a finished hypothesis scores (1 - ctc_weight) * (the attention decoder's s(y)) + ctc_weight * (minus the CTC loss of y).  Specified in float64
    in tests/ctc_prefix_ref.py; include/cfm.h states the kernels.  Each row's `pre_beam` best attention classes are its candidates (beam <= pre_beam
    <= min(16, V); default min(16, V, ceil(1.5 beam))); per row the `beam` best by the combined offer go to the prune, which is unchanged.

    Once per search the CTC head's logits (CTCDecoder's packed projection, no dropout) become class-major log-probabilities (cfm.ctc_logprob_t,
    B * V * Tp * 4 bytes); per step cfm.ctc_topk (k = pre_beam), cfm.ctc_prefix_score, cfm.dec_beam_prune and cfm.ctc_prefix_advance, which carries
    each kept row's CTC state (2 * R * Tp * 8 bytes, double-buffered by step parity) from its parent's.  search() returns what
    AttentionBeamSearch.search returns, the scores being the combined ones; there is no length normalisation.  eos != blank."""

    _SNAP = AttentionBeamSearch._SNAP + ("ctc_state", "ctc_psi")
    _who = "JointBeamSearch"

    def __init__(self, decoder, ctc, beam=10, ctc_weight=0.3, pre_beam=None, blank=0, sos=None, eos=None, max_len=None, steps_per_replay=8, use_graph=True):
        super().__init__(decoder, beam=beam, sos=sos, eos=eos, max_len=max_len, steps_per_replay=steps_per_replay, use_graph=use_graph)
        if not isinstance(ctc, CTCDecoder):
            raise TypeError("JointBeamSearch: ctc is a CTCDecoder, got %s" % type(ctc).__name__)
        V = self.left.output_layer.out_features
        if ctc.ctc_lo.out_features != V:
            raise ValueError("JointBeamSearch: the CTC head has %d classes, the attention decoder %d" % (ctc.ctc_lo.out_features, V))
        if ctc.ctc_lo.in_features != self.left.output_layer.in_features:
            raise ValueError("JointBeamSearch: the CTC head reads %d features, the attention decoder's memory has %d" %
                             (ctc.ctc_lo.in_features, self.left.output_layer.in_features))
        self.ctc, self.ctc_weight, self.blank = ctc, float(ctc_weight), int(blank)
        if not 0.0 < self.ctc_weight <= 1.0:
            raise ValueError("JointBeamSearch: ctc_weight = %r outside (0, 1] (0 is AttentionBeamSearch)" % (ctc_weight,))
        self.pre_beam = min(16, V, -(-3 * self.beam // 2)) if pre_beam is None else int(pre_beam)
        if not self.beam <= self.pre_beam <= min(16, V):
            raise ValueError("JointBeamSearch: pre_beam = %d outside beam = %d .. min(16, V) = %d" % (self.pre_beam, self.beam, min(16, V)))
        if not 0 <= self.blank < V or self.blank == self.eos:
            raise ValueError("JointBeamSearch: blank = %d inside the vocabulary and different from eos = %d" % (self.blank, self.eos))
        self._head = _JointWeights(decoder, self.left, ctc)

    def _state(self, B, T, Lmax, dev, prec):
        S = super()._state(B, T, Lmax, dev, prec)
        V, R, Tp = self.left.output_layer.out_features, B * self.beam, (T + 3) // 4 * 4
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        S.update(ctc_x=z(B, V, Tp), ctc_state=z(2, R, Tp, 2), ctc_psi=z(R))
        return S

    def search(self, encoder_out, encoder_out_lens, return_device=False):
        if self.ctc.training:
            raise RuntimeError("JointBeamSearch is an eval-mode operation (inference only); call .eval() on the CTC head")
        return super().search(encoder_out, encoder_out_lens, return_device)

    def _prepare(self, S, encoder_out, T):
        if T > 0:
            pk = self.ctc._weights(cfm.resolve_precision(self.ctc))
            cfm.ctc_logprob_t(CTCDecoder._logits(encoder_out.detach(), pk), pk.V, S["lens"], out=S["ctc_x"])

    def _begin(self, S, lens, Lmax):
        """Every row starts as the empty prefix, in half 0 (step 0): gamma_n = -inf, gamma_b the running sum of the blank column, psi = 0."""
        super()._begin(S, lens, Lmax)
        T = S["mem_kv"].shape[1] // lens.shape[0]
        S["ctc_psi"].zero_()
        if T > 0:
            # the running sum also covers columns t >= lens[b] of ctc_x, which hold zeros or an earlier search's values, and half 1 is left as it
            # was: the kernels read frames t < lens[b] of the half the step counter names, nothing else
            S["ctc_state"][0, :, :, 0] = float("-inf")
            S["ctc_state"][0, :, :T, 1] = S["ctc_x"][:, self.blank, :T].cumsum(-1).repeat_interleave(self.beam, 0)

    def _select(self, logits, po, buf):
        S, K, P, R = self._S, self.beam, self.pre_beam, logits.shape[0]
        T = S["mem_kv"].shape[1] // S["lens"].shape[0]
        top = (buf("pre_idx", torch.int32, 1, R, P), buf("pre_logp", torch.float32, 1, R, P), buf("lse", torch.float32, 1, R))
        cfm.ctc_topk(logits.view(1, R, po.Vp), po.V, S["rows"], P, out=top)
        out = (buf("topk_idx", torch.int32, R, K), buf("topk_logp", torch.float32, R, K), buf("cand_psi", torch.float32, R, K))
        cfm.ctc_prefix_score(S["ctc_x"], T, S["ctc_state"], S["ctc_psi"], top[0].view(R, P), top[1].view(R, P), S, K, self.ctc_weight, self.blank, self.eos, out=out)
        cfm.dec_beam_prune(out[0], out[1], S, self.left.embed[0].weight.detach(), self._pe, self.eos, po.V)
        cfm.ctc_prefix_advance(S["ctc_x"], T, S["ctc_state"], S["ctc_psi"], S, K, self.blank, self.eos)
