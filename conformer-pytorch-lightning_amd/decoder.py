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
import torch
import torch.nn as nn

import cfm
import token_log
from cfm import packing


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
        self._log = token_log.TokenLog(self.B)

    def reset(self, streams=None):
        """New utterances on the given streams (all by default): no previous class, frame 0, hypotheses emptied."""
        if self.S is None:
            raise RuntimeError("cfm: CTCGreedyStream on %s -- this framework runs on MI355X (HIP) only; there is no CPU path" % self.dev)
        idx = slice(None) if streams is None else torch.as_tensor(list(streams), dtype=torch.long, device=self.dev)
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
        if lens is None:
            lens = torch.full((B,), C, dtype=torch.int32, device=self.dev)
        elif not isinstance(lens, torch.Tensor) and len(lens) != B:
            raise ValueError("CTCGreedyStream.decode: %d lens for %d streams" % (len(lens), B))
        token_log.grow(self.S, ("hyps", "frames", "token_logp"), self._log.most() + C)
        idx, logp, _, lens, V = self.ctc._topk(enc_chunk, lens, 1, "greedy_search")
        cfm.ctc_greedy(idx, logp, lens, V, blank=self.blank, state=self.S)
        rep = torch.cat([self.S["count"], self.S["overflow"].to(torch.int64)]).tolist()
        counts, overflow = rep[:B], rep[B]
        if overflow:
            raise RuntimeError("CTCGreedyStream: a stream emitted more symbols than the hypothesis buffer holds")
        return self._log.take(self.S["hyps"], counts)
