"""The reference's training objective -- `Transducer.forward` / `rnnt_loss` / `ctc_loss` of src/model.py:71-124 -- over this repository's modules.

    loss = ctc_weight * CTC + transducer_weight * RNN-T                  (model.py:84; train.sh: 0.2 and 0.8)

`TransducerObjective.forward(batch)` takes the reference's 6-tuple batch and returns its dict (model.py:89-93).  The wiring is model.py:95-124:
the predictor reads add_blank(labels) (a blank in front, ignore_id -> blank), the RNN-T targets are where(labels == ignore_id, blank, labels),
the CTC loss is summed.  The joint and the RNN-T loss are one step over a packed lattice (TransducerJoint.rnnt_loss(packed=True); packed=False
selects the padded joint).

`forward_window(micro_batches)` is the same objective over a whole accumulation window, one loss per micro-batch -- the
`DataParallelTrainer(window_loss_fn=...)` form: ConformerEncoder.forward_window(return_rows=True), CTCDecoder.forward_window over the row matrix,
the predictor ONCE for the window (label matrices padded to the window's longest with ignore_id; the LSTM is causal, so what a micro-batch's rows
read does not change), and TransducerJoint.forward_window, whose packed lattice spans every micro-batch's valid cells.

`StreamingRecognizer` is the reference's streaming product -- `Transducer.greedy_search_streaming_app` (model.py:178-199) and
`greedy_search_streaming_eval` (:126-165): feature windows (step) or waveform blocks (step_audio) in, tokens out -- for B streams at once, all state on the device.

`OfflineRecognizer` is its whole-utterance product -- `Transducer.greedy_search` (model.py:202-212), the path of predict_step and of the /recognize/
endpoint -- for a ragged batch of utterances at once.
"""
import torch
import torch.nn as nn

import utils


class TransducerObjective(nn.Module):

    def __init__(self, encoder, predictor, joint, ctc, blank=0, ignore_id=-1, ctc_weight=0.0, transducer_weight=1.0, packed=True, attention=None,
                 attention_weight=0.0, lsm_weight=0.0, reverse_weight=0.0):
        """attention: a decoder.TransformerDecoder / BiTransformerDecoder; the objective then adds attention_weight * loss_attn
        (decoder.AttentionLoss with lsm_weight and reverse_weight, model.py:85).  Without it nothing changes."""
        super().__init__()
        self.encoder, self.predictor, self.joint, self.ctc = encoder, predictor, joint, ctc
        self.blank, self.ignore_id = blank, ignore_id
        self.ctc_weight, self.transducer_weight = ctc_weight, transducer_weight
        self.packed = packed
        self.attention_weight = float(attention_weight)
        self.attention_loss = None
        if attention is not None:
            import decoder
            self.attention_loss = decoder.AttentionLoss(attention, lsm_weight=lsm_weight, reverse_weight=reverse_weight, ignore_id=ignore_id)

    def _text(self, labels):
        return torch.where(labels == self.ignore_id, self.blank, labels).to(torch.int32)

    def rnnt_loss(self, encoder_out, encoder_out_lens, padded_labels, label_lengths):
        """model.py:95-113."""
        predictor_out = self.predictor(utils.add_blank(padded_labels, self.blank, self.ignore_id))
        return self.joint.rnnt_loss(encoder_out, predictor_out, self._text(padded_labels), encoder_out_lens.to(torch.int32),
                                    label_lengths.to(torch.int32), blank=self.blank, reduction="mean", packed=self.packed)

    def forward(self, batch):
        _, padded_feats, feats_length, padded_labels, label_lengths, _ = batch
        encoder_out, encoder_mask = self.encoder(padded_feats, feats_length)
        encoder_out_lens = encoder_mask.squeeze(1).sum(1)
        loss_rnnt = self.rnnt_loss(encoder_out, encoder_out_lens, padded_labels, label_lengths)
        loss_ctc = self.ctc(encoder_out, encoder_out_lens, padded_labels, label_lengths).sum()
        loss = self.ctc_weight * loss_ctc + self.transducer_weight * loss_rnnt
        out = {"loss": loss, "loss_ctc": loss_ctc, "loss_rnnt": loss_rnnt, "encoder_out": encoder_out, "encoder_out_lens": encoder_out_lens}
        if self.attention_loss is not None:
            out["loss_attn"] = self.attention_loss(encoder_out, encoder_mask, padded_labels, label_lengths)[0]
            out["loss"] = loss + self.attention_weight * out["loss_attn"]
        return out

    def forward_window(self, micro_batches):
        """The losses of an accumulation window's micro-batches (each the reference's 6-tuple), a 1-D tensor whose entry g equals
        forward(micro_batches[g])["loss"] (train mode; dropout masks differ, as between any two calls)."""
        rows, outs = self.encoder.forward_window([(mb[1], mb[2]) for mb in micro_batches], return_rows=True)
        ctc_groups, shapes = [], []
        for (y, mask), mb in zip(outs, micro_batches):
            B, T = y.shape[0], y.shape[1]
            lens = mask.squeeze(1).sum(1)
            ctc_groups.append((B, T, lens, mb[3], mb[4]))
            shapes.append((B, T, lens))
        loss_ctc = self.ctc.forward_window(rows, ctc_groups)
        labels = [mb[3] for mb in micro_batches]
        Umax = max(lab.size(1) for lab in labels)
        window = torch.cat([nn.functional.pad(lab, (0, Umax - lab.size(1)), value=self.ignore_id) for lab in labels], 0)
        pred = self.predictor(utils.add_blank(window, self.blank, self.ignore_id))              # (sum B_g, Umax + 1, P)
        groups, s = [], 0
        for (B, T, lens), lab, mb in zip(shapes, labels, micro_batches):
            U1 = lab.size(1) + 1
            groups.append((B, T, lens, pred[s:s + B, :U1], self._text(lab), mb[4]))
            s += B
        loss_rnnt = self.joint.forward_window(rows, groups, blank=self.blank)
        loss = self.ctc_weight * loss_ctc + self.transducer_weight * loss_rnnt
        if self.attention_loss is not None:                   # one decoder pass per micro-batch, on its slice of the encoder rows
            attn = [self.attention_loss(y, mask, mb[3], mb[4])[0] for (y, mask), mb in zip(outs, micro_batches)]
            loss = loss + self.attention_weight * torch.stack(attn)
        return loss


def _check_ctc(ctc, encoder, who):
    if ctc is not None and ctc.ctc_lo.in_features != encoder.encoder_dim:
        raise ValueError("%s: the CTC head reads %d encoder features, the encoder gives %d" % (who, ctc.ctc_lo.in_features, encoder.encoder_dim))
    return ctc


def _ctc_stream(ctc, encoder, streams, blank, who):
    if _check_ctc(ctc, encoder, who) is None:
        return None
    import decoder
    return decoder.CTCGreedyStream(ctc, streams, blank=blank)


class StreamingRecognizer:
    """B independent utterances recognised chunk by chunk: `encoder.StreamingBatch` (one batched encoder step, per-stream K/V rings) feeding
    `greedy.ChunkGreedySearch` (chunk-lookahead greedy search, csrc/greedy.hip) on the same stream -- the encoder's output buffer is the
    decoder's input, no torch operation and no host decision in between; per step the host reads one "streams done" counter per graph
    replay of the decoder and, at the end, the new tokens.

    The reference's `greedy_search_streaming_app(chunk, cache, pred_input_step, offset, ...)` maps onto `step`: its encoder caches and
    offset live in the StreamingBatch, its `pred_input_step` / predictor cache in the ChunkGreedySearch (carry=True).  carry=False is
    `greedy_search_streaming_eval`, which restarts the predictor from blank / zeros on every chunk (a quirk of the reference, kept).

    step_audio(samples, lens=None, sample_lens=None, final=None) is step() from the waveform: fbank.StreamingFbank writes the feature windows straight
    into the encoder step's input buffer (fbank_args: its num_mel_bins, dither, seed, ...; the defaults are the reference's settings without dither);
    with sample_lens / final the audio comes in packets of any size and an utterance ends where it ends.  sample_rate (Hz): audio at another rate than
    the fbank's (browser and telephone audio at 48, 44.1, 8 kHz) goes through a resample.StreamingResampler first, state on the device; step_audio then
    takes packets only, at most accepts()[b] source samples of stream b per call.

    step(frames (B, (chunk - 1) * 4 + 7, F), lens=None, frame_lens=None) -> list of B lists: the tokens the step added.

    frame_lens[b] (list or tensor, B entries): the valid FEATURE frames of stream b's window, left-aligned, 0 .. window -- the reference's short final
    chunk (`end = min(cur + decoding_window, num_frames)`, model.py:145-147), legal at any step.  The encoder step is then length-aware end to end
    (encoder.StreamingBatch): stream b gets c_b = ((n_b - 1) // 2 - 1) // 2 encoder frames (0 below 7 feature frames), exactly the reference's batch-1
    forward_chunk on the shorter window, its state advances by c_b, and the decoder reads those c_b frames (`encoder_stream.out_lens`, on the device).
    frame_lens[b] = 0 is an idle stream: nothing of its encoder or decoder state changes, so it needs no reset before it continues.

    lens[b] (without frame_lens): how many of the chunk's encoder frames the DECODER reads for stream b; the encoder still runs and advances the whole
    window.  Giving both raises: frame_lens already fixes the decoder's lengths.

    beam = 1..15 (default None: the greedy decoder above, unchanged): the decoder is `greedy.StreamingBeamSearch`, a beam carried across the chunks
    (streams * beam <= 64; max_frames encoder frames per utterance, max_len tokens per hypothesis; n_steps is its max_symbols).  step / step_audio then
    return the decoder's records (stable, best, nbest); step takes final[b], true where stream b's utterance ends with this step, and step_audio passes
    its own final through -- to the step that runs the utterance's last window.  hyps() is stable + the rest of best per stream, stable_hyps() the part
    that can no longer change, nbest() the n-best list of the streams that are final and done (None for the others)."""

    def __init__(self, encoder, predictor, joint, streams, decoding_chunk_size, num_decoding_left_chunks, blank=0, n_steps=64, carry=True, causal_conv=False,
                 steps_per_replay=8, graph=True, fbank_args=None, ctc=None, beam=None, max_frames=None, max_len=None, sample_rate=None):
        import encoder as encoder_module
        import greedy
        if joint.enc_ffn.in_features != encoder.encoder_dim:
            raise ValueError("StreamingRecognizer: the joint reads %d encoder features, the encoder gives %d" % (joint.enc_ffn.in_features, encoder.encoder_dim))
        self.ctc_decoder = _ctc_stream(ctc, encoder, streams, blank, "StreamingRecognizer")
        self.B, self.chunk = int(streams), int(decoding_chunk_size)
        self.encoder_stream = encoder_module.StreamingBatch(encoder, streams, decoding_chunk_size, num_decoding_left_chunks, causal_conv=causal_conv, graph=graph)
        self.beam = None if beam is None else int(beam)
        if self.beam is None:
            if max_frames is not None or max_len is not None:
                raise ValueError("StreamingRecognizer: max_frames and max_len belong to the beam search (beam=k)")
            self.decoder = greedy.ChunkGreedySearch(predictor, joint, streams, decoding_chunk_size, blank=blank, n_steps=n_steps, steps_per_replay=steps_per_replay,
                                                    use_graph=graph, carry=carry, fused=True)
        else:
            if not carry:
                raise ValueError("StreamingRecognizer: beam search carries the predictor across chunks (carry=False is the greedy decoder's)")
            if max_frames is None:
                raise ValueError("StreamingRecognizer: beam=k needs max_frames, the most encoder frames of an utterance")
            self.decoder = greedy.StreamingBeamSearch(predictor, joint, streams, self.beam, decoding_chunk_size, max_frames, max_len=max_len, blank=blank,
                                                      max_symbols=n_steps, steps_per_replay=steps_per_replay, use_graph=graph)
            self._last = [dict(stable=[], best=([], 0.0), nbest=None) for _ in range(int(streams))]
        self.window = self.encoder_stream.window
        self.encoder_out = None
        self.audio, self.fbank_args = None, dict(fbank_args or {})      # step_audio's fbank.StreamingFbank (made on first use) and its keyword arguments
        self.resampler = None                                           # resample.StreamingResampler when sample_rate is not the fbank's rate
        rate = self.fbank_args.get("sample_frequency", 16000)
        if sample_rate is not None and sample_rate != rate:
            import resample
            if int(rate) != rate:
                raise ValueError("StreamingRecognizer: cannot resample to the fbank's %g Hz, not a whole rate" % rate)
            self.resampler = resample.StreamingResampler(self.B, sample_rate, int(rate), self.encoder_stream.dev)

    def step(self, frames, lens=None, frame_lens=None, final=None):
        if lens is not None and frame_lens is not None:
            raise ValueError("StreamingRecognizer.step: give lens (encoder frames the decoder reads) or frame_lens (feature frames of each window), not both")
        if final is not None and self.beam is None:
            raise ValueError("StreamingRecognizer.step: final belongs to the beam search (beam=k); the greedy decoder has nothing held back")
        self.encoder_out = self.encoder_stream.step(frames, frame_lens)                 # (B, chunk, D), overwritten by the next step
        return self._decode(self.encoder_stream.out_lens if frame_lens is not None else lens, final)

    def _decode(self, lens, final=None):
        """The step's encoder chunk and per-stream lengths to the RNN-T decoder and, when there is a CTC head, to its best-path decoder too."""
        if self.ctc_decoder is not None:
            self.ctc_decoder.decode(self.encoder_out, lens)
        if self.beam is None:
            return self.decoder.decode(self.encoder_out, lens)
        self._last = self.decoder.decode(self.encoder_out, lens, final)
        return self._last

    def step_audio(self, samples, lens=None, sample_lens=None, final=None):
        """step() from the waveform (the reference's deploy.py preprocess_stream + greedy_search_streaming_app): samples (B, n) int16 | float32 on
        the int16 scale, left-aligned.  One fbank launch writes the feature windows into the encoder step's input buffer.

        Whole blocks (no sample_lens, no final): fbank.StreamingFbank.n_next new samples per stream, n_first for a stream that was reset (and then
        for the call: the others read their first n_next); lens[b] as in step().

        Packets of any size: sample_lens[b] >= 0 new samples of stream b (host values: a list or a CPU tensor), final[b] true when its utterance ends
        with them.  A stream runs a whole window once it holds n_first samples, the utterance's short last window when it is final, and idles (no
        state of it changes) otherwise: the windows are those of the reference's greedy_search_streaming_eval loop over the whole utterance
        (model.py:133-147), so features, encoder rows and tokens do not depend on how the audio was cut.  The window lengths go from the fbank kernel
        to the encoder step and the decoder on the device.  A call takes at most audio.accepts()[b] samples of stream b (n_first + n_next - 1 less what it
        holds; more raises ValueError); after the first such call, a call without sample_lens brings samples.shape[1] samples for every stream, and
        lens raises (the window lengths fix what the decoder reads).  The serving loop:

            new = rec.step_audio(block, sample_lens=n, final=last)    # packets as they arrive; last[b] with the last packet of stream b
            while rec.pending():                                     # windows still held back by the one-window-per-call rule
                new = rec.step_audio(block[:, :0], sample_lens=[0] * B, final=last)
            rec.reset(ended)                                         # streams whose utterance is over and no longer pending"""
        ragged = sample_lens is not None or final is not None
        if lens is not None and (ragged or (self.audio is not None and self.audio.schedule is not None)):
            raise ValueError("StreamingRecognizer.step_audio: give lens (encoder frames the decoder reads, whole blocks only) or sample_lens / final "
                             "(packets of any size: the window lengths fix what the decoder reads), not both")
        if self.resampler is not None and not ragged:
            raise ValueError("StreamingRecognizer.step_audio: audio at %d Hz is resampled to %d Hz, and a resampled block is not a whole number of fbank blocks: "
                             "give packets (sample_lens / final), at most accepts() samples per stream" % (self.resampler.orig_freq, self.resampler.new_freq))
        if self.audio is None:
            import fbank
            self.audio = fbank.StreamingFbank(self.B, self.chunk, self.encoder_stream.dev, **self.fbank_args)
        if self.resampler is not None:                                                  # packets at the source rate -> packets at the fbank's rate
            if samples.dim() != 2 or samples.shape[0] != self.B:
                raise ValueError("StreamingRecognizer.step_audio wants (%d, n) samples, got %s" % (self.B, tuple(samples.shape)))
            sample_lens, final = self.resampler.check(sample_lens, final, samples.shape[1])
            for b, (n, room) in enumerate(zip(sample_lens, self.accepts())):            # raises before anything changes
                if n > room:
                    raise ValueError("StreamingRecognizer.step_audio: stream %d is handed %d samples at %d Hz and accepts %d (what its filter bank can take after "
                                     "resampling, a final flush included)" % (b, n, self.resampler.orig_freq, room))
            samples, _, sample_lens = self.resampler.step(samples, sample_lens, final)  # the flushed tail and the end of the utterance arrive together
        self.audio.step(samples, self.encoder_stream.input_buffer(self.audio.fbank.num_mel_bins), sample_lens, final)
        if self.audio.schedule is None:
            self.encoder_out = self.encoder_stream.step_resident()
            return self._decode(lens)
        self.encoder_out = self.encoder_stream.step_resident(self.audio.frame_lens, host_lens=[m for _, m in self.audio.windows])
        if self.beam is None:
            return self._decode(self.encoder_stream.out_lens)
        held = set(self.audio.pending())                                                # an utterance ends with the step that runs its last window
        return self._decode(self.encoder_stream.out_lens, [bool(f) and b not in held for b, f in enumerate(self.audio.schedule.final)])

    def accepts(self):
        """Samples, at the rate the audio arrives at, that each stream can take in the next step_audio(..., sample_lens).  With a resampler: the most
        source samples s whose output, were the packet final, still fits the filter bank -- ceil(n (held + s) / o) <= audio.accepts()[b], where `held`
        are the stream's source samples no emitted block has consumed (at most flush_max output samples' worth)."""
        if self.audio is None:
            import fbank
            self.audio = fbank.StreamingFbank(self.B, self.chunk, self.encoder_stream.dev, **self.fbank_args)
        room = self.audio.accepts()
        if self.resampler is None:
            return room
        rs = self.resampler
        return [max(0, a * rs.o // rs.n - h) for a, h in zip(room, rs.schedule.held())]

    def pending(self):
        """Streams that still hold a window to run (fbank.StreamingFbank.pending): call step_audio with sample_lens 0 until it is empty."""
        return [] if self.audio is None else self.audio.pending()

    def reset(self, streams=None):
        """New utterances on the given streams (all by default): audio carry, encoder position and left context, predictor state and hypotheses."""
        streams = None if streams is None else list(streams)
        self.encoder_stream.reset(streams)
        self.decoder.reset(streams)
        if self.beam is not None:
            for b in (range(self.B) if streams is None else streams):
                self._last[b] = dict(stable=[], best=([], 0.0), nbest=None)
        if self.ctc_decoder is not None:
            self.ctc_decoder.reset(streams)
        if self.audio is not None:
            self.audio.reset(streams)
        if self.resampler is not None:
            self.resampler.reset(streams)

    def hyps(self):
        """Everything emitted per stream since its last reset; beam=k: the stable prefix and the rest of the best live hypothesis (which may still
        change), the best entry of the n-best list once the stream is done."""
        if self.beam is None:
            return self.decoder.hyps()
        return [list(r["stable"]) + list(r["best"][0][len(r["stable"]):]) for r in self._last]

    def stable_hyps(self):
        """beam=k: per stream the common prefix of all live hypotheses -- it only grows, and every entry of the final n-best list begins with it."""
        if self.beam is None:
            raise RuntimeError("StreamingRecognizer.stable_hyps: the recogniser was built without a beam (beam=None): hyps() never changes what it has returned")
        return [list(r["stable"]) for r in self._last]

    def nbest(self):
        """beam=k: per stream [(tokens, score)] best first once its utterance is final and decoded, None until then."""
        if self.beam is None:
            raise RuntimeError("StreamingRecognizer.nbest: the recogniser was built without a beam (beam=None)")
        return [None if r["nbest"] is None else [(list(t), sc) for t, sc in r["nbest"]] for r in self._last]

    def ctc_hyps(self):
        """The CTC head's best-path hypotheses per stream since its last reset (the recogniser was built with ctc=...)."""
        if self.ctc_decoder is None:
            raise RuntimeError("StreamingRecognizer.ctc_hyps: the recogniser was built without a CTC head (ctc=None)")
        return self.ctc_decoder.hyps()


class OfflineRecognizer:
    """Whole utterances in, tokens out, a ragged batch at a time: `ConformerEncoder.forward_utterances` feeding `greedy.BatchedGreedySearch` -- the
    reference's `Transducer.greedy_search` (model.py:202-212: forward_chunk_by_chunk with the lengths in the chunk-size slot, i.e. one forward_chunk
    over the whole utterance, then basic_greedy_search), which it runs at batch 1.  Item b's tokens are those of that batch-1 call on utterance b.

    recognize(feats (B,T,F), lengths (B,)) -> list of B token lists; items shorter than 7 frames (no encoder frame) give [].
    recognize_audio(samples (B,N) int16 | float32 on the int16 scale, lengths (B,) samples, sample_rate=None) -> the same from the waveform, through
    fbank.KaldiFbank (deploy.py preprocess); `fbank`: a KaldiFbank, or None for the reference's settings without dither.  sample_rate (Hz; also on
    recognize_ctc_audio and align_audio): audio at another rate than the fbank's goes through resample.Resampler first, on the device.
    The lengths stay on the device; the only host read is the search's own.  encoder_out / encoder_out_lens: what the last call's search read.
    ctc: a decoder.CTCDecoder on the same encoder; recognize_ctc / recognize_ctc_audio then decode its output instead (the hybrid model's cheap first pass),
    and align / align_audio give a known transcript's token spans in encoder frames (frame_seconds converts a frame to its start time).
    align(..., head="rnnt") aligns on the transducer head instead (TransducerJoint.forced_align; no CTC head needed): per token the frame that emits
    it.  recognize(..., timestamps=True) aligns each utterance's 1-best against itself on that head: {"tokens", "frames", "logp", "score"}.
    score / score_audio recognise and then score the hypotheses against known transcripts on the device (metrics.py, cfm.edit_distance).
    attention: a decoder.TransformerDecoder / BiTransformerDecoder (or a ready decoder.AttentionRescorer) on the same encoder; recognize(beam=k,
    rescore=True), recognize_ctc(beam=k, rescore=True) and their _audio forms then re-rank each n-best list by the attention decoder
    (first_pass_weight, reverse_weight: AttentionRescorer's) and return (tokens, final score) pairs, best first.  recognize_attention /
    recognize_attention_audio decode with the attention decoder itself (decoder.AttentionBeamSearch); with ctc= as well, recognize_joint /
    recognize_joint_audio decode with both heads (decoder.JointBeamSearch).  attention=None changes nothing and adds no launch."""

    def __init__(self, encoder, predictor, joint, blank=0, n_steps=64, fbank=None, ctc=None, attention=None, first_pass_weight=0.5, reverse_weight=0.0,
                 **search_kw):
        import greedy
        if joint.enc_ffn.in_features != encoder.encoder_dim:
            raise ValueError("OfflineRecognizer: the joint reads %d encoder features, the encoder gives %d" % (joint.enc_ffn.in_features, encoder.encoder_dim))
        self.ctc, self.blank = _check_ctc(ctc, encoder, "OfflineRecognizer"), blank
        self.encoder = encoder
        self.search = greedy.BatchedGreedySearch(predictor, joint, blank=blank, n_steps=n_steps, **search_kw)
        self.fbank = fbank
        self.encoder_out = self.encoder_out_lens = self._beam = None
        self._resamplers = {}                                # sample_rate -> resample.Resampler, made on first use
        self.rescorer = self._attention = None               # _attention: decoder.AttentionBeamSearch, made on the first recognize_attention
        self._joint = None                                   # decoder.JointBeamSearch, made on the first recognize_joint
        if attention is not None:
            import decoder
            self.rescorer = attention if isinstance(attention, decoder.AttentionRescorer) else decoder.AttentionRescorer(
                attention, first_pass_weight=first_pass_weight, reverse_weight=reverse_weight)
            if self.rescorer.left.output_layer.in_features != encoder.encoder_dim:
                raise ValueError("OfflineRecognizer: the attention decoder reads %d features, the encoder gives %d" %
                                 (self.rescorer.left.output_layer.in_features, encoder.encoder_dim))

    def _check_rescore(self, rescore, beam, who):
        if rescore and beam is None:
            raise ValueError("OfflineRecognizer.%s: rescore=True re-ranks an n-best list; pass beam=k" % who)
        if rescore and self.rescorer is None:
            raise RuntimeError("OfflineRecognizer.%s: rescore=True, but the recogniser was built without an attention decoder (attention=None)" % who)

    def _align_rnnt(self, labels, label_lengths, who):
        """TransducerJoint.forced_align of the labels on self.encoder_out: the predictor in eval mode over [blank] + labels, as TransducerObjective
        prepares them (padding beyond label_lengths[b] reads as blank; the LSTM is causal, so it changes no valid row)."""
        pr, jn = self.search.predictor, self.search.joint
        if pr.training or jn.training:
            raise RuntimeError("OfflineRecognizer.%s: alignment on the RNN-T head is an eval-mode operation" % who)
        dev, B = self.encoder_out.device, self.encoder_out.shape[0]
        labels, llens = torch.as_tensor(labels).to(dev), torch.as_tensor(label_lengths)
        if labels.dim() != 2 or labels.shape[0] != B or llens.shape != (B,):
            raise ValueError("OfflineRecognizer.%s: %d utterances, but labels %s, label lengths %s" % (who, B, tuple(labels.shape), tuple(llens.shape)))
        valid = torch.arange(labels.shape[1], device=llens.device)[None, :] < llens[:, None]       # built where the lengths are: no transfer back
        text = torch.where(valid.to(dev), labels, self.blank)
        pred_out = pr(utils.add_blank(text, self.blank, -1))
        return jn.forced_align(self.encoder_out, pred_out, text.to(torch.int32), self.encoder_out_lens, llens, blank=self.blank)

    def _timestamps(self, hyps):
        """The hypotheses aligned against themselves on the RNN-T head: per utterance {"tokens", "frames", "logp", "score"}."""
        lens = [len(h) for h in hyps]
        labels = torch.full((len(hyps), max(lens, default=0)), self.blank, dtype=torch.int64)
        for b, h in enumerate(hyps):
            labels[b, :len(h)] = torch.tensor(h, dtype=torch.int64)
        out = []
        for e in self._align_rnnt(labels, lens, "recognize"):
            tokens = [] if e is None else e["tokens"]           # None: no encoder frame, so no token either
            out.append({"tokens": [t[0] for t in tokens], "frames": [t[1] for t in tokens], "logp": [t[2] for t in tokens],
                        "score": float("-inf") if e is None else e["score"]})
        return out

    @torch.no_grad()
    def recognize(self, feats, lengths, beam=None, rescore=False, timestamps=False):
        """beam=None: the greedy search, a list of B token lists.  beam = 1..15: greedy.BeamSearch over groups of at most 64 // beam utterances,
        per utterance a list of (tokens, score), best first; an utterance with no encoder frame gives [([], 0.0)].  rescore=True (with beam): the
        lists re-ranked by the attention decoder, (tokens, final score).
        timestamps=True: each utterance's best hypothesis is aligned against itself on the RNN-T head (the Viterbi path of its own tokens, never
        worse than the path the search took).  beam=None: a list of {"tokens", "frames": the encoder frame that emits each token (frame_seconds
        converts it), "logp": the token's log-probability there, "score": the path's}; an utterance with no encoder frame has empty lists and
        score -inf.  With beam: (the n-best lists as without timestamps, that list for the best entries)."""
        self._check_rescore(rescore, beam, "recognize")
        self.encoder_out, self.encoder_out_lens = self.encoder.forward_utterances(feats, lengths)
        if beam is None:
            hyps = self.search.search(self.encoder_out, self.encoder_out_lens)[0]
            return self._timestamps(hyps) if timestamps else hyps
        import greedy
        if self._beam is None or self._beam.beam != int(beam):
            self._beam = greedy.BeamSearch(self.search.predictor, self.search.joint, beam, blank=self.blank, max_symbols=self.search.n_steps)
        group, out = 64 // self._beam.beam, []
        for b0 in range(0, self.encoder_out.shape[0], group):
            out.extend(self._beam.search(self.encoder_out[b0:b0 + group], self.encoder_out_lens[b0:b0 + group]))
        if rescore:
            out = self.rescorer.rescore(self.encoder_out, self.encoder_out_lens, out)
        return (out, self._timestamps([list(n[0][0]) for n in out])) if timestamps else out

    def _features(self, samples, lengths, sample_rate=None):
        """The waveform batch through the fbank; sample_rate (Hz; None: the fbank's own) other than the fbank's sample_frequency goes through a cached
        resample.Resampler first (deploy.py preprocess :108-110), whose device-side output lengths the fbank reads."""
        if self.fbank is None:
            import fbank
            self.fbank = fbank.KaldiFbank()
        if sample_rate is not None and sample_rate != self.fbank.sample_frequency:
            rs = self._resamplers.get(sample_rate)
            if rs is None:
                import resample
                if int(self.fbank.sample_frequency) != self.fbank.sample_frequency:
                    raise ValueError("OfflineRecognizer: cannot resample to the fbank's %g Hz, not a whole rate" % self.fbank.sample_frequency)
                rs = self._resamplers[sample_rate] = resample.Resampler(sample_rate, int(self.fbank.sample_frequency))
            samples, lengths = rs(samples, lengths)
        return self.fbank(samples, lengths)

    def recognize_audio(self, samples, lengths, beam=None, sample_rate=None, rescore=False, timestamps=False):
        self._check_rescore(rescore, beam, "recognize_audio")
        return self.recognize(*self._features(samples, lengths, sample_rate), beam=beam, rescore=rescore, timestamps=timestamps)

    @torch.no_grad()
    def recognize_ctc(self, feats, lengths, beam=None, rescore=False):
        """The CTC head's hypotheses of the same ragged batch: forward_utterances once, then decoder.CTCDecoder.greedy_search (beam=None: a list
        of B token lists) or prefix_beam_search(beam) (per utterance a list of (tokens, score), best first).  An utterance with no encoder
        frame gives [] (beam: the empty hypothesis alone, [([], 0.0)]).  rescore=True (with beam): re-ranked by the attention decoder."""
        if self.ctc is None:
            raise RuntimeError("OfflineRecognizer.recognize_ctc: the recogniser was built without a CTC head (ctc=None)")
        self._check_rescore(rescore, beam, "recognize_ctc")
        self.encoder_out, self.encoder_out_lens = self.encoder.forward_utterances(feats, lengths)
        if beam is None:
            return self.ctc.greedy_search(self.encoder_out, self.encoder_out_lens, blank=self.blank)
        nbest = self.ctc.prefix_beam_search(self.encoder_out, self.encoder_out_lens, beam=beam, blank=self.blank)
        return self.rescorer.rescore(self.encoder_out, self.encoder_out_lens, nbest) if rescore else nbest

    def recognize_ctc_audio(self, samples, lengths, beam=None, sample_rate=None, rescore=False):
        self._check_rescore(rescore, beam, "recognize_ctc_audio")
        return self.recognize_ctc(*self._features(samples, lengths, sample_rate), beam=beam, rescore=rescore)

    @torch.no_grad()
    def recognize_attention(self, feats, lengths, beam=10, rescore=False):
        """The attention decoder's own hypotheses of the same ragged batch: forward_utterances once, then decoder.AttentionBeamSearch (the left
        decoder searches) over groups of at most 1024 // beam utterances -- per utterance a list of (tokens, score), best first; an utterance with
        no encoder frame gives [([], 0.0)].  rescore=True (a recogniser built with reverse_weight > 0, i.e. with a right decoder): the search's
        device n-best triple goes through the rescorer, so the right decoder re-ranks the left decoder's search; (tokens, final score)."""
        if self.rescorer is None:
            raise RuntimeError("OfflineRecognizer.recognize_attention: the recogniser was built without an attention decoder (attention=None)")
        if rescore and not self.rescorer.reverse_weight > 0.0:
            raise ValueError("OfflineRecognizer.recognize_attention: rescore=True re-ranks the left decoder's search by the right decoder; build the "
                             "recogniser with reverse_weight > 0 (a BiTransformerDecoder)")
        import decoder
        self.encoder_out, self.encoder_out_lens = self.encoder.forward_utterances(feats, lengths)
        if self._attention is None or self._attention.beam != int(beam):
            self._attention = decoder.AttentionBeamSearch(self.rescorer.decoder, beam=beam, sos=self.rescorer.sos, eos=self.rescorer.eos)
        group, out, triples = max(1, 1024 // self._attention.beam), [], []
        for b0 in range(0, self.encoder_out.shape[0], group):
            nbest, triple = self._attention.search(self.encoder_out[b0:b0 + group], self.encoder_out_lens[b0:b0 + group], return_device=True)
            out.extend(nbest)
            triples.append(triple)
        if not rescore:
            return out
        triple = triples[0] if len(triples) == 1 else tuple(torch.cat([t[k] for t in triples], 0) for k in range(3))
        return self.rescorer.rescore(self.encoder_out, self.encoder_out_lens, triple)

    def recognize_attention_audio(self, samples, lengths, beam=10, sample_rate=None, rescore=False):
        return self.recognize_attention(*self._features(samples, lengths, sample_rate), beam=beam, rescore=rescore)

    @torch.no_grad()
    def recognize_joint(self, feats, lengths, beam=10, ctc_weight=0.3, rescore=False):
        """Joint CTC/attention decoding of the same ragged batch: forward_utterances once, then decoder.JointBeamSearch (the left decoder's beam
        search, every candidate also scored by the CTC head's prefix probability) over groups of at most 1024 // beam utterances -- per utterance a
        list of (tokens, combined score), best first; an utterance with no encoder frame gives [([], 0.0)].  rescore=True: as recognize_attention,
        the right decoder re-ranks the search's n-best triple (a recogniser built with reverse_weight > 0)."""
        self._check_joint(rescore, "recognize_joint")
        import decoder
        if self._joint is None or (self._joint.beam, self._joint.ctc_weight) != (int(beam), float(ctc_weight)):
            self._joint = decoder.JointBeamSearch(self.rescorer.decoder, self.ctc, beam=beam, ctc_weight=ctc_weight, blank=self.blank, sos=self.rescorer.sos,
                                                  eos=self.rescorer.eos)
        self.encoder_out, self.encoder_out_lens = self.encoder.forward_utterances(feats, lengths)
        group, out, triples = max(1, 1024 // self._joint.beam), [], []
        for b0 in range(0, self.encoder_out.shape[0], group):
            nbest, triple = self._joint.search(self.encoder_out[b0:b0 + group], self.encoder_out_lens[b0:b0 + group], return_device=True)
            out.extend(nbest)
            triples.append(triple)
        if not rescore:
            return out
        triple = triples[0] if len(triples) == 1 else tuple(torch.cat([t[k] for t in triples], 0) for k in range(3))
        return self.rescorer.rescore(self.encoder_out, self.encoder_out_lens, triple)

    def _check_joint(self, rescore, who):
        if self.ctc is None:
            raise RuntimeError("OfflineRecognizer.%s: the recogniser was built without a CTC head (ctc=None)" % who)
        if self.rescorer is None:
            raise RuntimeError("OfflineRecognizer.%s: the recogniser was built without an attention decoder (attention=None)" % who)
        if rescore and not self.rescorer.reverse_weight > 0.0:
            raise ValueError("OfflineRecognizer.%s: rescore=True re-ranks the left decoder's search by the right decoder; build the recogniser with "
                             "reverse_weight > 0 (a BiTransformerDecoder)" % who)

    def recognize_joint_audio(self, samples, lengths, beam=10, ctc_weight=0.3, sample_rate=None, rescore=False):
        self._check_joint(rescore, "recognize_joint_audio")
        return self.recognize_joint(*self._features(samples, lengths, sample_rate), beam=beam, ctc_weight=ctc_weight, rescore=rescore)

    @torch.no_grad()
    def align(self, feats, lengths, labels, label_lengths, return_path=False, head="ctc"):
        """Forced alignment of known transcripts with the CTC head: forward_utterances once, as recognize_ctc, then
        decoder.CTCDecoder.forced_align.  labels [B, Umax], label_lengths (B,).  Per utterance None (no alignment exists, e.g. no encoder frame
        for a non-empty transcript) or {"score", "tokens": [(token, start_frame, end_frame, logp)]} with inclusive ENCODER frames;
        frame_seconds converts them.
        head="rnnt": on the transducer head instead, the one recognize reads (TransducerJoint.forced_align; works without a CTC head): per
        utterance None (no encoder frame) or {"score", "tokens": [(token, frame, logp)]}, frame the encoder frame that emits the token.  There
        is no state path: return_path raises."""
        if head not in ("ctc", "rnnt"):
            raise ValueError("OfflineRecognizer.align: head must be \"ctc\" or \"rnnt\", got %r" % (head,))
        if head == "rnnt":
            if return_path:
                raise ValueError("OfflineRecognizer.align: return_path belongs to the CTC head (head=\"rnnt\" has frames, not a state path)")
            self.encoder_out, self.encoder_out_lens = self.encoder.forward_utterances(feats, lengths)
            return self._align_rnnt(labels, label_lengths, "align")
        if self.ctc is None:
            raise RuntimeError("OfflineRecognizer.align: the recogniser was built without a CTC head (ctc=None)")
        self.encoder_out, self.encoder_out_lens = self.encoder.forward_utterances(feats, lengths)
        return self.ctc.forced_align(self.encoder_out, self.encoder_out_lens, labels, label_lengths, return_path=return_path)

    def align_audio(self, samples, lengths, labels, label_lengths, return_path=False, sample_rate=None, head="ctc"):
        return self.align(*self._features(samples, lengths, sample_rate), labels, label_lengths, return_path=return_path, head=head)

    @torch.no_grad()
    def score(self, feats, lengths, labels, label_lengths, beam=None, head="rnnt"):
        """Recognise, then score against known transcripts (metrics.py over cfm.edit_distance): head="rnnt" is recognize, head="ctc" recognize_ctc.
        labels [B, Umax] with label_lengths (B,), padding ignored, as for align.  Returns {"hyps": what the recogniser returned, "dist" int32 [B]
        and "counts" int32 [B, 4] = (S, D, I, hits) of each utterance's best hypothesis, on the device, "error_rate": (S + D + I) / reference
        tokens of the batch}; with beam also "oracle": metrics.nbest_errors' per-utterance entries, and "oracle_error_rate"."""
        import metrics
        if head not in ("rnnt", "ctc"):
            raise ValueError("OfflineRecognizer.score: head must be \"rnnt\" or \"ctc\", got %r" % (head,))
        hyps = (self.recognize if head == "rnnt" else self.recognize_ctc)(feats, lengths, beam=beam)
        dev = self.encoder_out.device
        refs = metrics._packed((torch.as_tensor(labels), label_lengths), dev, "OfflineRecognizer.score")
        if refs[0].shape[0] != len(hyps):
            raise ValueError("OfflineRecognizer.score: %d utterances, but labels %s" % (len(hyps), tuple(refs[0].shape)))
        best = hyps if beam is None else [n[0][0] for n in hyps]
        dist, counts = metrics.edit_distance(best, refs, device=dev)
        out = {"hyps": hyps, "dist": dist, "counts": counts, "error_rate": metrics.ErrorRate(dev).add_counts(counts, refs[1].clamp(0, refs[0].shape[1])).compute()}
        if beam is not None:
            out["oracle"] = metrics.nbest_errors(hyps, refs, dev)
            out["oracle_error_rate"] = metrics.oracle_error_rate(hyps, refs, dev, errors=out["oracle"])
        return out

    def score_audio(self, samples, lengths, labels, label_lengths, beam=None, head="rnnt", sample_rate=None):
        return self.score(*self._features(samples, lengths, sample_rate), labels, label_lengths, beam=beam, head=head)

    def frame_seconds(self, frame):
        """Start time in seconds of encoder frame `frame`: the front-end's two stride-2, width-3 convolutions make encoder frame i start at feature
        frame 4 i, and feature frame j starts at sample j * shift of the recogniser's fbank (the reference's 10 ms at 16 kHz when
        none was given).  A token aligned to frames [start, end] spans frame_seconds(start) .. frame_seconds(end + 1)."""
        shift, rate = (self.fbank.shift, self.fbank.sample_frequency) if self.fbank is not None else (160, 16000.0)
        return 4 * frame * shift / rate
