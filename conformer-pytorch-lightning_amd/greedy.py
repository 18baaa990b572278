"""RNN-T greedy search for B streams at once, resident on the device -- the reference's `Transducer.basic_greedy_search`
(src/model.py:215-269) without its host loop.

The reference decodes ONE utterance with a Python `while t < T'` loop: per iteration one LSTM step, one joint evaluation, an argmax and
TWO host synchronisations (`joint_out_max != self.blank`, `.item()`), i.e. it is bound by launch + sync latency ("host-bound").
Here the per-stream control state -- frame index t, the symbols emitted on the current frame, the predictor's input token and LSTM state,
the hypothesis buffer and its length -- lives in device tensors and one decoding step is a fixed sequence of device operations for all B
streams, with the reference's branches turned into selects:

    pred = projection(LSTM(embed(token), state))          the reference recomputes it only after a non-blank; it is a pure function
                                                            of (token, state), which change only then -- recomputing gives the same value
    k    = argmax(ffn_out(tanh(enc_ffn(enc[t]) + pred_ffn(pred))))      (log_softmax dropped: monotone)
    non-blank:  append k, token <- k, state <- the LSTM's new state, per-frame count + 1
    blank, or per-frame count == n_steps:  t + 1, per-frame count <- 0      (model.py:262-267, including the quirk that a frame left because of
                                                                            the cap keeps "previous output was non-blank")
    a stream with t == T'_b is finished and no longer changes.

`steps_per_replay` such steps are captured in ONE HIP graph; the host replays it and looks at a single "all finished" flag per replay -- one
synchronisation per `steps_per_replay` steps instead of two per step, and B streams share every weight read.  `enc_ffn` is applied to all
frames once (model.py:250 does it per step).  Everything runs in float32 torch operations on the reference's own parameters (the joint
and the predictor are tiny here: one row per stream); the result is the reference's token sequence per stream wherever the two best logits
of a decision are further apart than f32 rounding (DESIGN.md's margin rule) -- tests compare with the oracle's restatement of the loop, with
tokens produced by running the reference's predictor / joint modules, and with a float64 restatement of the step (tests/greedy_ref.py).

`BatchedGreedySearch` decides one frame per step, `ChunkGreedySearch` (the streaming recogniser's decoder) all remaining frames of a chunk;
`BeamSearch` is the RNN-T beam search on the same packs (n-best lists with scores, device only), `StreamingBeamSearch` carries its beam across
chunks as `ChunkGreedySearch` carries the greedy hypothesis.  Shared, once: `_Head` (weights key, f32 packs, padded vocabulary, limits, LSTM step),
the base `_Search` (eval guard, "weights or buffers changed -> drop descriptor(s) and graph", capture then replay), the beam helpers, token_log.py.
"""
import ctypes

import torch
import torch.nn.functional as F

import cfm
import token_log
from cfm import packing


class _Head:
    """What both searches need of one (predictor, joint) pair: the identity of its weights, their f32 packs for csrc/greedy.hip, the limits
    of the fused steps, the weight half of either ctypes descriptor and the LSTM step as torch operations."""

    def __init__(self, predictor, joint):
        self.predictor, self.joint = predictor, joint
        self._packs = packing.Slot()

    def weights_key(self):
        """Identity of the current weights: packing.weights_key over the predictor's and the joint's parameters."""
        return packing.weights_key(list(self.predictor.parameters()) + list(self.joint.parameters()))

    def padded_vocab(self):
        return (self.joint.ffn_out.out_features + 15) // 16 * 16                        # whole 16-class tiles: the out_w / out_b packs' rows, every per-class buffer's width

    def fused_limits(self, B, dev, chunk=None):
        """None when the fused step takes B streams on dev, else what it needs; chunk: the lookahead step's frames (it also applies enc_ffn)."""
        pr, jn = self.predictor, self.joint
        dims = (pr.embed_size, pr.hidden_size, pr.projection.out_features, jn.pred_ffn.out_features) + (() if chunk is None else (jn.enc_ffn.in_features,))
        if (dev.type == "cuda" and B <= 64 and (chunk is None or chunk <= 32) and pr.num_layers <= 4 and all(d % 16 == 0 for d in dims) and pr.rnn.bias and
                jn.pred_ffn.in_features == pr.projection.out_features):
            return None
        return ("the fused greedy step needs a GPU, <= 64 streams, %s<= 4 LSTM layers with biases and dimensions that are multiples of 16 (there is no "
                "fallback)" % ("" if chunk is None else "chunk <= 32, "))

    def packs(self, dev, enc_ffn=False):
        """f32 packs for csrc/greedy.hip, rebuilt when the weights change (weights_key): [W_ih | W_hh] per layer with rows ordered [unit][gate],
        b_ih + b_hh likewise, the vocabulary projection padded to a multiple of 16 rows (bias -inf there: never the argmax).  enc_ffn: also
        ef_w / ef_b, which only the chunk-lookahead step reads -- added on request, so that the single-frame search holds no copy of them."""
        pr, jn = self.predictor, self.joint
        f32 = lambda t: t.detach().float().contiguous()

        def build():
            H = pr.hidden_size
            perm = (torch.arange(H, device=dev)[:, None] + H * torch.arange(4, device=dev)[None, :]).reshape(-1)     # row u*4 + gate <- gate*H + u
            W = {"embed": f32(pr.embed.weight), "lstm_w": [], "lstm_b": []}
            for l in range(pr.num_layers):
                w = torch.cat([getattr(pr.rnn, "weight_ih_l%d" % l).detach().float(), getattr(pr.rnn, "weight_hh_l%d" % l).detach().float()], 1)
                b = getattr(pr.rnn, "bias_ih_l%d" % l).detach().float() + getattr(pr.rnn, "bias_hh_l%d" % l).detach().float()
                W["lstm_w"].append(w[perm].contiguous())
                W["lstm_b"].append(b[perm].contiguous())
            V, Vp = jn.ffn_out.out_features, self.padded_vocab()
            ow = torch.zeros((Vp, jn.ffn_out.in_features), device=dev)
            ow[:V] = jn.ffn_out.weight.detach().float()
            ob = torch.full((Vp,), float("-inf"), device=dev)
            ob[:V] = jn.ffn_out.bias.detach().float()
            W.update(proj_w=f32(pr.projection.weight), proj_b=f32(pr.projection.bias), pf_w=f32(jn.pred_ffn.weight), pf_b=f32(jn.pred_ffn.bias), out_w=ow, out_b=ob, Vp=Vp)
            return W
        W = self._packs.get((self.weights_key(), str(dev)), build)
        if enc_ffn and "ef_w" not in W:
            W.update(ef_w=f32(jn.enc_ffn.weight), ef_b=f32(jn.enc_ffn.bias))
        return W

    def fill_weights(self, d, W):
        """The weight pointers and the dimensions that come with them, in a cfm.GreedyDesc or cfm.GreedyChunkDesc d."""
        pr, jn = self.predictor, self.joint
        for l in range(pr.num_layers):
            d.lstm_w[l], d.lstm_b[l] = W["lstm_w"][l].data_ptr(), W["lstm_b"][l].data_ptr()
        for k in ("embed", "proj_w", "proj_b", "pf_w", "pf_b", "out_w", "out_b") + (("ef_w", "ef_b") if hasattr(d, "ef_w") else ()):
            setattr(d, k, W[k].data_ptr())
        d.L, d.E, d.H, d.P, d.J, d.Vp = pr.num_layers, pr.embed_size, pr.hidden_size, pr.projection.out_features, jn.pred_ffn.out_features, W["Vp"]

    def lstm_step(self, x, h, c):
        """One LSTM step on (B, E) inputs with nn.LSTM's parameters (eval mode: no inter-layer dropout); torch.nn.LSTM restated for T = 1."""
        rnn = self.predictor.rnn
        hs, cs = [], []
        for l in range(rnn.num_layers):
            w_ih, w_hh = getattr(rnn, "weight_ih_l%d" % l), getattr(rnn, "weight_hh_l%d" % l)
            b_ih, b_hh = (getattr(rnn, "bias_ih_l%d" % l), getattr(rnn, "bias_hh_l%d" % l)) if rnn.bias else (None, None)
            gates = F.linear(x, w_ih, b_ih) + F.linear(h[l], w_hh, b_hh)
            i, f, g, o = gates.chunk(4, dim=-1)
            c1 = torch.sigmoid(f) * c[l] + torch.sigmoid(i) * torch.tanh(g)
            x = torch.sigmoid(o) * torch.tanh(c1)
            hs.append(x)
            cs.append(c1)
        return x, torch.stack(hs), torch.stack(cs)


def replay_until_done(graph, run, done, limit):
    """graph.replay() (no graph: run()) until done(), the one host synchronisation per replay; returns the replays it took, raises at limit."""
    for n in range(1, limit + 1):
        if graph is not None:
            graph.replay()
        else:
            run()
        if done():
            return n
    raise RuntimeError("greedy search did not finish within its step bound")


class _Search:
    """The host bookkeeping of the searches.  Descriptor(s) and graph hold addresses of packs and state buffers: whoever replaces either
    calls _drop().  A subclass has _run_steps() (the steps of one replay) and keeps its descriptor in _desc, or one per step parity in _descs."""

    def __init__(self, predictor, joint, blank, steps_per_replay, use_graph, even_steps=False, head=None):
        """head: what stands for the weights -- an object with weights_key(); default: _Head(predictor, joint).  A search without a predictor and
        a joint (decoder.AttentionBeamSearch) passes its own, None for both, and guards train mode itself."""
        self.predictor, self.joint, self._head = predictor, joint, _Head(predictor, joint) if head is None else head
        self.blank, self.use_graph, self._key_w, self._enc_keep = int(blank), bool(use_graph), None, None
        self.steps_per_replay = int(steps_per_replay) + (int(steps_per_replay) & 1 if even_steps else 0)       # even: the beam searches' step parity
        self._drop()

    def _require_eval(self, who):
        if self.predictor.training or self.joint.training:
            raise RuntimeError("%s is an eval-mode operation (the predictor's dropout would be live)" % who)

    def _drop(self):
        self._graph = self._desc = self._descs = None

    def _sync_weights(self):
        """New weights (_Head.weights_key): descriptor(s) and graph go; the packs are rebuilt by their own key."""
        wkey = self._head.weights_key()
        if self._key_w != wkey:
            self._key_w = wkey
            self._drop()

    def _replay(self, S, snap, done, limit):
        """_run_steps captured in a graph (packing.capture_step) when one is wanted and missing (snap: what the steps change in S; the graph holds
        the addresses of S's tensors, the packs and the descriptor), then replay_until_done."""
        if self.use_graph and self._graph is None and S["token"].is_cuda:
            self._graph, _ = packing.capture_step(self._run_steps, S["token"].device, [S[k] for k in snap])
        return replay_until_done(self._graph, self._run_steps, done, limit)

    def _f32_chunk(self, enc_chunk):
        """enc_chunk as contiguous float32 -- itself when it is --, kept alive while a descriptor holds its address."""
        self._enc_keep = enc_chunk if (enc_chunk.dtype == torch.float32 and enc_chunk.is_contiguous()) else enc_chunk.float().contiguous()
        return self._enc_keep


class BatchedGreedySearch(_Search):

    def __init__(self, predictor, joint, blank=0, n_steps=64, steps_per_replay=32, use_graph=True, fused=None):
        """fused: one step = six HIP launches on f32 weights (csrc/greedy.hip, include/cfm.h cfm_greedy_step) instead of ~45 torch operations;
        default: on an MI355X when the sizes fit (B <= 64 streams, dimensions multiples of 16), the torch-operation form otherwise (and on CPU)."""
        super().__init__(predictor, joint, blank, steps_per_replay, use_graph)
        self.n_steps, self.fused, self._S, self._key = int(n_steps), fused, None, None

    # -- fused step (_fused_ok / _fused_weights: what tests/test_greedy_step_gpu.py builds a step from) -----------------------------------------
    def _fused_ok(self, B, dev):
        return self._head.fused_limits(B, dev) is None

    def _fused_weights(self, dev):
        return self._head.packs(dev)

    def _fused_desc(self, S, W, B, T):
        pr, jn = self.predictor, self.joint
        L, H = pr.num_layers, pr.hidden_size
        dev = S["t"].device
        for k, shape, dt in (("h_new", (L, B, H), torch.float32), ("c_new", (L, B, H), torch.float32), ("pred", (B, pr.projection.out_features), torch.float32),
                             ("act", (B, jn.pred_ffn.out_features), torch.float32), ("pmax", (W["Vp"] // 16, B), torch.float32),
                             ("pidx", (W["Vp"] // 16, B), torch.int32), ("done8", (B,), torch.uint8), ("n_done", (1,), torch.int32)):
            if k not in S:
                S[k] = torch.zeros(shape, dtype=dt, device=dev)
        d = cfm.GreedyDesc()
        self._head.fill_weights(d, W)
        for k in ("enc_proj", "token", "t", "count", "frame_count", "hyps", "lens", "h", "c", "h_new", "c_new", "pred", "act", "pmax", "pidx", "n_done"):
            setattr(d, k, S[k].data_ptr())
        d.done = S["done8"].data_ptr()
        d.hyp_cap, d.hyp_ld = int(S["cap"][0]), S["hyps"].shape[1]
        d.B, d.T, d.blank, d.n_steps = B, T, self.blank, self.n_steps
        return d

    # -- one step as torch operations (the CPU form, and the GPU's beyond the fused step's limits) ---------------------------------------------
    def _step(self, S):
        ar = S["ar"]
        e = S["enc_proj"][ar, torch.minimum(S["t"], S["tmax"])]                       # (B, J): the frame each stream is on
        y, h1, c1 = self._head.lstm_step(self.predictor.embed(S["token"]), S["h"], S["c"])
        pred = self.predictor.projection(y)
        z = self.joint.ffn_out(torch.tanh(e + self.joint.pred_ffn(pred)))
        k = z.argmax(dim=-1)
        live = ~S["done"]
        nb = (k != self.blank) & live
        pos = torch.minimum(S["count"], S["cap"])
        S["hyps"][ar, pos] = torch.where(nb, k, S["hyps"][ar, pos])
        S["count"].add_(nb.to(torch.int64))
        S["token"].copy_(torch.where(nb, k, S["token"]))
        S["h"].copy_(torch.where(nb[None, :, None], h1, S["h"]))
        S["c"].copy_(torch.where(nb[None, :, None], c1, S["c"]))
        S["frame_count"].add_(nb.to(torch.int64))
        adv = ((k == self.blank) | (S["frame_count"] >= self.n_steps)) & live
        S["t"].add_(adv.to(torch.int64))
        S["frame_count"].mul_((~adv).to(torch.int64))
        S["done"].copy_(S["t"] >= S["lens"])

    _SNAP = ("t", "count", "frame_count", "hyps", "token", "h", "c", "done")             # what a step changes (packing.capture_step)

    def _state(self, B, T, dev):
        L, H = self.predictor.num_layers, self.predictor.hidden_size
        J = self.joint.enc_ffn.out_features
        cap = T * self.n_steps                                                          # the most a stream can emit
        z64 = lambda *s: torch.zeros(s, dtype=torch.int64, device=dev)
        return dict(ar=torch.arange(B, device=dev), enc_proj=torch.zeros((B, T, J), device=dev), t=z64(B), tmax=torch.full((B,), T - 1, dtype=torch.int64, device=dev),
                    lens=z64(B), token=z64(B), h=torch.zeros((L, B, H), device=dev), c=torch.zeros((L, B, H), device=dev), count=z64(B), frame_count=z64(B),
                    hyps=z64(B, cap + 1), cap=torch.full((B,), cap, dtype=torch.int64, device=dev), done=torch.zeros((B,), dtype=torch.bool, device=dev),
                    all_done=torch.zeros((), dtype=torch.bool, device=dev))

    def _prepare(self, enc_out, enc_lens, token, state):
        """The state to start from, in buffers for (B, T) on enc_out's device; new weights or new buffers drop descriptor and graph."""
        (B, T, _), dev = enc_out.shape, enc_out.device
        self._sync_weights()
        key = (B, T, str(dev))
        if self._key != key:
            self._S, self._key = self._state(B, T, dev), key
            self._drop()
        why_not = self._head.fused_limits(B, dev)
        if self.fused and why_not:
            raise RuntimeError(why_not)
        S, fused = self._S, why_not is None if self.fused is None else bool(self.fused)
        self._fused = fused
        if fused and self._desc is None:
            self._desc = self._fused_desc(S, self._head.packs(dev), B, T)
        S["enc_proj"].copy_(self.joint.enc_ffn(enc_out.float()))
        S["lens"].copy_(torch.as_tensor(enc_lens, device=dev).to(torch.int64).clamp(0, T))
        for k in ("t", "count", "frame_count", "hyps"):
            S[k].zero_()
        S["token"].fill_(self.blank) if token is None else S["token"].copy_(token.reshape(B))
        if state is None:
            S["h"].zero_(); S["c"].zero_()
        else:
            S["h"].copy_(state[0]); S["c"].copy_(state[1])
        S["done"].copy_(S["t"] >= S["lens"])
        if fused:
            S["done8"].copy_(S["done"].to(torch.uint8))
            S["n_done"].copy_(S["done"].sum().to(torch.int32).reshape(1))

    def _run_steps(self):
        S = self._S
        if self._fused:
            lib = cfm.lib()
            for _ in range(self.steps_per_replay):
                cfm.check(lib.cfm_greedy_step(ctypes.byref(self._desc), cfm.stream()), "cfm_greedy_step")
            S["all_done"].copy_((S["n_done"] >= S["t"].shape[0]).reshape(()))
        else:
            for _ in range(self.steps_per_replay):
                self._step(S)
            S["all_done"].copy_(S["done"].all())

    @torch.no_grad()
    def search(self, enc_out, enc_lens, token=None, state=None):
        """enc_out (B, T', E) float32 encoder output, enc_lens (B,) valid frames per stream.  token (B,) / state (h, c): the predictor's input
        and LSTM state to start from (a continued stream, model.py:186-192); default: blank and zeros.  Returns (list of B token lists,
        (token, (h, c)) to continue with)."""
        self._require_eval("greedy search")
        self._prepare(enc_out, enc_lens, token, state)
        (B, T, _), S = enc_out.shape, self._S
        limit = (T * (self.n_steps + 1)) // self.steps_per_replay + 2                   # every step emits or advances: at most T (n_steps + 1) of them
        self._replay(S, self._SNAP + (("done8", "n_done") if self._fused else ()), lambda: bool(S["all_done"]), limit)
        counts = S["count"].tolist()
        hyps = S["hyps"].cpu()
        return [hyps[b, :counts[b]].tolist() for b in range(B)], (S["token"].clone(), (S["h"].clone(), S["c"].clone()))


class ChunkGreedySearch(_Search):
    """The decoder of a batched streaming recogniser: `streams` utterances decoded chunk by chunk (`chunk` encoder frames per call), all
    state -- the predictor's input token and LSTM state, the hypothesis buffer that ACCUMULATES across chunks and its counts -- resident on
    the device.  It is the reference's `greedy_search_streaming_app` (src/model.py:178-199; carry=True) / `greedy_search_streaming_eval`
    (:126-165; carry=False: that path passes cache=None, pred_input_step=None for every chunk, so the predictor restarts from blank / zeros
    each chunk -- a quirk of the reference, kept) around `basic_greedy_search`, for all streams at once.

    One decoding step is a LOOKAHEAD step: the predictor output is a pure function of (token, LSTM state), which change only when a symbol
    is emitted, so between two emissions the joint is evaluated for all remaining frames of the chunk against the one current predictor
    output and the first frame whose argmax is not blank is found on the device.  That is the reference's sequence of decisions -- the blank
    frames before the emission are the ones its loop steps over one by one with the same predictor output -- in at most
    1 + (most emissions of any stream in the chunk) steps instead of frames + emissions (`steps` holds the number the last decode needed).

    On an MI355X a step is cfm_greedy_chunk_step (csrc/greedy.hip: the skinny predictor launches, a compact row list of the frames still
    to decide, the vocabulary projection as an M-tiled f32 MFMA product, one control workgroup per stream), `steps_per_replay` of them
    captured in one HIP graph; the host reads one "streams done" counter per replay (`replays`); the steps a replay holds beyond the chunk's
    last one are empty launches (every kernel of the step returns at once when all streams are done).  Sizes outside the kernel's limits
    (64 streams, chunk 32, 4 LSTM layers, dimensions multiples of 16) raise.  On the CPU the same step runs as torch operations (`_step`)."""

    def __init__(self, predictor, joint, streams, chunk, blank=0, n_steps=64, steps_per_replay=4, use_graph=True, carry=True, fused=None, max_tokens=None):
        super().__init__(predictor, joint, blank, steps_per_replay, use_graph)
        self.B, self.chunk, self.n_steps, self.carry = int(streams), int(chunk), int(n_steps), bool(carry)
        if self.B < 1 or self.chunk < 1 or self.n_steps < 1 or self.steps_per_replay < 1:
            raise ValueError("ChunkGreedySearch: streams, chunk, n_steps and steps_per_replay are positive")
        self.dev = next(predictor.parameters()).device
        self.fused = (self.dev.type == "cuda") if fused is None else bool(fused)
        if self.fused and self._head.fused_limits(self.B, self.dev, self.chunk):
            raise RuntimeError(self._head.fused_limits(self.B, self.dev, self.chunk))
        self.S = self._state(max(1, int(max_tokens) if max_tokens is not None else 2 * self.chunk * self.n_steps))     # decode needs count + chunk * n_steps
        self._log = token_log.TokenLog(self.B)
        self.steps = self.replays = self.total_steps = self.total_replays = 0

    # -- state -----------------------------------------------------------------------------------------------------------------------------
    def _state(self, cap):
        pr, jn, B, C, dev = self.predictor, self.joint, self.B, self.chunk, self.dev
        L, H, J = pr.num_layers, pr.hidden_size, jn.enc_ffn.out_features
        z64 = lambda *s: torch.zeros(s, dtype=torch.int64, device=dev)
        z32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
        S = dict(ar=torch.arange(B, device=dev), frames=torch.arange(C, device=dev), enc_proj=torch.zeros((B, C, J), device=dev), t=z64(B), lens=z64(B),
                 token=torch.full((B,), self.blank, dtype=torch.int64, device=dev), h=torch.zeros((L, B, H), device=dev), c=torch.zeros((L, B, H), device=dev),
                 count=z64(B), frame_count=z64(B), hyps=z64(B, cap), steps=z32(1), overflow=z32(1), n_done=z32(1))
        if self.fused:
            Vp = self._head.padded_vocab()
            S.update(h_new=torch.zeros((L, B, H), device=dev), c_new=torch.zeros((L, B, H), device=dev), pred=torch.zeros((B, pr.projection.out_features), device=dev),
                     pp=torch.zeros((B, J), device=dev), act=torch.zeros((B * C, J), device=dev), pmax=torch.zeros((B * C, Vp // 16), device=dev),
                     pidx=z32(B * C, Vp // 16), rows=z32(B * C), row_off=z32(B), row_cnt=z32(B), n_rows=z32(1), done8=torch.zeros((B,), dtype=torch.uint8, device=dev))
        return S

    def _fused_desc(self, S, W):
        d = cfm.GreedyChunkDesc()
        self._head.fill_weights(d, W)
        for k in ("enc_proj", "token", "t", "count", "frame_count", "hyps", "lens", "h", "c", "h_new", "c_new", "pred", "pp", "act", "pmax", "pidx", "rows", "row_off",
                  "row_cnt", "n_rows", "steps", "overflow", "n_done"):
            setattr(d, k, S[k].data_ptr())
        d.done = S["done8"].data_ptr()
        d.hyp_cap = d.hyp_ld = S["hyps"].shape[1]
        d.B, d.chunk, d.D, d.blank, d.n_steps, d.carry = self.B, self.chunk, self.joint.enc_ffn.in_features, self.blank, self.n_steps, int(self.carry)
        return d

    def _prepare(self):
        """The descriptor for the current weights and buffers (_sync_weights; _grow drops it too)."""
        self._sync_weights()
        if self.fused and self._desc is None:
            self._desc = self._fused_desc(self.S, self._head.packs(self.dev, enc_ffn=True))

    def _grow(self, need):
        if token_log.grow(self.S, ("hyps",), need):
            self._drop()                                                                # descriptor and graph hold the old buffer's address

    # -- one lookahead step as torch operations (the CPU form; csrc/greedy.hip's cfm_greedy_chunk_step restated) ---------------------------------
    def _step(self, S):
        pr, jn, ar = self.predictor, self.joint, S["ar"]
        t, lens, fc = S["t"], S["lens"], S["frame_count"]
        live = t < lens
        S["steps"].add_(live.any().to(torch.int32))
        y, h1, c1 = self._head.lstm_step(pr.embed(S["token"]), S["h"], S["c"])
        pp = jn.pred_ffn(pr.projection(y))
        k = jn.ffn_out(torch.tanh(S["enc_proj"] + pp[:, None, :])).argmax(dim=-1)       # (B, chunk): every frame against the one predictor output
        f = S["frames"][None, :]
        nb = (k != self.blank) & (f >= t[:, None]) & (f < lens[:, None])
        emit = nb.any(dim=1)
        fstar = nb.to(torch.int64).argmax(dim=1)                                        # the first such frame
        kk = k.gather(1, fstar[:, None])[:, 0]
        cap = S["hyps"].shape[1]
        room = S["count"] < cap
        S["overflow"].add_((emit & ~room).any().to(torch.int32))
        pos = S["count"].clamp(max=cap - 1)
        S["hyps"][ar, pos] = torch.where(emit & room, kk, S["hyps"][ar, pos])
        S["count"].add_(emit.to(torch.int64))
        S["token"].copy_(torch.where(emit, kk, S["token"]))
        S["h"].copy_(torch.where(emit[None, :, None], h1, S["h"]))
        S["c"].copy_(torch.where(emit[None, :, None], c1, S["c"]))
        fc1 = torch.where(fstar == t, fc, torch.zeros_like(fc)) + 1
        capped = fc1 >= self.n_steps
        t_emit = fstar + capped.to(torch.int64)
        fc_emit = torch.where(capped, torch.zeros_like(fc1), fc1)
        S["t"].copy_(torch.where(emit, t_emit, torch.where(live, lens, t)))
        S["frame_count"].copy_(torch.where(emit, fc_emit, torch.where(live, torch.zeros_like(fc), fc)))

    def _begin_eager(self, enc):
        S = self.S
        S["enc_proj"].copy_(self.joint.enc_ffn(enc.float()))
        S["t"].zero_(); S["frame_count"].zero_(); S["steps"].zero_()
        if not self.carry:
            m = S["lens"] > 0
            S["token"].copy_(torch.where(m, torch.full_like(S["token"], self.blank), S["token"]))
            S["h"].mul_((~m)[None, :, None].to(S["h"].dtype)); S["c"].mul_((~m)[None, :, None].to(S["c"].dtype))

    def _run_steps(self):
        if self.fused:
            lib = cfm.lib()
            for _ in range(self.steps_per_replay):
                cfm.check(lib.cfm_greedy_chunk_step(ctypes.byref(self._desc), cfm.stream()), "cfm_greedy_chunk_step")
        else:
            for _ in range(self.steps_per_replay):
                self._step(self.S)

    _SNAP = ("t", "count", "frame_count", "hyps", "token", "h", "c", "steps", "overflow", "n_done")             # what a step changes (packing.capture_step)

    # -- public ---------------------------------------------------------------------------------------------------------------------------
    def reset(self, streams=None):
        """New utterances on the given streams (all by default): token <- blank, LSTM state and hypotheses emptied (Transducer.init_state)."""
        S = self.S
        streams = None if streams is None else list(streams)
        idx = packing.stream_index(streams, self.dev)
        S["token"][idx] = self.blank
        for k in ("count", "t", "frame_count", "hyps"):
            S[k][idx] = 0
        S["h"][:, idx] = 0
        S["c"][:, idx] = 0
        self._log.reset(streams)

    def hyps(self):
        """Everything emitted per stream since its last reset."""
        return self._log.hyps()

    def state(self):
        """(token (B,), (h, c) (L, B, H)): the predictor input and LSTM state the next chunk starts from (copies)."""
        return self.S["token"].clone(), (self.S["h"].clone(), self.S["c"].clone())

    def set_state(self, token, state):
        """Continue from a carried (token (B,), (h, c) (L, B, H)), as `BatchedGreedySearch.search(..., token, state)` does."""
        self.S["token"].copy_(token.reshape(self.B))
        self.S["h"].copy_(state[0])
        self.S["c"].copy_(state[1])

    @torch.no_grad()
    def decode(self, enc_chunk, lens=None):
        """enc_chunk (B, chunk, E) float32 encoder output of one chunk; lens (B,): how many of its frames belong to each stream (default: all;
        0: the stream is idle and nothing about it changes).  Returns a list of B lists: the tokens this chunk added."""
        self._require_eval("greedy search")
        B, C, S, dev = self.B, self.chunk, self.S, self.dev
        if tuple(enc_chunk.shape[:2]) != (B, C) or enc_chunk.device != dev:
            raise ValueError("ChunkGreedySearch.decode wants (%d, %d, E) on %s, got %s on %s" % (B, C, dev, tuple(enc_chunk.shape), enc_chunk.device))
        self._grow(self._log.most() + C * self.n_steps)                                 # the most any stream can hold after this chunk
        self._prepare()
        host = packing.stream_lens("ChunkGreedySearch.decode", "lens", B, lens, C, S["lens"])
        maybe_live = host is None or any(host)                                          # lens on the device: the host does not know who is idle
        if self.fused:
            self._desc.enc = self._f32_chunk(enc_chunk).data_ptr()
            cfm.check(cfm.lib().cfm_greedy_chunk_begin(ctypes.byref(self._desc), cfm.stream()), "cfm_greedy_chunk_begin")
        else:
            self._begin_eager(enc_chunk)
        limit = (C * (self.n_steps + 1)) // self.steps_per_replay + 2                   # a lookahead step emits or finishes a stream: fewer than the single-frame bound
        done = (lambda: int(S["n_done"]) >= B) if self.fused else (lambda: bool((S["t"] >= S["lens"]).all()))
        self.replays = self._replay(S, self._SNAP + (("done8",) if self.fused else ()), done, limit) if maybe_live else 0
        rep = torch.cat([S["count"], S["overflow"].to(torch.int64), S["steps"].to(torch.int64)]).tolist()
        counts, overflow, self.steps = rep[:B], rep[B], rep[B + 1]
        if overflow:
            raise RuntimeError("ChunkGreedySearch: a stream emitted more symbols than the hypothesis buffer holds")
        self.total_steps += self.steps
        self.total_replays += self.replays
        return self._log.take(S["hyps"], counts)


def _beam_state(head, K, B, T, max_len, dev):
    """The device buffers of cfm.RnntBeamDesc for B utterances of at most T frames, K hypotheses each (both beam searches)."""
    pr, jn = head.predictor, head.joint
    L, H, R, Vp = pr.num_layers, pr.hidden_size, B * K, head.padded_vocab()
    n_nodes = int(cfm.lib().cfm_rnnt_beam_nodes(B, T, max_len, K))
    z = lambda dt, *s: torch.zeros(s, dtype=dt, device=dev)
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    return dict(enc_proj=z(f32, B, T, jn.enc_ffn.out_features), lens=z(i64, B), token=z(i64, R), t=z(i64, R), hash=z(i64, R), fc=z(i32, R), len=z(i32, R),
                node=z(i32, R), parent=z(i32, R), ext=z(i32, R), live=z(i32, R), score=z(f32, R), h=z(f32, 2, L, R, H), c=z(f32, 2, L, R, H),
                h_new=z(f32, L, R, H), c_new=z(f32, L, R, H), pred=z(f32, R, pr.projection.out_features), act=z(f32, R, jn.pred_ffn.out_features),
                logits=z(f32, R, Vp), topk_idx=z(i32, R, K + 1), topk_logp=z(f32, R, K + 1), lse=z(f32, R), nodes=z(i32, n_nodes, 2), fin_score=z(f32, B, K),
                fin_node=z(i32, B, K), fin_len=z(i32, B, K), n_fin=z(i32, B), step=z(i32, B), done=z(torch.uint8, B), n_done=z(i32, 1),
                nbest_tokens=z(i64, B, K, max_len), nbest_len=z(i32, B, K), nbest_score=z(f32, B, K), all_done=z(torch.bool))


# what a beam step changes (packing.capture_step); the scratch a step writes before it reads it is not among them
_BEAM_SNAP = ("token", "t", "hash", "fc", "len", "node", "parent", "ext", "live", "score", "h", "c", "nodes", "fin_score", "fin_node", "fin_len", "n_fin", "step", "done",
              "n_done", "nbest_tokens", "nbest_len", "nbest_score")


def _fill_beam_desc(d, search, S, W, B, T, len_by_frames, parity):
    """The cfm.RnntBeamDesc d filled for the steps of one parity (the h / c buffer a step reads alternates); S's tensors go by field name."""
    search._head.fill_weights(d, W)
    for k, _ in cfm.RnntBeamDesc._fields_:
        if k in S:
            setattr(d, k, S[k].data_ptr())
    d.B, d.T, d.V, d.beam, d.blank, d.max_symbols = B, T, search.joint.ffn_out.out_features, search.beam, search.blank, search.max_symbols
    d.n_nodes, d.max_len, d.len_by_frames, d.parity = S["nodes"].shape[0], S["nbest_tokens"].shape[2], len_by_frames, parity
    return d


def _nbest_lists(nbest_tokens, nbest_len, nbest_score, rows):
    """The device's n-best buffers read back: per utterance in rows its [(tokens, score)], best first, the unused (-inf) entries left out."""
    lens, scores, toks = nbest_len.tolist(), nbest_score.tolist(), nbest_tokens.cpu()
    return [[(toks[b, j, :lens[b][j]].tolist(), scores[b][j]) for j in range(len(scores[b])) if scores[b][j] != float("-inf")] for b in rows]


class BeamSearch(_Search):
    """RNN-T beam search on the device: per utterance the `beam` best finished hypotheses with their scores (log of the summed probability
    of the alignments found, no length normalisation).  The search is alignment-length synchronous and is specified in float64 in
    tests/rnnt_beam_ref.py; include/cfm.h (cfm_rnnt_beam_step) restates it.  max_symbols: the most symbols emitted on one frame (the role
    n_steps plays in the greedy searches); max_len: the most tokens of a hypothesis (default: the utterance's frames).

    The B * beam <= 64 hypotheses are the rows of the fused step (csrc/greedy.hip: the greedy step's predictor and joint launches, the
    log-softmax top-k of the CTC decoder, one ranking / merging workgroup per utterance); `steps_per_replay` steps (made even: the LSTM state
    alternates between two buffers by step parity) are captured in one HIP graph and the host reads one "utterances done" counter per replay.
    Device only: there is no torch-operation form; CPU tensors and sizes outside the kernels' limits raise."""

    def __init__(self, predictor, joint, beam, blank=0, max_symbols=64, max_len=None, steps_per_replay=16, use_graph=True):
        super().__init__(predictor, joint, blank, steps_per_replay, use_graph, even_steps=True)
        self.beam, self.max_symbols, self.max_len = int(beam), int(max_symbols), None if max_len is None else int(max_len)
        if not 1 <= self.beam <= 15:
            raise ValueError("BeamSearch: beam = %d outside 1..15 (the top-k launch returns 16 classes, one of which may be the blank)" % self.beam)
        if self.max_symbols < 1 or self.steps_per_replay < 1 or (self.max_len is not None and self.max_len < 0):
            raise ValueError("BeamSearch: max_symbols and steps_per_replay are positive, max_len is not negative")
        if not 0 <= self.blank < joint.ffn_out.out_features or self.beam + 1 > joint.ffn_out.out_features:
            raise ValueError("BeamSearch: blank inside the vocabulary, beam + 1 <= its size")
        self._S = self._key = None
        self.steps = self.replays = 0

    def _state(self, B, T, dev):
        return _beam_state(self._head, self.beam, B, T, T if self.max_len is None else self.max_len, dev)

    def _make_descs(self, S, W, B, T):
        """The descriptor of the steps of either parity."""
        return [_fill_beam_desc(cfm.RnntBeamDesc(), self, S, W, B, T, int(self.max_len is None), parity) for parity in (0, 1)]

    def _run_steps(self):
        lib, S = cfm.lib(), self._S
        for i in range(self.steps_per_replay):
            cfm.check(lib.cfm_rnnt_beam_step(ctypes.byref(self._descs[i & 1]), cfm.stream()), "cfm_rnnt_beam_step")
        S["all_done"].copy_((S["n_done"] >= S["lens"].shape[0]).reshape(()))

    @torch.no_grad()
    def search(self, enc_out, enc_lens):
        """enc_out (B, T', E) float32 encoder output on the device, enc_lens (B,) valid frames per utterance.  Returns per utterance a list
        of (tokens, score), best first, at most `beam`; an utterance without frames gives [([], 0.0)]."""
        self._require_eval("beam search")
        (B, T, _), dev, K = enc_out.shape, enc_out.device, self.beam
        if dev.type != "cuda":
            raise RuntimeError("BeamSearch runs on the device only: enc_out is on %s (there is no fallback)" % dev)
        if B * K > 64 or B < 1 or T < 1:
            raise RuntimeError("BeamSearch: B * beam = %d * %d rows, the fused step takes 1..64 (and T' >= 1)" % (B, K))
        why_not = self._head.fused_limits(B * K, dev)
        if why_not:
            raise RuntimeError(why_not)
        self._sync_weights()
        key = (B, T, K, str(dev))
        if self._key != key:                                                            # new buffers: descriptors and graph hold their addresses
            self._S, self._key = self._state(B, T, dev), key
            self._drop()
        S = self._S
        if self._descs is None:
            self._descs = self._make_descs(S, self._head.packs(dev), B, T)
        S["enc_proj"].copy_(self.joint.enc_ffn(enc_out.float()))
        S["lens"].copy_(torch.as_tensor(enc_lens, device=dev).to(torch.int64).clamp(0, T))
        cfm.check(cfm.lib().cfm_rnnt_beam_begin(ctypes.byref(self._descs[0]), cfm.stream()), "cfm_rnnt_beam_begin")
        limit = (T + S["nbest_tokens"].shape[2] + 1) // self.steps_per_replay + 2         # a step adds one to every live t + len: at most T + max_len + 1 of them
        self.replays = self._replay(S, _BEAM_SNAP, lambda: bool(S["all_done"]), limit)
        out = _nbest_lists(S["nbest_tokens"], S["nbest_len"], S["nbest_score"], range(B))
        self.steps = int(S["step"].max())
        return out


class StreamingBeamSearch(_Search):
    """The RNN-T beam search of `BeamSearch` with the beam carried across encoder chunks: `streams` utterances decoded chunk by chunk, every
    hypothesis, the trie and the projected frames fed so far ((streams, max_frames, J): no ring, a live hypothesis may sit many frames behind
    the newest) resident on the device.  Specified in float64 in tests/rnnt_beam_ref_stream.py; include/cfm.h (cfm_rnnt_beam_stream_*)
    restates it.

    A stream whose utterance has not ended steps only while every live hypothesis is at least two frames behind the frames it holds, and
    PAUSES otherwise; `final` lifts the rule and the stream runs to its n-best list.  Holding one frame back makes the decisions those of the
    offline search on the whole utterance however the frames were cut: tokens and order are BeamSearch's (max_len given explicitly there too)
    wherever float32 tells the candidates apart.  The beam trails the encoder by one frame.

    decode(enc_chunk, lens, final) returns per stream dict(stable=tokens, best=(tokens, score), nbest=None | [(tokens, score)] best first):
    `best` is the top-ranked live hypothesis, `stable` the longest common prefix of all live hypotheses -- it only grows and is a prefix of
    every entry of the final n-best list: what a UI may print without retracting it --, `nbest` the result once the stream is final and done
    (`best` is then its first entry).  A done stream ignores feeds until `reset`.

    Limits: streams * beam <= 64, 1 <= beam <= 15, max_frames encoder frames per utterance (more raises), max_len tokens per hypothesis
    (default: max_frames).  `steps_per_replay` is made even (the LSTM state alternates between two buffers by step parity, and a paused
    stream must find its state at parity 0 of the next decode).  Device only: there is no torch-operation form."""

    def __init__(self, predictor, joint, streams, beam, chunk, max_frames, max_len=None, blank=0, max_symbols=64, steps_per_replay=8, use_graph=True):
        super().__init__(predictor, joint, blank, steps_per_replay, use_graph, even_steps=True)
        self.B, self.beam, self.chunk, self.max_frames, self.max_symbols = int(streams), int(beam), int(chunk), int(max_frames), int(max_symbols)
        self.max_len = self.max_frames if max_len is None else int(max_len)
        if not 1 <= self.beam <= 15 or self.B < 1 or self.B * self.beam > 64:
            raise ValueError("StreamingBeamSearch: 1 <= beam <= 15 and streams * beam <= 64 rows (streams=%d beam=%d)" % (self.B, self.beam))
        if self.chunk < 1 or self.max_frames < 1 or self.max_len < 0 or self.max_symbols < 1 or self.steps_per_replay < 1:
            raise ValueError("StreamingBeamSearch: chunk, max_frames, max_symbols and steps_per_replay are positive, max_len is not negative")
        if not 0 <= self.blank < joint.ffn_out.out_features or self.beam + 1 > joint.ffn_out.out_features:
            raise ValueError("StreamingBeamSearch: blank inside the vocabulary, beam + 1 <= its size")
        self.dev = next(predictor.parameters()).device
        if self.dev.type != "cuda":
            raise RuntimeError("StreamingBeamSearch runs on the device only: the predictor is on %s (there is no fallback)" % self.dev)
        why_not = self._head.fused_limits(self.B * self.beam, self.dev)
        if why_not is None and joint.enc_ffn.in_features % 16:
            why_not = "the streaming beam search needs an encoder dimension that is a multiple of 16 (there is no fallback)"
        if why_not:
            raise RuntimeError(why_not)
        self.S = self._state()
        self.steps = self.replays = self.total_steps = self.total_replays = 0
        self._stable = [[] for _ in range(self.B)]
        self._nbest = [None] * self.B
        self._step_host, self._avail_host = [0] * self.B, [0] * self.B
        self.reset()

    def _state(self):
        B, K, C, dev = self.B, self.beam, self.chunk, self.dev
        S = _beam_state(self._head, K, B, self.max_frames, self.max_len, dev)
        z = lambda dt, *s: torch.zeros(s, dtype=dt, device=dev)
        S.update(chunk_proj=z(torch.float32, B * C, self.joint.enc_ffn.out_features), avail=z(torch.int32, B), final=z(torch.uint8, B), paused=z(torch.uint8, B),
                 feed_final=z(torch.uint8, B), overflow=z(torch.int32, 1), best_tokens=z(torch.int64, B, max(self.max_len, 1)), best_len=z(torch.int32, B),
                 stable_len=z(torch.int32, B), best_score=z(torch.float32, B), mask=z(torch.uint8, B))
        return S

    def _make_descs(self, W):
        out, S = [cfm.RnntBeamStreamDesc(), cfm.RnntBeamStreamDesc()], self.S
        for parity, d in enumerate(out):
            _fill_beam_desc(d.beam, self, S, W, self.B, self.max_frames, 0, parity)
            for k in ("chunk_proj", "avail", "final", "paused", "feed_final", "overflow", "best_tokens", "best_len", "stable_len", "best_score"):
                setattr(d, k, S[k].data_ptr())
            d.ef_w, d.ef_b = W["ef_w"].data_ptr(), W["ef_b"].data_ptr()
            d.chunk, d.D = self.chunk, self.joint.enc_ffn.in_features
        return out

    def _prepare(self):
        """The descriptors for the current weights (_sync_weights); the state buffers stay."""
        self._sync_weights()
        if self._descs is None:
            self._descs = self._make_descs(self._head.packs(self.dev, enc_ffn=True))

    def _run_steps(self):
        lib, S = cfm.lib(), self.S
        for i in range(self.steps_per_replay):
            cfm.check(lib.cfm_rnnt_beam_stream_step(ctypes.byref(self._descs[i & 1]), cfm.stream()), "cfm_rnnt_beam_stream_step")
        S["all_done"].copy_((S["n_done"] >= self.B).reshape(()))

    def reset(self, streams=None):
        """New utterances on the given streams (all by default): the empty hypothesis, no frames, not final."""
        self._prepare()
        idx = list(range(self.B)) if streams is None else [int(b) for b in streams]
        mask = [0] * self.B
        for b in idx:
            mask[b] = 1
            self._stable[b], self._nbest[b], self._step_host[b], self._avail_host[b] = [], None, 0, 0
        self.S["mask"].copy_(torch.tensor(mask, dtype=torch.uint8))
        cfm.check(cfm.lib().cfm_rnnt_beam_stream_reset(ctypes.byref(self._descs[0]), self.S["mask"].data_ptr(), cfm.stream()), "cfm_rnnt_beam_stream_reset")

    @torch.no_grad()
    def decode(self, enc_chunk, lens=None, final=None):
        """enc_chunk (B, chunk, E) float32 encoder output of one chunk on the device; lens (B,): how many of its frames belong to each stream
        (default: all; 0: nothing arrives); final (B,) truthy where the utterance ends with this feed (it may come with 0 frames)."""
        self._require_eval("beam search")
        B, C, S, dev = self.B, self.chunk, self.S, self.dev
        if tuple(enc_chunk.shape[:2]) != (B, C) or enc_chunk.device != dev:
            raise ValueError("StreamingBeamSearch.decode wants (%d, %d, E) on %s, got %s on %s" % (B, C, dev, tuple(enc_chunk.shape), enc_chunk.device))
        self._prepare()
        packing.stream_lens("StreamingBeamSearch.decode", "lens", B, lens, C, S["lens"])
        packing.stream_lens("StreamingBeamSearch.decode", "final flags", B, final, 1, S["feed_final"], default=0)
        self._descs[0].enc = self._descs[1].enc = self._f32_chunk(enc_chunk).data_ptr()
        lib = cfm.lib()
        cfm.check(lib.cfm_rnnt_beam_stream_feed(ctypes.byref(self._descs[0]), cfm.stream()), "cfm_rnnt_beam_stream_feed")
        # a step adds one to every live t + len, which is the steps the stream has taken: at most avail + max_len + 1 of them in all
        most = max(min(a + C, self.max_frames) + self.max_len + 1 - s for a, s in zip(self._avail_host, self._step_host))
        S["all_done"].copy_((S["n_done"] >= B).reshape(()))
        self.replays = 0 if bool(S["all_done"]) else self._replay(S, _BEAM_SNAP + ("paused",), lambda: bool(S["all_done"]), most // self.steps_per_replay + 2)
        cfm.check(lib.cfm_rnnt_beam_stream_report(ctypes.byref(self._descs[0]), cfm.stream()), "cfm_rnnt_beam_stream_report")
        ints = torch.cat([S["avail"], S["step"], S["best_len"], S["stable_len"], S["done"].to(torch.int32), S["overflow"]]).tolist()
        avail, step, best_len, stable_len, done = (ints[i * B:(i + 1) * B] for i in range(5))
        overflow = ints[5 * B]
        if overflow:
            S["overflow"].zero_()
            raise RuntimeError("StreamingBeamSearch: a stream was fed more than max_frames = %d encoder frames (nothing of it changed)" % self.max_frames)
        self.steps = max(s - s0 for s, s0 in zip(step, self._step_host))
        self.total_steps += self.steps
        self.total_replays += self.replays
        self._step_host, self._avail_host = step, avail
        top = max([n for n, dn in zip(best_len, done) if not dn] + [0])
        best_tokens = S["best_tokens"][:, :top].cpu() if top else None
        best_score = S["best_score"].tolist()
        fresh = [b for b in range(B) if done[b] and self._nbest[b] is None]
        if fresh:
            for b, nbest in zip(fresh, _nbest_lists(S["nbest_tokens"], S["nbest_len"], S["nbest_score"], fresh)):
                self._nbest[b] = nbest
        out = []
        for b in range(B):
            if done[b]:
                out.append(dict(stable=list(self._stable[b]), best=(list(self._nbest[b][0][0]), self._nbest[b][0][1]), nbest=[(list(t), s) for t, s in self._nbest[b]]))
                continue
            row = best_tokens[b, :best_len[b]].tolist() if best_len[b] else []
            self._stable[b].extend(row[len(self._stable[b]):stable_len[b]])
            out.append(dict(stable=list(self._stable[b]), best=(row, best_score[b]), nbest=None))
        return out
