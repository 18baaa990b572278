"""Float64 restatement of one step of the batched RNN-T greedy search (greedy.py, csrc/greedy.hip) for the tests: the predictor's LSTM cell per
layer, the projection, the joint's input and vocabulary projection over all B streams at once, and the loop's bookkeeping (model.py:255-267)
as a host loop over the streams; plus a margin-aware float64 search for one utterance (the oracle's loop, oracle.rnnt_greedy_search, that also
records how far apart the two best logits were at every decision).

The margin rule: an f32 evaluation of the joint picks the float64 argmax whenever the two best logits are further apart than the f32 error of
a logit; where they are closer, either of them is a correct result, and a search may go a different way from that decision on."""
import numpy as np
import torch

import synth


def modules(V, E, H, P, J, L, seed, enc_dim=None, shaped=False):
    """RNNPredictor(V, embed E, output P, hidden H, L layers) and TransducerJoint(V, enc_dim, P, J) on synthetic weights, eval mode.
    shaped: synth.greedy_joint_ (a search over the head is not degenerate); otherwise the plain synthetic values."""
    import joint
    import predictor
    pr = predictor.RNNPredictor(V, E, P, H, 0.1, L).eval()
    jn = joint.TransducerJoint(V, enc_dim or J, P, J).eval()
    synth.load_synth_(pr, seed)
    synth.load_synth_(jn, seed + 1)
    if shaped:
        synth.greedy_joint_(jn, V)
    return pr, jn


def params64(pr, jn):
    """float64 CPU copies under the oracle's prefixes: "p." predictor, "j." joint."""
    P = {"p." + k: v.detach().double().cpu() for k, v in pr.state_dict().items()}
    P.update({"j." + k: v.detach().double().cpu() for k, v in jn.state_dict().items()})
    return P


def num_layers(P):
    n = 0
    while ("p.rnn.weight_ih_l%d" % n) in P:
        n += 1
    return n


def step64(P, token, h, c, e):
    """token (B,) int, h / c (L, B, H), e (B, J) the enc_ffn row each stream is on.  Returns float64 CPU tensors: h_new / c_new (L, B, H),
    pred (B, P), act (B, J), logits (B, V), and gate_max = max |gate pre-activation| over all layers."""
    token = torch.as_tensor(token).long().cpu()
    h, c, e = (torch.as_tensor(v).double().cpu() for v in (h, c, e))
    x = P["p.embed.weight"][token]
    hs, cs, gate_max = [], [], 0.0
    for l in range(num_layers(P)):
        gates = (x @ P["p.rnn.weight_ih_l%d" % l].t() + P["p.rnn.bias_ih_l%d" % l] +
                 h[l] @ P["p.rnn.weight_hh_l%d" % l].t() + P["p.rnn.bias_hh_l%d" % l])
        gate_max = max(gate_max, float(gates.abs().max()))
        i, f, g, o = gates.chunk(4, dim=-1)
        c1 = torch.sigmoid(f) * c[l] + torch.sigmoid(i) * torch.tanh(g)
        x = torch.sigmoid(o) * torch.tanh(c1)
        hs.append(x)
        cs.append(c1)
    pred = x @ P["p.projection.weight"].t() + P["p.projection.bias"]
    act = torch.tanh(e + pred @ P["j.pred_ffn.weight"].t() + P["j.pred_ffn.bias"])
    logits = act @ P["j.ffn_out.weight"].t() + P["j.ffn_out.bias"]
    return dict(h_new=torch.stack(hs), c_new=torch.stack(cs), pred=pred, act=act, logits=logits, gate_max=gate_max)


def argmax_within(z, delta):
    """z (..., N) float64.  Returns (argmax with the lowest index on ties, as torch.argmax; top-2 gap; boolean mask of the entries within
    delta of the maximum)."""
    top = z.max(-1, keepdim=True).values
    k = z.argmax(-1)
    gap = top[..., 0] - z.scatter(-1, k[..., None], float("-inf")).max(-1).values if z.shape[-1] > 1 else torch.full_like(top[..., 0], float("inf"))
    return k, gap, z >= top - delta


def control(st, k, h_new, c_new, blank, n_steps):
    """model.py:255-267 on a host copy of the search state (numpy arrays: token, t, count, frame_count, lens int64 [B], hyps int64 [B, ld],
    done bool [B], h / c [L, B, H], n_done int, cap int) driven by the step's class k [B]; h_new / c_new are the step's LSTM candidates.
    Returns the state after the step (new arrays)."""
    s = {n: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for n, v in st.items()}
    for b in range(len(k)):
        was_done, kb = bool(s["done"][b]), int(k[b])
        nb = kb != blank and not was_done
        if nb:
            s["hyps"][b, min(int(s["count"][b]), s["cap"])] = kb
            s["count"][b] += 1
            s["token"][b] = kb
            s["frame_count"][b] += 1
            s["h"][:, b] = h_new[:, b]
            s["c"][:, b] = c_new[:, b]
        if (kb == blank or s["frame_count"][b] >= n_steps) and not was_done:
            s["t"][b] += 1
            s["frame_count"][b] = 0
        s["done"][b] = s["t"][b] >= s["lens"][b]
        if s["done"][b] and not was_done:
            s["n_done"] += 1
    return s


def search64(P, enc_proj, n, blank, n_steps, delta, token=None, state=None):
    """oracle.rnnt_greedy_search (model.py:215-269) for one utterance on float64 parameters, enc_proj (T', J) = enc_ffn(encoder output)
    already applied, n valid frames.  Returns (tokens, (token, (h, c)), first): first is the number of tokens emitted before the first
    decision whose two best logits are within delta of each other, None when there is no such decision."""
    from oracle import conformer_oracle as O
    L, H = num_layers(P), P["p.rnn.weight_hh_l0"].shape[1]
    enc_proj = torch.as_tensor(enc_proj).double().cpu()
    h, c = (torch.zeros((L, H), dtype=torch.float64),) * 2 if state is None else (state[0].double().cpu(), state[1].double().cpu())
    token = blank if token is None else int(token)
    t, hyps, per_frame, first = 0, [], 0, None
    while t < int(n):
        pred, new_h, new_c = O.predictor_step(P, "p.", token, h, c)
        pf = pred @ P["j.pred_ffn.weight"].t() + P["j.pred_ffn.bias"]            # pre_project=False skips both input projections
        logits = O.joint_forward(P, "j.", enc_proj[t][None, None, :], pf[None, None, :], pre_project=False).reshape(-1)
        k, gap, _ = argmax_within(logits, 0.0)
        k = int(k)
        if first is None and float(gap) <= delta:
            first = len(hyps)
        if k != blank:
            hyps.append(k)
            per_frame += 1
            token, h, c = k, new_h, new_c
        if k == blank or per_frame >= n_steps:
            t += 1
            per_frame = 0
    return hyps, (token, (h, c)), first


def random_state(S, rs, V, n_steps):
    """Undoctored values in every state tensor of a BatchedGreedySearch._state dict S that one step reads: tokens, LSTM state, frame index
    (T' and beyond too), per-frame and total counts, lengths (0 and beyond T'), finished streams that still have frames and carry a state;
    the fused step's done8 / n_done and scratch (NaN / -1: every entry the step owns must be written) when present.  Returns the host copy
    control() starts from."""
    L, B, H = S["h"].shape
    T, J = S["enc_proj"].shape[1:]
    cap = int(S["cap"][0])
    t = rs.randint(0, T + 2, B)                          # t == T' and T' + 1: the frame clamp of the joint's input
    lens = rs.randint(0, T + 3, B)                       # 0 and beyond T'
    lens[::5] = 0
    done = (t >= lens) | (rs.rand(B) < 0.2)              # some finished streams with frames left: `done` alone decides
    vals = dict(token=rs.randint(0, V, B), t=t, lens=lens, frame_count=rs.randint(0, n_steps, B), count=rs.randint(0, cap + 1, B),
                hyps=rs.randint(-5, V, (B, S["hyps"].shape[1])))
    for k, v in vals.items():
        S[k].copy_(torch.from_numpy(v.astype(np.int64)))
    S["h"].copy_(torch.from_numpy(rs.uniform(-1, 1, (L, B, H)).astype(np.float32)))
    S["c"].copy_(torch.from_numpy((2.0 * rs.standard_normal((L, B, H))).astype(np.float32)))
    S["enc_proj"].copy_(torch.from_numpy(rs.standard_normal((B, T, J)).astype(np.float32)))
    S["done"].copy_(torch.from_numpy(done))
    if "done8" in S:
        S["done8"].copy_(torch.from_numpy(done.astype(np.uint8)))
        S["n_done"].fill_(int(done.sum()))
        for k in ("h_new", "c_new", "pred", "act", "pmax"):
            S[k].fill_(float("nan"))
        S["pidx"].fill_(-1)
    host = {k: S[k].cpu().numpy().copy() for k in ("token", "t", "lens", "frame_count", "count", "hyps", "h", "c")}
    host.update(done=done.copy(), n_done=int(done.sum()), cap=cap)
    return host


def enc_rows(S, host):
    """(B, J) the enc_ffn row each stream's step reads: frame min(t, T' - 1)."""
    B, T = S["enc_proj"].shape[:2]
    return S["enc_proj"].cpu()[torch.arange(B), torch.from_numpy(np.minimum(host["t"], T - 1))]


def check_search(pr, jn, enc, lens, blank, n_steps, res, delta, token0=None, state0=None):
    """A BatchedGreedySearch.search result `res` stream by stream against search64 (margin rule): tokens equal up to the first decision
    whose two best float64 logits are within delta; where there is none, all tokens and the final token equal and the final h / c close.
    Returns (streams with no close decision, their tokens, max|d| / max|ref| of their final h and c)."""
    P64 = params64(pr, jn)
    enc_proj = enc.double().cpu() @ P64["j.enc_ffn.weight"].t() + P64["j.enc_ffn.bias"]
    hyps, (tok, (hh, cc)) = res
    hh, cc = hh.double().cpu(), cc.double().cpu()
    clean, ntok, dh, dc, mh, mc = 0, 0, 0.0, 0.0, 1e-30, 1e-30
    for b in range(enc.shape[0]):
        st = None if state0 is None else (state0[0][:, b], state0[1][:, b])
        ref, (rt, (rh, rc)), first = search64(P64, enc_proj[b], int(lens[b]), blank, n_steps, delta, None if token0 is None else int(token0[b]), st)
        if first is not None:
            assert hyps[b][:first] == ref[:first], (b, first, hyps[b][:first + 1], ref[:first + 1])
            continue
        assert hyps[b] == ref, (b, hyps[b], ref)
        assert int(tok[b]) == rt, (b, int(tok[b]), rt)
        dh, dc = max(dh, float((hh[:, b] - rh).abs().max())), max(dc, float((cc[:, b] - rc).abs().max()))
        mh, mc = max(mh, float(rh.abs().max())), max(mc, float(rc.abs().max()))
        clean += 1
        ntok += len(ref)
    return clean, ntok, max(dh / mh, dc / mc)
