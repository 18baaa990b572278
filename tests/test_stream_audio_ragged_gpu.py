"""GPU: audio packets of any size -- fbank.StreamingFbank.step(samples, out, sample_lens, final) (csrc/fbank.hip, the mode with n_new set) and
transducer.StreamingRecognizer.step_audio(samples, sample_lens=..., final=...).

  1. features: every window a stream runs equals the offline KaldiFbank rows [pos, pos + m) of its utterance BIT FOR BIT (same kernel arithmetic,
     same absolute-frame dither), rows >= m are exactly zero in a buffer pre-filled with NaN, and the device's carry length, position and window
     lengths equal the host mirror after every call -- for a random packetisation, dither 0 and 0.1, int16 and f32 input;
  2. whole blocks: without sample_lens the step is what it was, and after the switch sample_lens = [n_next] * B gives the same windows.  The offline
     KaldiFbank rows stand in for the parent commit's bits here: the existing streaming test holds the whole-block path to exactly them, and the
     digest comparison against the parent's build is the cost run's (profiles/r12_stream_audio_ragged.txt);
  3. what lies behind a stream's own samples in its row is never read: 50 N(0,1) or NaN there moves no bit;
  4. end to end (config-1 encoder, the shaped head with the recorded blank bias, fp32): tokens per stream equal those of a driver that cuts the
     offline features by the reference's schedule (tests/test_stream_audio_ragged_cpu.py ref_windows) and calls step(frames, frame_lens=...), for an
     aligned and two random packetisations; encoder rows [0, c_b) bit-identical where the two schedules coincide (the aligned one) -- and, as measured,
     for the random ones too, so all are held to equality (the figure is printed);
  5. one captured graph serves every packetisation;  6. a stream reset mid-utterance and reused gives a fresh recogniser's tokens;
  7. chunk 16, 64 streams, a quarter of them ending on short windows, against the same driver."""
import random

import numpy as np
import pytest
import torch

import greedy_ref
import synth
from conftest import load_golden
from test_fbank_gpu import clip, clip_cmvn, long_signal
from test_stream_audio_ragged_cpu import num_frames, ref_windows, samples_for

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TOL_FP32 = 5e-5 * 2.0                                    # tests/test_stream_ragged_gpu.py: TOL["fp32"] * 2


def c_of(n):
    return 0 if n < 7 else ((n - 1) // 2 - 1) // 2


def utterances(lengths, spacing):
    sig = long_signal()
    return [sig[b * spacing: b * spacing + n].copy() for b, n in enumerate(lengths)]


def offline(utts, dither=0.0, seed=5, dtype=torch.int16):
    import fbank
    batch = np.zeros((len(utts), max(max(len(u) for u in utts), 400)), np.int16)
    for b, u in enumerate(utts):
        batch[b, :len(u)] = u
    feats, n = fbank.KaldiFbank(dither=dither, seed=seed)(torch.from_numpy(batch).to(DEV).to(dtype), torch.tensor([len(u) for u in utts], dtype=torch.int32, device=DEV))
    assert n.tolist() == [num_frames(len(u)) for u in utts]
    return feats


def packets(utts, accepts, pending, n_first, n_next, rng=None, cap=None):
    """Generator of (takes, final, cursor before) per call until every stream is final and none is pending.  rng None: the aligned packetisation
    (n_first, then n_next per call, the rest with `final`); else random sizes 0 .. min(accepts, cap).  send() nothing; reads accepts() / pending()."""
    B = len(utts)
    cur, final = [0] * B, [False] * B
    calls = 0
    while not all(final) or pending():
        calls += 1
        assert calls < 2000
        acc = accepts()
        takes = []
        for b in range(B):
            left = len(utts[b]) - cur[b]
            if final[b]:
                n = 0
            elif rng is None:
                n = min(left, n_first if cur[b] == 0 else n_next)
            else:
                n = min(rng.randint(0, min(acc[b], cap)), left)
            takes.append(n)
            final[b] = final[b] or left == n
        yield takes, list(final), list(cur)
        cur = [c + n for c, n in zip(cur, takes)]


def block_of(utts, takes, cur, dtype, garbage="pattern", seed=0):
    """(B, max takes + 5) left-aligned packets, (B, 0) when no stream brings a sample; behind a stream's own samples: -77, 50 N(0,1) or NaN (f32 only)."""
    B, width = len(utts), max(takes) + (5 if max(takes) else 0)              # a call that only drains brings a (B, 0) block
    blk = np.zeros((B, width), np.float32)
    if garbage == "pattern":
        blk[:] = -77.0
    elif garbage == "noise":
        blk[:] = np.round(50.0 * synth.normal(seed, (B, width)))
    elif garbage == "nan":
        blk[:] = np.nan
    for b, n in enumerate(takes):
        blk[b, :n] = utts[b][cur[b]:cur[b] + n]
    t = torch.from_numpy(blk)
    return (t.to(torch.int16) if dtype == torch.int16 else t).to(DEV)


def run_fbank(utts, ref, dither, dtype, seed, cap, garbage="pattern", check=True):
    """Drive a StreamingFbank (chunk 2) over the utterances; returns the list of output buffers (clones) and the final valid carries."""
    import fbank
    B = len(utts)
    sf = fbank.StreamingFbank(B, 2, DEV, dither=dither, seed=5)
    assert sf.accepts() == [sf.n_first + sf.n_next - 1] * B and sf.pending() == [] and sf.frame_lens is None
    out = torch.empty((B, sf.window, 80), dtype=torch.float32, device=DEV)
    outs, ran = [], [[] for _ in range(B)]
    for step, (takes, final, cur) in enumerate(packets(utts, sf.accepts, sf.pending, sf.n_first, sf.n_next, random.Random(seed), cap)):
        out.fill_(float("nan"))
        got = sf.step(block_of(utts, takes, cur, dtype, garbage, seed=100 + step), out, sample_lens=takes, final=final)
        assert got is out
        outs.append(out.clone())
        if not check:
            continue
        carry, fresh, pos, carry_len = sf._state
        assert carry_len.tolist() == sf.schedule.carry and pos.tolist() == sf.schedule.pos and fresh.tolist() == [0] * B, step
        assert sf.frame_lens.tolist() == [m for _, m in sf.windows], step
        for b, (first, m) in enumerate(sf.windows):
            assert torch.equal(out[b, :m], ref[b, first:first + m]), (step, b, first, m)
            assert bool((out[b, m:] == 0).all()), (step, b, m)
            if m >= 7:
                ran[b].append((first, m))
    if check:
        assert ran == [ref_windows(num_frames(len(u)), 2) for u in utts]
        assert len(outs) >= 10
    carry, _, _, carry_len = sf._state
    return outs, [carry[b, :n].clone() for b, n in enumerate(carry_len.tolist())]


FBANK_LENGTHS = [399, samples_for(19), 32000, samples_for(15, 77)]           # below one frame; ends on a whole window; 25 windows; ends on a 7-frame window


@pytest.mark.parametrize("dtype", [torch.int16, torch.float32])
@pytest.mark.parametrize("dither", [0.0, 0.1])
def test_features_equal_offline_bit_for_bit_for_random_packets(dither, dtype):
    utts = utterances(FBANK_LENGTHS, 0)
    utts[2] = clip(True).copy()                                              # with its stretch of digital silence
    ref = offline(utts, dither, dtype=dtype)
    if dither:
        assert not torch.equal(ref, offline(utts, 0.0, dtype=dtype))
    run_fbank(utts, ref, dither, dtype, seed=11, cap=2500)
    run_fbank(utts, ref, dither, dtype, seed=12, cap=600)


def test_whole_blocks_unchanged_and_the_switch_keeps_the_windows():
    import fbank
    B, chunk = 3, 2
    sf = fbank.StreamingFbank(B, chunk, DEV, dither=0.1, seed=5)
    total = sf.n_first + 5 * sf.n_next
    sig = long_signal()
    wave = np.stack([sig[s:s + total] for s in (0, 7000, 13000)])
    ref, _ = fbank.KaldiFbank(dither=0.1, seed=5)(torch.from_numpy(wave).to(DEV), torch.full((B,), total, dtype=torch.int32, device=DEV))
    out = torch.empty((B, sf.window, 80), dtype=torch.float32, device=DEV)
    cursor = 0
    for step in range(6):
        n = sf.n_first if step == 0 else sf.n_next
        blk = torch.from_numpy(wave[:, cursor:cursor + n].copy()).to(DEV)
        if step < 3:
            sf.step(blk, out)                                                # the whole-block path: no lengths were ever given
            assert sf.schedule is None and sf.frame_lens is None and len(sf._state) == 3 and sf._state[0].shape[1] == sf.carry_n
        elif step == 3:
            assert sf.accepts() == [sf.n_first + sf.n_next - 1 - sf.carry_n] * B
            sf.step(blk, out, sample_lens=[sf.n_next] * B)                   # the switch: the carry is widened
        else:
            sf.step(blk, out)                                                # after it: samples.shape[1] new samples per stream
        assert torch.equal(out, ref[:, step * sf.hop: step * sf.hop + sf.window]), step
        if step >= 3:
            assert sf.frame_lens.tolist() == [sf.window] * B and sf._state[3].tolist() == [sf.carry_n] * B and sf._state[2].tolist() == [(step + 1) * sf.hop] * B
        cursor += n
    s2 = fbank.StreamingFbank(B, chunk, DEV, dither=0.1, seed=5)             # packets from the first call on
    s2.step(torch.from_numpy(wave[:, :s2.n_first].copy()).to(DEV), out, sample_lens=[s2.n_first] * B)
    assert torch.equal(out, ref[:, :s2.window])
    with pytest.raises(ValueError, match="stream 0 is handed"):
        s2.step(torch.zeros((B, 4000), dtype=torch.int16, device=DEV), out)  # 4000 > accepts(): a refused call changes nothing
    with pytest.raises(ValueError, match="host values"):
        s2.step(torch.zeros((B, 10), dtype=torch.int16, device=DEV), out, sample_lens=torch.zeros(B, dtype=torch.int32, device=DEV))
    s2.step(torch.from_numpy(wave[:, s2.n_first:s2.n_first + s2.n_next].copy()).to(DEV), out)
    assert torch.equal(out, ref[:, s2.hop:s2.hop + s2.window])


def test_nothing_behind_a_streams_own_samples_is_read():
    utts = utterances(FBANK_LENGTHS, 0)
    ref = offline(utts, 0.1, dtype=torch.float32)
    base, carry = run_fbank(utts, ref, 0.1, torch.float32, seed=21, cap=900, garbage="zeros", check=False)
    for garbage in ("noise", "nan"):
        outs, c2 = run_fbank(utts, ref, 0.1, torch.float32, seed=21, cap=900, garbage=garbage, check=garbage == "nan")
        assert len(outs) == len(base) and all(torch.equal(a, b) for a, b in zip(outs, base)), garbage
        assert all(torch.equal(a, b) for a, b in zip(carry, c2)), garbage


# ----------------------------------------------------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def precision():
    import cfm
    before = cfm.get_precision()
    yield cfm.set_precision
    cfm.set_precision(before)


def models():
    import encoder
    _, meta = load_golden("stream_asr")
    enc = synth.load_synth_(encoder.ConformerEncoder(cmvn=None, **meta["cfg"]).eval(), meta["wseed"])
    enc.global_cmvn = clip_cmvn()
    h = meta["head"]
    pr, jn = greedy_ref.modules(h["V"], h["embed"], h["hidden"], h["P"], h["J"], h["layers"], meta["hseed"], enc_dim=meta["cfg"]["encoder_dim"], shaped=True)
    with torch.no_grad():
        jn.ffn_out.bias[meta["blank"]] += meta["blank_bias"]
    return enc.to(DEV), pr.to(DEV), jn.to(DEV), meta


def recognizer(m, B, chunk):
    import transducer
    enc, pr, jn, meta = m
    return transducer.StreamingRecognizer(enc, pr, jn, B, chunk, meta["left"], blank=meta["blank"], n_steps=meta["n_steps"])


def run_audio(rec, utts, rng=None, cap=None, graphs=None, only=None):
    """step_audio over the utterances (streams in `only`, the others get nothing and are final).  Per stream: [(first frame, frames, tokens, rows)]."""
    import fbank
    B = len(utts)
    probe = fbank.PacketSchedule(B, rec.chunk, 400, 160)
    accepts = lambda: rec.audio.accepts() if rec.audio is not None else probe.accepts()
    rows = [[] for _ in range(B)]
    for takes, final, cur in packets(utts, accepts, rec.pending, probe.n_first, probe.n_next, rng, cap):
        new = rec.step_audio(block_of(utts, takes, cur, torch.int16), sample_lens=takes, final=final)
        if graphs is not None:
            graphs.append(rec.encoder_stream.graph)
        lens = rec.encoder_stream.out_lens.tolist()
        for b, (first, m) in enumerate(rec.audio.windows):
            assert lens[b] == c_of(m)
            if m >= 7:
                rows[b].append((first, m, new[b], rec.encoder_out[b, :lens[b]].clone()))
            else:
                assert new[b] == []
    return rows


def run_driver(rec, feats, utts):
    """The same utterances from the OFFLINE features, cut by the reference's schedule: stream b's k-th window in step k, idle afterwards."""
    B, chunk, window = len(utts), rec.chunk, rec.window
    wins = [ref_windows(num_frames(len(u)), chunk) for u in utts]
    rows = [[] for _ in range(B)]
    for s in range(max(len(w) for w in wins)):
        buf = torch.zeros((B, window, feats.shape[2]), dtype=torch.float32, device=DEV)
        fl = [0] * B
        for b in range(B):
            if s < len(wins[b]):
                first, m = wins[b][s]
                buf[b, :m], fl[b] = feats[b, first:first + m], m
        new = rec.step(buf, frame_lens=fl)
        for b in range(B):
            if fl[b]:
                rows[b].append((wins[b][s][0], fl[b], new[b], rec.encoder_out[b, :c_of(fl[b])].clone()))
            else:
                assert new[b] == []
    return rows


def compare(got, want, exact, what):
    """Windows, tokens and valid encoder rows per stream.  Every caller asks for exact rows: they were measured bit-identical for aligned and for random
    packets (a stream's rows do not depend on what the other streams of the batch do in the same step); TOL_FP32 is what a caller would fall back to."""
    worst, tokens = 0.0, 0
    for b, (g, w) in enumerate(zip(got, want)):
        assert [(f, m) for f, m, _, _ in g] == [(f, m) for f, m, _, _ in w], (what, b)
        for k, ((_, _, tg, yg), (_, _, tw, yw)) in enumerate(zip(g, w)):
            assert tg == tw, (what, b, k, tg, tw)
            tokens += len(tg)
            worst = max(worst, float((yg.double() - yw.double()).abs().max() / yw.double().abs().max().clamp_min(1e-30)))
            if exact:
                assert torch.equal(yg, yw), (what, b, k, worst)
    print("  step_audio vs the offline-feature driver [%s]: %d tokens, encoder rows max|d|/max|ref| = %.3e" % (what, tokens, worst))
    assert worst < TOL_FP32, (what, worst)
    return tokens


E2E_LENGTHS = [samples_for(43, 11), samples_for(19), samples_for(30, 100), 900]       # windows of 11 x 4 + one of 11; two whole; 11, 11, 11, then 6 left; none


def test_tokens_do_not_depend_on_the_packets(precision):
    precision("fp32")
    m = models()
    utts = utterances(E2E_LENGTHS, 6000)
    feats = offline(utts)
    want = run_driver(recognizer(m, 4, 2), feats, utts)
    assert [len(w) for w in want] == [5, 2, 3, 0] and want[0][-1][1] == 11 and want[2][-1][:2] == (16, 11)
    aligned = recognizer(m, 4, 2)
    tokens = compare(run_audio(aligned, utts), want, True, "aligned packets")
    assert tokens > 0 and aligned.hyps() == [sum((t for _, _, t, _ in w), []) for w in want]
    # the documented drain call on a finished recogniser: a (B, 0) block (no sample pointer at all) is an idle step
    empty = torch.zeros((4, 0), dtype=torch.int16, device=DEV)
    assert empty.data_ptr() == 0 and aligned.pending() == []
    off, y = aligned.encoder_stream.offsets.clone(), aligned.encoder_out.clone()
    assert aligned.step_audio(empty, sample_lens=[0] * 4, final=[True] * 4) == [[], [], [], []]
    assert all(m < 7 for m in aligned.audio.frame_lens.tolist()) and aligned.encoder_stream.out_lens.tolist() == [0] * 4
    assert torch.equal(aligned.encoder_stream.offsets, off) and not bool(aligned.encoder_out.any()) and aligned.audio._state[3].tolist() == aligned.audio.schedule.carry
    assert aligned.encoder_stream._host_off == off.tolist()                   # the host's offset bound follows each stream's own frames, idle steps included
    graphs = []
    for seed, cap in ((3, 400), (4, 3279)):
        rec = recognizer(m, 4, 2)
        compare(run_audio(rec, utts, random.Random(seed), cap, graphs if cap == 400 else None), want, True, "random packets, at most %d" % cap)
        assert rec.hyps() == aligned.hyps()
    # one capture serves every packetisation
    assert len(graphs) >= 20 and graphs[0] is not None and all(g is graphs[0] for g in graphs)
    # a stream reset in the middle of an utterance and reused: a fresh recogniser's tokens
    half = [u[:len(u) // 2] if b == 0 else u[:0] for b, u in enumerate(utts)]
    fresh = recognizer(m, 4, 2)
    src = max(range(4), key=lambda b: len(aligned.hyps()[b]))                 # the utterance with the most tokens, now on stream 0
    other = [utts[src] if b == 0 else u[:0] for b, u in enumerate(utts)]
    want_other = run_audio(fresh, other, random.Random(9), 1000)
    assert rec.pending() == []                                               # every stream of `rec` is drained: start over on stream 0, stop half way (not final)
    graph = rec.encoder_stream.graph
    rec.reset([0])
    assert rec.hyps()[0] == [] and rec.hyps()[1] == aligned.hyps()[1]
    n = len(half[0])
    rec.step_audio(block_of(half, [2000, 0, 0, 0], [0] * 4, torch.int16), sample_lens=[2000, 0, 0, 0], final=[False, True, True, True])
    rec.step_audio(block_of(half, [n - 2000, 0, 0, 0], [2000, 0, 0, 0], torch.int16), sample_lens=[n - 2000, 0, 0, 0], final=[False, True, True, True])
    assert rec.encoder_stream.offsets.tolist()[0] == 4 and rec.audio.schedule.pos[0] == 16          # two whole windows into the utterance
    rec.reset([0])
    got_other = run_audio(rec, other, random.Random(10), 1500)
    compare(got_other, want_other, True, "after a reset mid-utterance")
    assert rec.hyps()[0] == fresh.hyps()[0] and len(rec.hyps()[0]) > 0 and rec.hyps()[1:] == aligned.hyps()[1:]
    assert graph is not None and rec.encoder_stream.graph is graph


def test_chunk16_64_streams_a_quarter_ending_on_short_windows(precision):
    precision("fp32")
    m = models()
    B, chunk = 64, 16
    short = [7, 8, 23, 40, 66, 9, 37, 65]
    lengths = [samples_for(64 + short[(b // 4) % 8], 13 * b % 160) if b % 4 == 0 else samples_for(67 + 64) for b in range(B)]
    lengths[2], lengths[3] = 300, samples_for(64 + 6)                         # no frame at all; one whole window and 6 frames left
    utts = utterances(lengths, 1500)
    feats = offline(utts)
    want = run_driver(recognizer(m, B, chunk), feats, utts)
    assert [len(w) for w in want[:5]] == [2, 2, 0, 1, 2] and {w[-1][1] for w in want[::4]} == set(short)
    rec = recognizer(m, B, chunk)
    compare(run_audio(rec, utts), want, True, "64 streams, aligned packets")
    rnd = recognizer(m, B, chunk)
    compare(run_audio(rnd, utts, random.Random(1), 21000), want, True, "64 streams, random packets")
    assert rnd.hyps() == rec.hyps() and sum(len(h) for h in rec.hyps()) > 0
