"""GPU: fbank.KaldiFbank / fbank.StreamingFbank (csrc/fbank.hip) and transducer.StreamingRecognizer.step_audio against tests/fbank_ref.py,
the torch restatement of torchaudio.compliance.kaldi.fbank, evaluated on the CPU in the same run.

  1. parity, dither 0: E_dev = max |device - float64 restatement| and E_f32 = max |float32 restatement - float64 restatement| over the
     unfloored cells; the gate is E_dev <= 2 E_f32 (the float32 restatement is what torchaudio computes).  Floored cells are floored on the
     device too, rows past an item's frame count are exactly 0, feats_length is exact.  int16 and float32 input.
  2. range: a full-scale square wave passes the same gate and stays finite.
  3. streaming equals offline bit for bit, chunk 2 and 16, with a stream reset half way, with and without dither.
  4. dither: seeded, and statistically the restatement's (the 0.2 bound: the worst cell is a one-FFT-bin mel filter, whose log-energy is the log
     of an exponential variate, standard deviation 1.28; two independent means over 2000 frames differ with sigma 1.28 sqrt(2 / 2000) = 0.04).
  5. step_audio(samples) returns exactly the tokens of step(windows cut from KaldiFbank's offline features)."""
import functools
import math

import numpy as np
import pytest
import torch

import fbank_ref as R
import greedy_ref
import synth
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
LOG_EPS = math.log(R.EPS)


@functools.lru_cache(None)
def clip(zeroed=False):
    g, _ = load_golden("fbank")
    pcm = g["pcm"].copy()
    if zeroed:
        pcm[8000:9000] = 0
    return pcm


@functools.lru_cache(None)
def long_signal():
    """The clip, periodically extended: chunk-16 streaming reads 62 160 samples per stream in six steps."""
    return np.tile(clip(), 4)


def gate(dev, sig, **kw):
    """(E_dev, E_f32, floored cells) of one item; asserts the floor."""
    f64 = R.fbank(sig, dtype=torch.float64, **kw)
    f32 = R.fbank(sig, dtype=torch.float32, **kw)
    assert dev.shape == f64.shape, (dev.shape, f64.shape)
    floored = (f64 - LOG_EPS).abs() < 1e-9
    if floored.any():
        assert float((dev.double()[floored] - LOG_EPS).abs().max()) <= 1e-5
    if floored.all():
        return 0.0, 0.0, int(floored.sum())
    return float((dev.double() - f64)[~floored].abs().max()), float((f32.double() - f64)[~floored].abs().max()), int(floored.sum())


@pytest.mark.parametrize("dtype", [torch.int16, torch.float32])
def test_parity_ragged_batch(dtype):
    import fbank
    sigs = [clip()[5000:5400], clip()[12000:16000], clip(True), clip()[:399]]
    lens = [len(s) for s in sigs]
    assert lens == [400, 4000, 32000, 399]
    batch = np.full((4, 32000), 1234, np.int16)                  # what lies past an item's length must not be read as signal
    for b, s in enumerate(sigs):
        batch[b, :len(s)] = s
    fb = fbank.KaldiFbank()
    feats, n = fb(torch.from_numpy(batch).to(DEV).to(dtype), torch.tensor(lens, dtype=torch.int32, device=DEV))
    assert feats.dtype == torch.float32 and tuple(feats.shape) == (4, 198, 80) and n.dtype == torch.int32
    assert n.tolist() == [1, 23, 198, 0]
    feats = feats.cpu()
    e_dev = e_f32 = 0.0
    nfl = []
    for b, s in enumerate(sigs):
        m = R.num_frames(len(s))
        assert bool((feats[b, m:] == 0).all()), "rows past the frame count of item %d" % b
        if m:
            d, f, k = gate(feats[b, :m], s)
            e_dev, e_f32 = max(e_dev, d), max(e_f32, f)
            nfl.append(k)
    print("fbank parity [%s]: E_dev %.3e, E_f32 %.3e, floored cells %s" % (dtype, e_dev, e_f32, nfl))
    assert nfl == [0, 0, 320]
    assert e_dev <= 2 * e_f32


def test_full_scale_square_wave():
    import fbank
    sig = np.where((np.arange(800) // 20) % 2 == 0, 32767, -32767).astype(np.int16)
    feats, n = fbank.KaldiFbank()(torch.from_numpy(sig)[None].to(DEV), torch.tensor([800], dtype=torch.int32, device=DEV))
    assert n.tolist() == [3] and bool(torch.isfinite(feats).all())
    e_dev, e_f32, _ = gate(feats[0].cpu(), sig)
    print("fbank square wave: E_dev %.3e, E_f32 %.3e" % (e_dev, e_f32))
    assert e_dev <= 2 * e_f32


@pytest.mark.parametrize("cfg", [dict(num_mel_bins=40, sample_frequency=8000), dict(num_mel_bins=20, frame_length=10, frame_shift=5, sample_frequency=8000),
                                 dict(num_mel_bins=64, frame_length=20, frame_shift=8)])
def test_other_window_sizes(cfg):
    """Padded windows of 256 (a radix-2 stage after the radix-4 ones), 128 and 512 with a 320-sample frame: the same gate."""
    import fbank
    sig = clip()[3000:9000]
    fb = fbank.KaldiFbank(**cfg)
    feats, n = fb(torch.from_numpy(sig)[None].to(DEV), torch.tensor([len(sig)], dtype=torch.int32, device=DEV))
    assert n.tolist() == [R.num_frames(len(sig), fb.win, fb.shift)] and feats.shape[1] == n.item()
    e_dev, e_f32, _ = gate(feats[0].cpu(), sig, **cfg)
    print("fbank %s: padded %d, E_dev %.3e, E_f32 %.3e" % (cfg, fb.padded, e_dev, e_f32))
    assert e_dev <= 2 * e_f32


@pytest.mark.parametrize("dither", [0.0, 0.1])
@pytest.mark.parametrize("chunk", [2, 16])
def test_streaming_equals_offline_bit_for_bit(chunk, dither):
    import fbank
    sf = fbank.StreamingFbank(3, chunk, DEV, dither=dither, seed=5)
    window, hop = (chunk - 1) * 4 + 7, 4 * chunk
    assert (sf.window, sf.hop, sf.carry_n) == (window, hop, 720)
    if chunk == 2:
        assert (sf.n_first, sf.n_next) == (2000, 1280)
    total = sf.n_first + 5 * sf.n_next
    sig = long_signal()
    starts, restart = [0, 7000, 13000], 21000
    first = np.stack([sig[s:s + total] for s in starts])
    second = first.copy()
    second[1] = sig[restart:restart + total]                       # stream 1's second utterance, at ITS index (the noise is keyed by the stream)
    off = fbank.KaldiFbank(dither=dither, seed=5)
    lens = torch.full((3,), total, dtype=torch.int32, device=DEV)
    ref1, _ = off(torch.from_numpy(first).to(DEV), lens)
    ref2, _ = off(torch.from_numpy(second).to(DEV), lens)
    if dither:
        plain, _ = fbank.KaldiFbank()(torch.from_numpy(first).to(DEV), lens)
        assert not torch.equal(plain, ref1)
    out = torch.empty((3, window, 80), dtype=torch.float32, device=DEV)
    cursor, frame = [0, 0, 0], [0, 0, 0]                           # samples / frames consumed of the stream's current utterance
    src = [first[0], first[1], first[2]]
    refs = [ref1[0], ref1[1], ref1[2]]
    fresh = [True] * 3
    with pytest.raises(ValueError, match="was reset"):
        sf.step(torch.zeros((3, sf.n_next), dtype=torch.int16, device=DEV), out)
    for step in range(6):
        if step == 3:
            sf.reset([1])
            src[1], refs[1], cursor[1], frame[1], fresh[1] = second[1], ref2[1], 0, 0, True
        width = sf.n_first if any(fresh) else sf.n_next
        block = np.full((3, width), -77, np.int16)                 # left-aligned; the rest of a row is not the stream's
        for b in range(3):
            n = sf.n_first if fresh[b] else sf.n_next
            block[b, :n] = src[b][cursor[b]:cursor[b] + n]
            cursor[b] += n
        sf.step(torch.from_numpy(block).to(DEV), out)
        for b in range(3):
            assert torch.equal(out[b], refs[b][frame[b]:frame[b] + window]), (chunk, dither, step, b)
            frame[b] += hop
        fresh = [False] * 3


def test_dither_is_seeded_and_has_the_restatements_statistics():
    import fbank
    x = torch.from_numpy(clip()[:8000].copy())[None].to(DEV)
    n = torch.tensor([8000], dtype=torch.int32, device=DEV)
    a, _ = fbank.KaldiFbank(dither=0.1, seed=3)(x, n)
    b, _ = fbank.KaldiFbank(dither=0.1, seed=3)(x, n)
    c, _ = fbank.KaldiFbank(dither=0.1, seed=4)(x, n)
    assert torch.equal(a, b) and not torch.equal(a, c)
    frames = 2000
    silence = torch.zeros((1, 400 + (frames - 1) * 160), dtype=torch.int16, device=DEV)
    dev, m = fbank.KaldiFbank(dither=1.0, seed=9)(silence, torch.tensor([silence.shape[1]], dtype=torch.int32, device=DEV))
    assert m.tolist() == [frames]
    torch.manual_seed(17)
    ref = R.fbank(np.zeros(silence.shape[1], np.int16), dither=1.0, dtype=torch.float32)
    diff = (dev[0].cpu().double().mean(0) - ref.double().mean(0)).abs()
    print("dither: per-bin mean log-mel differs by at most %.3f (bin %d)" % (float(diff.max()), int(diff.argmax())))
    assert float(diff.max()) <= 0.2


def clip_cmvn():
    """Global CMVN of the clip's own log-mel (float64 restatement), as the reference puts one between kaldi.fbank and its encoder: the
    synthetic weights are made for post-CMVN features ~ N(0, 1) (synth.fbank), and on raw log-mel of 5 to 28 the search emits only blanks."""
    import cmvn
    f = R.fbank(clip(), dtype=torch.float64)
    m = cmvn.GlobalCMVN.__new__(cmvn.GlobalCMVN)
    torch.nn.Module.__init__(m)
    m.norm_var = True
    m.register_buffer("mean", f.mean(0).float())
    m.register_buffer("istd", (1.0 / f.std(0)).float())
    return m


def test_step_audio_equals_step_on_offline_features():
    import cfm
    import encoder
    import fbank
    import transducer
    before = cfm.get_precision()
    cfm.set_precision("bf16")
    try:
        _, meta = load_golden("enc_cfg1_stream")
        enc = encoder.ConformerEncoder(cmvn=None, **meta["cfg"]).eval()
        synth.load_synth_(enc, meta["wseed"])
        enc.global_cmvn = clip_cmvn()
        enc = enc.to(DEV)
        pr, jn = greedy_ref.modules(73, 48, 80, 96, 64, 2, 51, enc_dim=meta["cfg"]["encoder_dim"], shaped=True)
        pr, jn = pr.to(DEV), jn.to(DEV)
        B, chunk, left, steps = 4, 16, 2, 4
        hop, window = 4 * chunk, (chunk - 1) * 4 + 7
        audio = transducer.StreamingRecognizer(enc, pr, jn, B, chunk, left, n_steps=3)
        frames = transducer.StreamingRecognizer(enc, pr, jn, B, chunk, left, n_steps=3)
        n_first, n_next = (window - 1) * 160 + 400, hop * 160
        total = n_first + (steps - 1) * n_next
        sig = np.stack([long_signal()[s:s + total] for s in (0, 9000, 17000, 26000)])
        wave = torch.from_numpy(sig).to(DEV)
        feats, _ = fbank.KaldiFbank()(wave, torch.full((B,), total, dtype=torch.int32, device=DEV))
        cursor, count = 0, 0
        for s in range(steps):
            n = n_first if s == 0 else n_next
            got = audio.step_audio(wave[:, cursor:cursor + n])
            y_audio = audio.encoder_out.clone()
            want = frames.step(feats[:, s * hop:s * hop + window].contiguous())
            assert torch.equal(audio.encoder_stream.input_buffer(), frames.encoder_stream.input_buffer())
            assert torch.equal(y_audio, frames.encoder_out) and got == want, s
            cursor += n
            count += sum(len(t) for t in got)
        assert audio.hyps() == frames.hyps() and count > 0
        audio.reset([2])
        assert audio.audio._fresh == [False, False, True, False] and audio.hyps()[2] == []
        with pytest.raises(ValueError, match="was reset"):
            audio.step_audio(wave[:, :n_next])
    finally:
        cfm.set_precision(before)
