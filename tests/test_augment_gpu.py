"""GPU: training augmentation on the device -- augment.SpeedPerturb (cfm_resample_group, csrc/resample.hip), augment.SpecAugment (cfm_spec_augment,
csrc/augment.hip) and augment.TrainFrontend.

  1. grouped resampling: batches of 6 items that mix the speeds 0.9 / 1.0 / 1.1, int16 and float32, every operand between guard bands, the columns
     past an item's samples poisoned (NaN; int16: full scale).  Item b equals cfm.resample on that item alone at its rate pair BIT FOR BIT, an
     identity item equals its input exactly, out_lens = ceil(n len / o) with exact +0.0 behind them, and each perturbed item passes the float64
     gate of tests/test_resample_gpu.py, |y - y_ref| <= (k + 2) 2^-24 sum |h| |x|.  Lengths per bank: 0, 1, o - 1, o + 1, 2 width + o + 1 and
     the two sides of the bank's tile edge;
  2. SpecAugment equals the integer reference (tests/spec_augment_ref.py) exactly: masked elements +0.0f, every other bit of the buffer -- NaNs,
     rows past an item's length, the stride gap, the guard bands -- untouched; the masks table; the same (seed, step, ids) twice; another step;
  3. TrainFrontend equals its stages called one by one, and a train-mode encoder takes what it returns."""
import functools

import numpy as np
import pytest
import torch

import extent
import spec_augment_ref as S
import test_resample_gpu as TR
from test_fbank_gpu import long_signal

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SPEEDS = (0.9, 1.0, 1.1)
IDENTITY_TILE = 2048                                                          # csrc/resample.hip: an identity bank copies in tiles of kTileOut samples


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(None)
def perturb():
    import augment
    return augment.SpeedPerturb(SPEEDS)


@functools.lru_cache(None)
def single(k):
    import resample
    return resample.Resampler(perturb().pairs[k][0])


def bank_lengths(k):
    o, n, width, _, _, _, _, tb = perturb().banks[k]
    edge = tb * o if o != n else IDENTITY_TILE                                # an input of `edge` samples ends on a tile's last output sample
    if o != n:
        assert perturb().num_samples(edge, k) == tb * n and perturb().num_samples(edge + 1, k) > tb * n
    return [0, 1, o - 1, o + 1, 2 * width + o + 1, edge, edge + 1]


def batches():
    """Four batches of six (bank, length): the 21 cases dealt round so that every batch mixes all three banks, filled up with three more."""
    cases = [(k, L) for i in range(7) for k, L in ((k, bank_lengths(k)[i]) for k in (0, 1, 2))]
    cases += [(2, 700), (0, 3), (1, 5)]
    return [cases[i::4] for i in range(4)]


@pytest.mark.parametrize("dtype", [torch.int16, torch.float32])
def test_grouped_resample_equals_the_single_pair_kernel_bit_for_bit(dtype):
    import cfm
    sp = perturb()
    assert sp.geometry == [(9, 10), (1, 1), (11, 10)]
    rng = np.random.default_rng(5 if dtype == torch.int16 else 6)
    worst, seen = 0.0, set()
    for batch in batches():
        assert {k for k, _ in batch} == {0, 1, 2}
        N = max(L for _, L in batch) + 3                                      # columns no item owns
        if dtype == torch.int16:
            x = rng.integers(-32768, 32768, size=(6, N)).astype(np.int16)
            for b, (_, L) in enumerate(batch):
                x[b, L:] = 32767
        else:
            x = rng.standard_normal((6, N)).astype(np.float32)
            for b, (_, L) in enumerate(batch):
                x[b, L:] = np.nan
        cap = max(sp.num_samples(N, k) for k, _ in batch)
        g = extent.Guards(DEV)
        xs = g.inp(torch.from_numpy(x), name="samples")
        lens = g.inp(torch.tensor([L for _, L in batch], dtype=torch.int32), name="lengths")
        bank = g.inp(torch.tensor([k for k, _ in batch], dtype=torch.int32), name="bank")
        tables = tuple(g.inp(t, name="table") for t in sp._host)
        out = g.out((6, cap), name="out")
        out_lens = g.out((6,), torch.int32, name="out_lens")
        cfm.resample_group(xs, lens, bank, tables, sp.banks, out, out_lens)
        torch.cuda.synchronize()
        g.check()
        got_lens = out_lens.cpu().tolist()
        assert got_lens == [sp.num_samples(L, k) for k, L in batch], (batch, got_lens)
        for b, (k, L) in enumerate(batch):
            m = got_lens[b]
            assert bool((bits(out[b, m:]) == 0).all()), ("not +0.0 behind the item", batch, b)
            if sp.geometry[k][0] == sp.geometry[k][1]:
                assert m == L and torch.equal(bits(out[b, :m]), bits(xs[b, :L].to(torch.float32))), ("identity item", batch, b)
                continue
            rs = single(k)
            one = torch.empty((1, rs.num_samples(N)), dtype=torch.float32, device=DEV)
            one_len = torch.empty((1,), dtype=torch.int32, device=DEV)
            cfm.resample(xs[b:b + 1], lens[b:b + 1], rs.tables(DEV), rs.geometry, one, one_len)
            assert int(one_len) == m and torch.equal(bits(out[b, :m]), bits(one[0, :m])), ("differs from cfm.resample on the item alone", batch, b)
            worst = max(worst, TR.gate(rs, sp.pairs[k][0], x[b, :L], out[b, :m].cpu().numpy(), "item of %d samples at speed %g" % (L, SPEEDS[k])))
            seen.add((k, L))
    assert len(seen) == 14 + 2
    print("  speeds 0.9 / 1.1, %s: worst |y_dev - y_ref| = %.2f x 2^-24 sum|h||x|" % (dtype, worst))


def test_speed_perturb_forward_sizes_from_the_columns():
    sp = perturb()
    x = torch.from_numpy(long_signal()[:5000].copy()).to(DEV).repeat(3, 1)
    lens = torch.tensor([5000, 4000, 0], dtype=torch.int32, device=DEV)
    y, n = sp(x, lens, [1, 0, 2])
    assert y.shape == (3, sp.num_samples(5000, 0)) and n.tolist() == [5000, sp.num_samples(4000, 0), 0]
    assert torch.equal(y[0, :5000], x[0].float()) and bool((y[0, 5000:] == 0).all()) and bool((y[2] == 0).all())
    y2, n2 = sp(x, lens, torch.tensor([2, 2, 2]))
    assert y2.shape == (3, sp.num_samples(5000, 2)) and n2.tolist() == [sp.num_samples(5000, 2), sp.num_samples(4000, 2), 0]
    with pytest.raises(ValueError, match="host values"):
        sp(x, lens, torch.tensor([0, 1, 2], device=DEV))


def poisoned_feats(F, seed):
    """Random features with a few planted NaNs inside the items and NaN in every row at or past an item's length."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((5, S.T_MAX, F)).astype(np.float32) + 2.0
    for b, T in enumerate(S.LENGTHS):
        x[b, T:] = np.nan
        if T > 2:
            x[b, rng.integers(0, T, size=3), rng.integers(0, F, size=3)] = np.nan
    return x


@pytest.mark.parametrize("F", S.FEATURES)
@pytest.mark.parametrize("counts", S.COUNTS)
def test_spec_augment_equals_the_integer_reference_exactly(F, counts):
    import augment
    nt, nf = counts
    x = poisoned_feats(F, 31 * F + nt)
    ids = torch.tensor(S.IDS, dtype=torch.int64, device=DEV)
    aug = augment.SpecAugment(nt, nf, S.MAX_T, S.MAX_F, seed=S.SEED)
    assert S.MAX_T > S.LENGTHS[2] > 1 and (S.MAX_F > F) == (F == 5)              # masks longer than an item, and than the feature axis

    def run(step):
        g = extent.Guards(DEV)
        feats = g.io(torch.from_numpy(x), ld=F + 3, name="feats")                # a stride gap of three floats behind every row
        lens = g.inp(torch.tensor(S.LENGTHS, dtype=torch.int32), name="lengths")
        masks = g.out((5, nt + nf, 2), torch.int32, name="masks")
        assert feats.stride() == (S.T_MAX * (F + 3), F + 3, 1)
        back = aug(feats, lens, ids=ids, step=step, masks=masks)
        torch.cuda.synchronize()
        g.check()
        assert back is feats
        return feats.cpu().numpy(), masks.cpu().numpy()

    tables = [S.mask_table(S.step_seed(S.SEED, s), S.IDS, S.LENGTHS, S.T_MAX, F, nt, nf, S.MAX_T, S.MAX_F) for s in S.STEPS]
    assert not np.array_equal(*tables)
    for step, table in zip(S.STEPS, tables):
        got, masks = run(step)
        want = S.apply_table(x, S.LENGTHS, table, nt)
        assert np.array_equal(masks, table), (step, masks.tolist(), table.tolist())
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), "step %d: the buffer differs from the reference in %d elements" % (
            step, int((got.view(np.int32) != want.view(np.int32)).sum()))
        changed = got.view(np.int32) != x.view(np.int32)
        assert changed.any() and bool((got.view(np.int32)[changed] == 0).all())   # something was masked, and only with +0.0f
        assert not changed[0].any() and bool(np.isnan(got[1, 1:]).all())           # the empty item; rows past a length keep their NaN
    again, masks = run(S.STEPS[0])
    assert np.array_equal(again.view(np.int32), S.apply_table(x, S.LENGTHS, tables[0], nt).view(np.int32)) and np.array_equal(masks, tables[0])


def test_spec_augment_defaults_count_steps_and_number_the_items():
    import augment
    x = torch.from_numpy(poisoned_feats(80, 1)).to(DEV)
    lens = torch.tensor(S.LENGTHS, dtype=torch.int32, device=DEV)
    aug = augment.SpecAugment(seed=77)
    for step in (0, 1):                                                          # the call counter is the step, arange(B) the ids
        masks = torch.full((5, 4, 2), -1, dtype=torch.int32, device=DEV)
        aug(x.clone(), lens, masks=masks)
        assert np.array_equal(masks.cpu().numpy(), S.mask_table(S.step_seed(77, step), range(5), S.LENGTHS, S.T_MAX, 80, 2, 2, 50, 50))
    empty = torch.empty((2, 0, 80), dtype=torch.float32, device=DEV)             # no frame at all: nothing to do, the table is zeros
    masks = torch.full((2, 4, 2), -1, dtype=torch.int32, device=DEV)
    aug(empty, torch.zeros(2, dtype=torch.int32, device=DEV), masks=masks)
    assert not masks.any()


def test_train_frontend_equals_its_stages_and_feeds_the_encoder():
    import augment
    import cfm
    import encoder
    import fbank
    import resample
    import synth
    sig = long_signal()
    lengths = [4800, 9600, 6123, 7777]                                           # 0.3 .. 0.6 s
    x = np.zeros((4, max(lengths)), np.int16)
    for b, L in enumerate(lengths):
        x[b, :L] = sig[4000 * b: 4000 * b + L]
    x, lens = torch.from_numpy(x).to(DEV), torch.tensor(lengths, dtype=torch.int32, device=DEV)
    choice, step = [0, 1, 2, 0], 5
    sp, spec, fb = augment.SpeedPerturb(SPEEDS), augment.SpecAugment(seed=9), fbank.KaldiFbank(dither=0.1, seed=21)
    front = augment.TrainFrontend(speed=sp, fbank=fb, spec=spec)
    feats, feats_length = front(x, lens, step, choice=choice)

    w, wl = augment.SpeedPerturb(SPEEDS)(x, lens, choice)
    f, fl = fbank.KaldiFbank(dither=0.1, seed=21).forward(w, wl, seed=augment.step_seed(21, step))
    plain = f.clone()
    augment.SpecAugment(seed=9)(f, fl, step=step)
    assert feats.shape == f.shape and torch.equal(bits(feats), bits(f)) and torch.equal(feats_length, fl)
    assert feats_length.tolist() == [fb.num_frames(sp.num_samples(L, k)) for L, k in zip(lengths, choice)]
    assert feats.shape[1] == fb.num_frames(sp.num_samples(max(lengths), 0)) and bool((feats != plain).any()) and bool((feats[feats != plain] == 0).all())
    other, _ = front(x, lens, step + 1, choice=choice)                           # another step: other dither, other masks
    assert not torch.equal(bits(other), bits(feats))

    bare = augment.TrainFrontend(fbank=fb)                                       # no augmentation: KaldiFbank alone
    assert bare.resampler is None and bare.speed is None and bare.spec is None
    a, al = bare(x, lens, step)
    b, bl = fb.forward(x, lens, seed=augment.step_seed(21, step))
    assert torch.equal(bits(a), bits(b)) and torch.equal(al, bl) and al.tolist() == [fb.num_frames(L) for L in lengths]
    a, al = augment.TrainFrontend(resampler=8000, fbank=fb)(x, lens, step)      # a source rate: resample.Resampler first
    b, bl = fb.forward(*resample.Resampler(8000)(x, lens), seed=augment.step_seed(21, step))
    assert torch.equal(bits(a), bits(b)) and torch.equal(al, bl)
    assert isinstance(augment.TrainFrontend().fbank, fbank.KaldiFbank) and augment.TrainFrontend().fbank.dither == 0.1

    cfg = dict(input_dim=80, kernel_size=15, encoder_dim=144, dropout=0.1, attention_dropout=0.1, pos_enc_dropout=0.1, hidden_dim=576, num_heads=4,
               encoder_num_layers=2, max_len=5000, use_relative=True)                # BASELINE config 1
    enc = synth.load_synth_(encoder.ConformerEncoder(cmvn=None, **cfg), 11).to(DEV).train()
    (y, mask), = enc.forward_window([(feats, feats_length)])
    torch.cuda.synchronize()
    assert y.shape[0] == 4 and y.shape[2] == 144 and bool(torch.isfinite(y).all())
    assert tuple(mask.shape) == (4, 1, y.shape[1]) and y.shape[1] == ((feats.shape[1] - 1) // 2 - 1) // 2
