"""CPU (no GPU): the host side of training augmentation (augment.py; include/cfm.h cfm_spec_augment / cfm_resample_group).

  1. the integer restatement of the SpecAugment draws (tests/spec_augment_ref.py) against the reference-style loop fed the same integers; the
     multiply-high draw reaches both ends of its range and nothing else; end <= T; T == 0 has no masks; another step is another table for the
     seeds tests/test_augment_gpu.py uses;
  2. SpeedPerturb's geometry (0.9 -> 9:10, 1.1 -> 11:10, 1.0 the identity, 0.95 -> 19:20), its output lengths against tests/resample_ref.py, the
     concatenated tables against packing.resample_tables, a speed that does not fit;
  3. argument validation, and no CPU path."""
import numpy as np
import pytest
import torch

import resample_ref as R
import spec_augment_ref as S


def test_hash_matches_a_plain_python_statement():
    def h32(seed, idx):
        h = ((idx * 0x9E3779B1) & S.M32) ^ seed
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & S.M32
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & S.M32
        return h ^ (h >> 16)
    rng = np.random.default_rng(0)
    for seed, idx in rng.integers(0, 1 << 32, size=(200, 2), dtype=np.uint64).tolist() + [[0, 0], [S.M32, S.M32]]:
        assert int(S.hash32(seed, idx)) == h32(seed, idx)
    assert S.step_seed(S.M32, 1) == (S.M32 + 0x9E3779B1) % (1 << 32) and S.step_seed(5, 0) == 5


@pytest.mark.parametrize("N", [1, 2, 50, 80])
def test_draws_cover_their_range_and_nothing_else(N):
    r = S.hash32(S.hash32(S.SEED, np.arange(1000, dtype=np.uint64)[:, None]), np.arange(100, dtype=np.uint64)[None, :]).reshape(-1)
    assert r.size == 10 ** 5
    u = S.uniform(r, N)
    assert int(u.min()) == 0 and int(u.max()) == N - 1
    counts = np.bincount(u, minlength=N)
    assert counts.size == N and bool((np.abs(counts - r.size / N) < 6 * np.sqrt(r.size / N) + 1).all())     # 6 sigma of a fair draw
    assert int(S.uniform(0, N)) == 0 and int(S.uniform(S.M32, N)) == N - 1                                # the ends of the 32-bit range


@pytest.mark.parametrize("F", S.FEATURES)
@pytest.mark.parametrize("counts", S.COUNTS)
def test_integer_reference_agrees_with_the_reference_style_loop(F, counts):
    nt, nf = counts
    rng = np.random.default_rng(F)
    seed = S.step_seed(S.SEED, S.STEPS[0])
    table = S.mask_table(seed, S.IDS, S.LENGTHS, S.T_MAX, F, nt, nf, S.MAX_T, S.MAX_F)
    assert table.shape == (5, nt + nf, 2) and table.dtype == np.int32
    feats = rng.standard_normal((5, S.T_MAX, F)).astype(np.float32) + 3.0           # no zero to begin with
    got = S.apply_table(feats, S.LENGTHS, table, nt)
    for b, T in enumerate(S.LENGTHS):
        if T == 0:
            assert not table[b].any() and np.array_equal(got[b], feats[b])
            continue
        d = S.draws(seed, S.IDS[b], T, F, nt, nf, S.MAX_T, S.MAX_F)
        want, pairs = S.reference_loop(feats[b, :T], nt, nf, S.MAX_T, S.MAX_F, S.replay(d))
        assert pairs == [tuple(p) for p in table[b].tolist()]
        assert np.array_equal(got[b, :T], want) and np.array_equal(got[b, T:], feats[b, T:])
        assert bool((table[b, :nt, 1] <= T).all()) and bool((table[b, nt:, 1] <= F).all()) and bool((table[b, :, 0] < table[b, :, 1]).all())
        assert bool((table[b, :nt, 0] < T).all()) and bool((table[b, nt:, 0] < F).all())


def test_end_never_passes_the_item_and_steps_differ():
    for T in (1, 2, 49, 50, 51, 1650):
        for item in range(50):
            t = S.mask_table(S.SEED, [item], [T], 4000, 80, 2, 2, S.MAX_T, S.MAX_F)[0]
            assert 0 <= t[:2, 0].min() and t[:2, 1].max() <= T and t[2:, 1].max() <= 80 and bool((t[:, 1] - t[:, 0] >= 1).all()) and bool((t[:, 1] - t[:, 0] <= 50).all())
    assert not S.mask_table(S.SEED, [0, 1], [0, -3], 64, 80, 2, 2, 50, 50).any()           # T == 0: no masks
    assert not S.mask_table(S.SEED, [0], [10], 64, 0, 2, 2, 50, 50).any()                   # no columns: none either
    for F in S.FEATURES:
        for nt, nf in S.COUNTS:
            a, b = (S.mask_table(S.step_seed(S.SEED, s), S.IDS, S.LENGTHS, S.T_MAX, F, nt, nf, S.MAX_T, S.MAX_F) for s in S.STEPS)
            assert not np.array_equal(a, b), (F, nt, nf)
    # other ids, other masks
    assert not np.array_equal(S.mask_table(S.SEED, [1], [64], 64, 80, 2, 2, 50, 50), S.mask_table(S.SEED, [2], [64], 64, 80, 2, 2, 50, 50))


def test_speed_perturb_geometry_and_lengths():
    import augment
    from cfm import packing
    sp = augment.SpeedPerturb((0.9, 1.0, 1.1, 0.95))
    assert sp.pairs == [(14400, 16000), (16000, 16000), (17600, 16000), (15200, 16000)]
    assert sp.geometry == [(9, 10), (1, 1), (11, 10), (19, 20)]
    for k, (orig, new) in enumerate(sp.pairs):
        for L in (0, 1, 8, 9, 10, 11, 12, 1000, 16000, 264017):
            assert sp.num_samples(L, k) == R.num_samples(L, orig, new), (k, L)
    assert sp.num_samples(16000, 0) == 17778 and sp.num_samples(16000, 1) == 16000 and sp.num_samples(16000, 2) == 14546
    # the concatenated tables are the single-pair tables end to end, and the rows say where
    taps, first, off = sp._host
    at = [0, 0, 0]
    for (orig, new), row in zip(sp.pairs, sp.banks):
        o, n, width, n_live, taps_at, first_at, off_at, tb = row
        assert (o, n, width) == R.geometry(orig, new)[:2] + (R.geometry(orig, new)[3],)
        if o == n:
            assert row[3:] == (0, 0, 0, 0, 0)
            continue
        t, f, q = packing.resample_tables(orig, new)
        assert [taps_at, first_at, off_at] == at and n_live == t.numel() and tb > 0
        assert torch.equal(taps[taps_at:taps_at + n_live], t) and torch.equal(first[first_at:first_at + n], f) and torch.equal(off[off_at:off_at + n + 1], q)
        at = [at[0] + t.numel(), at[1] + n, at[2] + n + 1]
    assert [taps.numel(), first.numel(), off.numel()] == at
    only = augment.SpeedPerturb((1.0,))
    assert only._host is None and only.tables("cpu") is None and only.num_samples(77, 0) == 77
    # the default: the reference's three speeds, and draws that are a function of the seed
    a, b = augment.SpeedPerturb(seed=5), augment.SpeedPerturb(seed=5)
    assert a.speeds == (0.9, 1.0, 1.1) and a.draw(64) == b.draw(64) and set(a.draw(200)) == {0, 1, 2}


def test_a_speed_that_does_not_fit_raises():
    import augment
    with pytest.raises(ValueError, match="phases"):
        augment.SpeedPerturb((0.9001,))                                          # 14401 : 16000 does not reduce: 16000 phases
    with pytest.raises(ValueError):
        augment.SpeedPerturb((1.0, 0.0))
    with pytest.raises(ValueError, match="RESAMPLE_MAX_BANKS"):
        augment.SpeedPerturb((0.9,) * 9)
    with pytest.raises(ValueError, match="LDS"):
        from cfm import packing
        packing.resample_group_tables([(14400, 16000)], lambda o, n, width: 0)


def test_argument_validation_and_no_cpu_path():
    import augment
    with pytest.raises(ValueError, match="at most 32"):
        augment.SpecAugment(num_t_mask=20, num_f_mask=13)
    augment.SpecAugment(num_t_mask=20, num_f_mask=12)
    with pytest.raises(ValueError, match="max_t 0"):
        augment.SpecAugment(max_t=0)
    with pytest.raises(ValueError, match="max_f -1"):
        augment.SpecAugment(max_f=-1)
    sp = augment.SpeedPerturb()
    assert sp.check([0, 2, 1], 3) == [0, 2, 1] and sp.check(torch.tensor([2, 2]), 2) == [2, 2]
    with pytest.raises(ValueError, match="an index into the 3 speeds"):
        sp.check([0, 3], 2)
    with pytest.raises(ValueError, match="2 choices for 3 items"):
        sp.check([0, 1], 3)
    with pytest.raises(ValueError, match="integers"):
        sp.check(torch.tensor([0.0, 1.0]), 2)
    with pytest.raises(ValueError, match="host values"):
        sp.check(torch.zeros(2, dtype=torch.int64, device="meta"), 2)            # any device but the host's
    x, lens = torch.zeros((2, 400), dtype=torch.int16), torch.tensor([400, 300], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sp(x, lens)
    with pytest.raises(RuntimeError, match="no CPU path"):
        augment.SpecAugment()(torch.zeros(2, 10, 80), torch.tensor([10, 5], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        augment.TrainFrontend(speed=sp, spec=augment.SpecAugment())(x, lens, 0)
    assert augment.step_seed(7, 3) == (7 + 3 * 0x9E3779B1) % (1 << 32)
