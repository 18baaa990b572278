"""CPU: the sample-rate converter's specification (tests/resample_ref.py), its host tables (cfm.packing.resample_tables), the host mirror of the
streaming bookkeeping (resample.ResampleSchedule) and the binding's new entry points.  Nothing here needs a GPU."""
import math
import random

import numpy as np
import pytest
import torch

import resample_ref as R

RATES = [48000, 44100, 22050, 8000]


def signal(seed, n):
    return np.random.default_rng(seed).standard_normal(n)


@pytest.mark.parametrize("rate", RATES)
def test_convolution_form_equals_the_definition(rate):
    o, n, _, width = R.geometry(rate, 16000)
    L = 7 * o + 3
    x = signal(rate, L)
    y = R.resample(x, rate, 16000)
    rng = random.Random(rate)
    which = [0, 1, len(y) - 2, len(y) - 1] + [rng.randrange(len(y)) for _ in range(60)]   # 64 samples, the utterance's first and last among them
    err = np.abs(y[which] - R.resample_samples(x, rate, 16000, which)).max()
    print("  %d Hz: convolution form vs double loop on 64 samples: %.3e" % (rate, err))
    assert err <= 1e-12


@pytest.mark.parametrize("rate", RATES)
def test_output_length(rate):
    o, n, _, width = R.geometry(rate, 16000)
    for L in (0, 1, o - 1, o, o + 1, width, 2 * width + o + 1):
        assert len(R.resample(signal(L, L), rate, 16000)) == math.ceil(n * L / o) == R.num_samples(L, rate, 16000), (rate, L)


def test_sine_at_48k_comes_out_as_the_16k_sine():
    t48, t16 = np.arange(4800) / 48000.0, np.arange(1600) / 16000.0
    y = R.resample(np.sin(2 * math.pi * 1000.0 * t48), 48000, 16000)
    err = np.abs(y - np.sin(2 * math.pi * 1000.0 * t16))[50:-50].max()
    print("  1 kHz sine, 48 -> 16 kHz: max error away from the ends %.3e" % err)
    assert err <= 1e-3


@pytest.mark.parametrize("rate", RATES + [11025])
def test_compact_tables(rate):
    from cfm import packing
    h = R.kernel(rate, 16000)
    taps, first, off = packing.resample_tables(rate, 16000)
    o, n, _, width = packing.resample_geometry(rate, 16000)
    ro, rn, _, rwidth = R.geometry(rate, 16000)
    assert (o, n, width) == (ro, rn, rwidth)
    assert h.shape == (n, 2 * width + o) and first.numel() == n and off.numel() == n + 1 and int(off[-1]) == taps.numel()
    assert taps.numel() * 4 <= packing.RESAMPLE_MAX_TABLE_BYTES
    dense = packing.unpack_resample_tables(taps, first, off, h.shape[1]).numpy()
    live = np.zeros(h.shape, bool)
    for j in range(n):
        live[j, int(first[j]):int(first[j]) + int(off[j + 1] - off[j])] = True
        assert (np.abs(h[j, live[j]]) >= 2.0 ** -60).all(), j                        # a contiguous run: nothing below the threshold inside it
    assert np.array_equal(dense[live], h[live].astype(np.float32))                    # float32 rounding of the float64 bank, nothing else
    assert (dense[~live] == 0).all() and (np.abs(h[~live]) < 2.0 ** -60).all()        # every dropped tap is below 2^-60
    lens = (off[1:] - off[:-1]).tolist()
    print("  %d Hz: %d phases, %d..%d live taps of %d, %d bytes" % (rate, n, min(lens), max(lens), h.shape[1], taps.numel() * 4))
    assert {48000: (37, 37), 44100: (33, 34), 22050: (16, 17), 8000: (12, 13), 11025: (12, 13)}[rate] == (min(lens), max(lens))


def test_table_limits_raise():
    from cfm import packing
    with pytest.raises(ValueError, match="RESAMPLE_MAX_PHASES"):
        packing.resample_tables(12345, 16000)
    with pytest.raises(ValueError, match="RESAMPLE_MAX_TABLE_BYTES"):
        packing.resample_tables(1600000, 1000)                                       # 1600 samples per block, 19394 live taps


@pytest.mark.parametrize("rate", RATES)
def test_host_mirror_emits_what_the_rule_allows(rate):
    import resample
    o, n, _, width = R.geometry(rate, 16000)
    rng = random.Random(rate)
    L = rng.randrange(5 * o, 40 * o)
    cuts = sorted(rng.randrange(L + 1) for _ in range(199))
    cuts = [0] + cuts + [L]                                                           # 200 packets, repeated cut points are empty packets
    sch, ref = resample.ResampleSchedule(2, o, n, width), R.StreamRef(rate, 16000)
    total = 0
    for k in range(200):
        n_new, final = cuts[k + 1] - cuts[k], k == 199
        want = sch.produces([n_new, 0], [final, False])
        got = sch.advance([n_new, 0], [final, False])
        assert got == want and got[1] == 0
        assert got[0] == ref.push(n_new, final), k
        total += got[0]
        if not final:
            assert total == ref.exist(cuts[k + 1], False) and total % n == 0
            assert all((q + 1) * o + width <= cuts[k + 1] for q in range(total // n))  # every emitted block had all of its taps' samples
            assert 0 <= sch.held()[0] < width + o
    assert total == math.ceil(n * L / o)
    assert sch.seen == [0, 0] and sch.blocks == [0, 0]                                # a final packet leaves the stream reset
    assert sch.flush_max == math.ceil(n * (width + o - 1) / o)


def test_library_exports_the_resampler_at_version_307():
    import cfm
    lib = cfm.lib()
    assert lib.cfm_version() == 307
    assert lib.cfm_resample is not None and lib.cfm_resample_stream is not None
    for rate in RATES:
        o, n, _, width = R.geometry(rate, 16000)
        assert lib.cfm_resample_tile_blocks(o, n, width) >= 1
    assert lib.cfm_resample_tile_blocks(441, 2000, 17) == 0


def test_no_cpu_path():
    import resample
    rs = resample.Resampler(44100)
    assert rs.num_samples(44100) == 16000 and rs.num_samples(1) == 1 and rs.num_samples(0) == 0
    with pytest.raises(RuntimeError, match="no CPU path"):
        rs(torch.zeros((1, 100), dtype=torch.int16), torch.tensor([100], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        resample.Resampler(16000)(torch.zeros((1, 100)), torch.tensor([100], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        resample.StreamingResampler(2, 44100, 16000, "cpu")
