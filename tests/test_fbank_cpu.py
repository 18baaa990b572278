"""CPU (no GPU): the log-mel front-end's host side -- the torch restatement of kaldi.fbank the GPU tests measure against (tests/fbank_ref.py),
the packed sparse mel table, the front-end's entry points in the built library and the loud failures.  No compute entry point is called."""
import math

import numpy as np
import pytest
import torch

import fbank_ref as R
from conftest import load_golden


def fixture_pcm(zero_stretch=True):
    g, meta = load_golden("fbank")
    assert meta["sample_rate"] == 16000 and g["pcm"].dtype == np.int16 and g["pcm"].size == 32000
    pcm = g["pcm"].copy()
    if zero_stretch:
        pcm[8000:9000] = 0
    return pcm


def test_restatement_frame_counts():
    assert [R.num_frames(n) for n in (399, 400, 559, 560)] == [0, 1, 1, 2]
    for n, m in ((399, 0), (400, 1), (559, 1), (560, 2)):
        assert tuple(R.fbank(np.zeros(n, np.int16) + 3).shape) == (m, 80)


def test_restatement_reproduces_the_recorded_figures():
    pcm = fixture_pcm()
    f64 = R.fbank(pcm, dtype=torch.float64)
    f32 = R.fbank(pcm, dtype=torch.float32)
    assert tuple(f64.shape) == (198, 80)
    assert abs(float(f64.min()) - (-15.9424)) < 1e-4 and abs(float(f64.min()) - math.log(R.EPS)) < 1e-6
    assert abs(float(f64.max()) - 28.51) < 5e-3
    floored = (f64 - math.log(R.EPS)).abs() < 1e-9
    assert int(floored.sum()) == 320 and int(floored.all(dim=1).sum()) == 4          # four fully floored frames
    smallest = float(f64[~floored].exp().min())
    assert abs(smallest - 21.3) < 0.05                                              # nothing else within 1e6 of the floor
    e = float((f32.double() - f64)[~floored].abs().max())
    print("float32 restatement vs float64 on the fixture: %.3e" % e)
    assert e < 1e-3                                                                 # 4.3e-4 with torch's pocketfft
    assert torch.equal((f32 - math.log(R.EPS)).abs() < 1e-6, floored)


def test_packed_mel_table_equals_the_dense_banks():
    from cfm import packing
    for bins, padded, sf in ((80, 512, 16000.0), (40, 256, 8000.0), (20, 128, 8000.0)):
        w, start, length, offset = packing.pack_mel_banks(bins, padded, sf)
        dense = R.mel_banks(bins, padded, sf, torch.float64).to(torch.float32)
        assert torch.equal(packing.unpack_mel_banks(w, start, length, offset, padded // 2), dense)
        assert w.dtype == torch.float32 and start.dtype == length.dtype == offset.dtype == torch.int32
        assert int(length.sum()) == w.numel() <= 512 and offset.tolist() == [int(length[:b].sum()) for b in range(bins)]
        assert int((start + length).max()) <= padded // 2 and bool((w > 0).all())
        assert int((dense > 0).sum(dim=0).max()) <= 2                                # FFT bins per mel bin, mel bins per FFT bin
        if bins == 80:
            assert int(length.min()) == 1 and int(length.max()) == 16 and int((dense[:, 0] > 0).sum()) == 0


def test_fbank_desc_matches_c():
    import cfm
    lib = cfm.lib()
    assert hasattr(lib, "cfm_fbank") and hasattr(lib, "cfm_fbank_stream") and lib.cfm_version() == 307


def test_no_cpu_path_and_window_limit():
    import fbank
    fb = fbank.KaldiFbank()
    assert (fb.win, fb.shift, fb.padded, fb.num_frames(32000)) == (400, 160, 512, 198)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fb.forward(torch.zeros((2, 800), dtype=torch.int16), torch.tensor([800, 400], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        fbank.StreamingFbank(2, 2, "cpu")
    with pytest.raises(ValueError, match="at most 512"):
        fbank.KaldiFbank(frame_length=64)                                           # 1024 samples at 16 kHz
    assert fbank.KaldiFbank(frame_length=32).padded == 512
