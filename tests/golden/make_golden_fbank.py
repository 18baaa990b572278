#!/usr/bin/env python
"""Generate tests/golden/fbank.npz: the first 32 000 int16 samples (2 s at 16 kHz) of the reference's samples/1.wav, read with the standard
`wave` module.  Data only; the expected features are not stored (tests/fbank_ref.py computes them).

    python tests/golden/make_golden_fbank.py <reference checkout>/samples/1.wav"""
import json
import os
import sys
import wave

import numpy as np

N = 32000
HERE = os.path.dirname(os.path.abspath(__file__))


def main(path):
    with wave.open(path, "rb") as f:
        assert f.getnchannels() == 1 and f.getsampwidth() == 2, "mono 16-bit PCM expected"
        rate = f.getframerate()
        pcm = np.frombuffer(f.readframes(N), dtype="<i2").astype(np.int16)
    assert pcm.size == N, "the clip is shorter than %d samples" % N
    meta = dict(source="reference samples/1.wav, samples [0, %d)" % N, sample_rate=rate, dtype="int16",
                note="waveform * (1 << 15) of a 16-bit file is these values")
    np.savez_compressed(os.path.join(HERE, "fbank.npz"), pcm=pcm, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8))
    print("fbank.npz: %d samples at %d Hz, min %d max %d" % (pcm.size, rate, pcm.min(), pcm.max()))


if __name__ == "__main__":
    main(sys.argv[1])
