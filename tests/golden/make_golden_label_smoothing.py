"""Writes tests/golden/label_smoothing.npz: the REFERENCE's LabelSmoothingLoss (src/label_smoothing_loss.py) run in float64 on the seeded logits
and targets of tests/attention_loss_ref.golden_case, smoothing {0, 0.1} x both normalisations, and its gradient by torch autograd.

    python tests/golden/make_golden_label_smoothing.py /path/to/reference/src

The reference is imported and run, nothing of it is copied; the fixture holds inputs and recorded results."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def main(src):
    sys.path.insert(0, src)
    sys.path.insert(0, os.path.dirname(HERE))
    import label_smoothing_loss                                 # the reference's
    assert os.path.dirname(os.path.abspath(label_smoothing_loss.__file__)) == os.path.abspath(src), label_smoothing_loss.__file__
    import attention_loss_ref as R
    z, t = R.golden_case()
    out = dict(logits=z.numpy(), target=t.numpy())
    cases = []
    for s in (0.0, 0.1):
        for nl in (False, True):
            zz = z.clone().requires_grad_(True)
            loss = label_smoothing_loss.LabelSmoothingLoss(z.shape[2], -1, s, nl)(zz, t)
            loss.backward()
            tag = "s%g_nl%d" % (s, nl)
            out["loss_" + tag], out["grad_" + tag] = loss.detach().numpy(), zz.grad.numpy()
            cases.append(dict(tag=tag, smoothing=s, normalize_length=nl))
    out["meta"] = np.frombuffer(json.dumps(dict(cases=cases, padding_idx=-1)).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "label_smoothing.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {c["tag"]: float(out["loss_" + c["tag"]]) for c in cases})


if __name__ == "__main__":
    main(sys.argv[1])
