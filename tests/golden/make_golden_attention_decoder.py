"""Writes tests/golden/attention_decoder_keys.json: the state_dict keys and shapes of the REFERENCE's attention decoders, by constructing its
classes (src/decoder.py TransformerDecoder and BiTransformerDecoder; constructing works, only their forward raises).

    python tests/golden/make_golden_attention_decoder.py /path/to/reference/src

The reference is imported, nothing of it is copied; the fixture is a list of names and shapes."""
import json
import os
import sys

CASES = {
    "transformer": dict(cls="TransformerDecoder", args=dict(vocab_size=37, decoder_dim=32, num_heads=4, hidden_dim=64, num_layers=2, dropout=0.1,
                                                             positional_dropout=0.1, self_attention_dropout=0.0, src_attention_dropout=0.0)),
    "bi": dict(cls="BiTransformerDecoder", args=dict(vocab_size=37, decoder_dim=32, num_heads=4, hidden_dim=64, num_layers=2, r_num_layers=1, dropout=0.1,
                                                     pos_enc_dropout=0.1, self_attention_dropout=0.0, src_attention_dropout=0.0)),
}


def main(src):
    sys.path.insert(0, src)
    import decoder                                              # the reference's
    assert os.path.dirname(os.path.abspath(decoder.__file__)) == os.path.abspath(src), decoder.__file__
    out = {}
    for name, case in CASES.items():
        mod = getattr(decoder, case["cls"])(**case["args"])
        out[name] = dict(cls=case["cls"], args=case["args"], state={k: list(v.shape) for k, v in mod.state_dict().items()})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "attention_decoder_keys.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path, {k: len(v["state"]) for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
