"""CPU: decoder.JointBeamSearch goes through the one "weights changed -> drop descriptor and graph" path of greedy._Search (as
tests/test_search_invalidation_cpu.py pins for the greedy searches), and BOTH heads take part: the attention decoder's weights and the CTC head's.
Sentinels stand in for the graph: nothing is launched."""
import pytest
import torch


def _search():
    import decoder
    torch.manual_seed(3)
    dec = decoder.TransformerDecoder(9, 16, 2, 32, 1, 0.0, 0.0, 0.0, 0.0).eval()
    ctc = decoder.CTCDecoder(9, 16, 0.0).eval()
    return decoder.JointBeamSearch(dec, ctc, beam=4), dec, ctc


@pytest.mark.parametrize("which", ["ctc", "attention"])
@pytest.mark.parametrize("how", ["new storage", "in place"])
def test_a_weight_change_of_either_head_drops_the_graph(which, how):
    s, dec, ctc = _search()
    s._sync_weights()
    key = s._key_w
    assert key == s._head.weights_key()
    graph = object()
    s._graph = graph
    s._sync_weights()                                                                   # unchanged weights: everything stays
    assert s._graph is graph and s._key_w == key
    p = ctc.ctc_lo.weight if which == "ctc" else dec.output_layer.bias
    if how == "new storage":
        p.data = p.data.clone()                                                         # the same values in new storage
    else:
        with torch.no_grad():
            p.mul_(1.5)                                                                 # the version counter moves
    s._sync_weights()
    assert s._graph is None and s._key_w != key and s._key_w == s._head.weights_key()
    key = s._key_w
    s._graph = graph
    s._sync_weights()
    assert s._graph is graph and s._key_w == key


def test_the_new_state_is_part_of_the_snapshot():
    import decoder
    assert set(decoder.AttentionBeamSearch._SNAP) < set(decoder.JointBeamSearch._SNAP)
    assert {"ctc_state", "ctc_psi"} <= set(decoder.JointBeamSearch._SNAP) and "ctc_x" not in decoder.JointBeamSearch._SNAP      # x is written once, before the loop
