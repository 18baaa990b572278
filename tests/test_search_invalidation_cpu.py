"""CPU: "weights or buffers changed -> drop descriptor and graph" is one code path (greedy._Search._sync_weights / _drop) for the searches that
run without a GPU.  Sentinels stand in for the descriptor and the graph: the torch-operation form (fused=False) builds neither."""
import pytest
import torch

import greedy_ref as R


def _searcher(kind):
    """(search, its prepare step, a call that replaces its hypothesis / state buffers) at E = H = P = J = 16, L = 1, V = 5."""
    import greedy
    pr, jn = R.modules(5, 16, 16, 16, 16, 1, 7)
    if kind == "batched":
        s = greedy.BatchedGreedySearch(pr, jn, fused=False)
        enc = torch.zeros((2, 3, 16))
        return s, jn, lambda: s._prepare(enc, [3, 2], None, None), lambda: s._prepare(torch.zeros((2, 4, 16)), [4, 2], None, None)
    s = greedy.ChunkGreedySearch(pr, jn, 2, 2, fused=False)
    return s, jn, s._prepare, lambda: s._grow(s.S["hyps"].shape[1] + 1)


@pytest.mark.parametrize("kind", ["batched", "chunk"])
def test_new_weights_and_new_buffers_drop_descriptor_and_graph(kind):
    s, jn, prepare, new_buffers = _searcher(kind)
    prepare()
    key = s._key_w
    assert key == s._head.weights_key()
    graph, desc = object(), object()
    s._graph, s._desc = graph, desc
    prepare()                                                                           # unchanged weights, same buffers: everything stays
    assert s._graph is graph and s._desc is desc and s._key_w == key
    p = jn.ffn_out.bias
    p.data = p.data.clone()                                                             # the same values in new storage
    prepare()
    assert s._graph is None and s._desc is None and s._key_w != key and s._key_w == s._head.weights_key()
    key = s._key_w
    s._graph, s._desc = graph, desc
    prepare()
    assert s._graph is graph and s._desc is desc and s._key_w == key
    new_buffers()                                                                       # ... and replaced buffers go the same way; the weights key stays
    assert s._graph is None and s._desc is None and s._key_w == key
