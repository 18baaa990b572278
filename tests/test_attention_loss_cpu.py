"""CPU: the float64 restatement of the label-smoothing loss (tests/attention_loss_ref.py) against the reference's own LabelSmoothingLoss (recorded
in tests/golden/label_smoothing.npz by tests/golden/make_golden_label_smoothing.py), the closed form the kernels evaluate against the definition,
the gradient against torch autograd, and what the public pieces do without a GPU."""
import numpy as np
import pytest
import torch

import attention_loss_ref as R
from conftest import load_golden


@pytest.fixture(scope="module")
def golden():
    arrays, meta = load_golden("label_smoothing")
    z, t = R.golden_case()
    assert np.array_equal(arrays["logits"], z.numpy()) and np.array_equal(arrays["target"], t.numpy()), "golden_case no longer makes the golden's inputs"
    return arrays, meta, z, t


def test_golden_has_ignored_and_edge_targets(golden):
    _, _, z, t = golden
    V = z.shape[2]
    assert V == 37 and int((t < 0).sum()) >= 3 and bool((t == 0).any()) and bool((t == V - 1).any())


def test_restatement_matches_the_reference(golden):
    arrays, meta, z, t = golden
    B, L, V = z.shape
    for c in meta["cases"]:
        got = R.loss(z.view(-1, V), t.view(-1), c["smoothing"], B, c["normalize_length"])
        want = float(arrays["loss_" + c["tag"]])
        assert abs(float(got) - want) <= 1e-12 * max(1.0, abs(want)), (c, float(got), want)


def test_gradient_matches_the_reference(golden):
    arrays, meta, z, t = golden
    B, L, V = z.shape
    for c in meta["cases"]:
        g = torch.full((B * L,), 1.0 / R.denominator(t.view(-1), B, c["normalize_length"]), dtype=torch.float64)
        got = R.grad(z.view(-1, V), t.view(-1), c["smoothing"], g).view(B, L, V)
        want = torch.from_numpy(arrays["grad_" + c["tag"]])
        assert float((got - want).abs().max()) <= 1e-12, c


@pytest.mark.parametrize("s", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("V", [2, 37, 5002])
def test_closed_form_is_the_divergence(s, V):
    g = torch.Generator().manual_seed(V + int(100 * s))
    z = torch.randn(9, V, generator=g, dtype=torch.float64) * 3.0
    t = torch.tensor([0, V - 1, -1, 1, V // 2, -1, 0, V - 1, 1 % V])
    a, b = R.rows_kl(z, t, s), R.rows_closed(z, t, s)
    assert float((a - b).abs().max()) <= 1e-11 * float(a.abs().max()), (s, V)
    assert float(a[t < 0].abs().max()) == 0.0 and float(b[t < 0].abs().max()) == 0.0


def test_gradient_is_autograd_of_the_definition():
    z, t = R.golden_case()
    V = z.shape[2]
    zz = z.view(-1, V).clone().requires_grad_(True)
    gsc = torch.rand(zz.shape[0], generator=torch.Generator().manual_seed(3), dtype=torch.float64) - 0.5
    (R.rows_kl(zz, t.view(-1), 0.1) * gsc).sum().backward()
    assert float((zz.grad - R.grad(z.view(-1, V), t.view(-1), 0.1, gsc)).abs().max()) <= 1e-14


def test_no_valid_target_gives_zero():
    z = torch.randn(4, 5, dtype=torch.float64)
    t = torch.full((4,), -1)
    assert float(R.loss(z, t, 0.1, 2, True)) == 0.0 and float(R.loss(z, t, 0.1, 2, False)) == 0.0
    assert float(R.grad(z, t, 0.1, torch.ones(4)).abs().max()) == 0.0


def test_label_smoothing_loss_module_has_the_references_surface_and_no_cpu_path():
    from label_smoothing_loss import LabelSmoothingLoss
    crit = LabelSmoothingLoss(37, -1, 0.1, normalize_length=True)
    assert (crit.size, crit.padding_idx, crit.smoothing, crit.normalize_length) == (37, -1, 0.1, True) and abs(crit.confidence - 0.9) < 1e-15
    assert not list(crit.parameters())
    z, t = R.golden_case()
    with pytest.raises(RuntimeError, match="no CPU path"):
        crit(z.float(), t)
    with pytest.raises(ValueError):
        LabelSmoothingLoss(37, -1, 1.0)


def test_lsm_ops_are_in_the_prototype_table_and_refuse_cpu_tensors():
    import cfm
    names = {p[0] for p in cfm.PROTOTYPES}
    assert {"cfm_lsm_loss", "cfm_lsm_grad", "cfm_lsm_reduce"} <= names
    z, t = R.golden_case()
    with pytest.raises(RuntimeError, match="no CPU path"):
        cfm.lsm_loss(None, None, None, t.view(-1).int(), 37, 0.1, logits=z.view(-1, 37).float())
    with pytest.raises(RuntimeError, match="no CPU path"):
        cfm.lsm_reduce(torch.zeros(4), torch.zeros(4, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------------- the decoder loss and the public layer
def test_masked_restatement_is_decoder_logits_without_masks():
    """decoder_logits_sites (keep masks, round trips) with nothing switched on is attention_decoder_ref.decoder_logits."""
    dec, memory, enc_lens, labels, lengths = R.decoder_case(5)
    P = {k: v.double() for k, v in dec.left_decoder.state_dict().items()}
    a = R.decoder_loss(P, labels, lengths, memory, enc_lens, 4, 0.1, 36, 36)
    b = R.decoder_loss(P, labels, lengths, memory, enc_lens, 4, 0.1, 36, 36, zmin=[])
    assert abs(float(a) - float(b)) <= 1e-12 * abs(float(a))
    c = R.decoder_loss(P, labels, lengths, memory, enc_lens, 4, 0.1, 36, 36, drops=dict(pos=0.1, self_a=0.1, src_a=0.1, out=0.1, hidden=0.1), seed=5)
    assert abs(float(c) - float(a)) > 1e-3                      # the masks do something


def test_sos_eos_matches_utils_add_sos_eos():
    import utils
    _, _, _, labels, lengths = R.decoder_case(5)
    tin, tg, mask = R.sos_eos(labels, lengths, 36, 36)
    ys_in, ys_out = utils.add_sos_eos(labels, 36, 36, -1)
    assert torch.equal(tin, ys_in) and torch.equal(tg, ys_out)
    assert mask[2].sum() == mask.shape[1] and bool(mask[2, :, 0].all()) and not bool(mask[2, :, 1:].any())     # the empty label row: sos only


def test_decoder_case_keeps_relu_away_from_zero():
    for T in (5, 19):
        assert R.attention_loss_reference(*R.decoder_case(T), 0.3)[2] >= 0.25


def test_attention_loss_refuses_what_it_cannot_do():
    import decoder
    one = decoder.TransformerDecoder(37, 32, 4, 64, 1, 0.0, 0.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="right decoder"):
        decoder.AttentionLoss(one, lsm_weight=0.1, reverse_weight=0.3)
    with pytest.raises(TypeError):
        decoder.AttentionLoss(torch.nn.Linear(2, 2))
    crit = decoder.AttentionLoss(one, lsm_weight=0.1)
    assert (crit.sos, crit.eos, crit.ignore_id) == (36, 36, -1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        crit(torch.zeros(2, 5, 32), torch.ones(2, 1, 5, dtype=torch.bool), torch.tensor([[1, 2], [3, -1]]), torch.tensor([2, 1]))


def test_objective_without_attention_is_unchanged():
    import inspect
    import transducer
    sig = inspect.signature(transducer.TransducerObjective.__init__)
    assert [sig.parameters[k].default for k in ("attention", "attention_weight", "lsm_weight", "reverse_weight")] == [None, 0.0, 0.0, 0.0]
    obj = transducer.TransducerObjective(torch.nn.Identity(), torch.nn.Identity(), torch.nn.Identity(), torch.nn.Identity(), ctc_weight=0.2, transducer_weight=0.8)
    assert obj.attention_loss is None and not [n for n, _ in obj.named_modules() if "attention" in n]
    src = inspect.getsource(transducer.TransducerObjective.forward)
    assert "if self.attention_loss is not None" in src         # the only new branch; the lines before it are the earlier forward
