"""Document-masked causal attention, CPU side: the mask builders, the fp32
reference and the mask threaded through the Llama model (with and without
activation checkpointing)."""

import pytest
import torch

from fms_fsdp_amd import ops
from fms_fsdp_amd.ops import reference

EOS = 0

# eos at position 0 and two eos in a row; eos at the last position; no eos;
# an ordinary row. Four different rows in one batch.
TOKENS = torch.tensor([
    [0, 5, 6, 0, 0, 7, 8, 9],
    [3, 4, 5, 6, 7, 8, 9, 0],
    [3, 4, 5, 6, 7, 8, 9, 1],
    [1, 2, 0, 3, 0, 4, 5, 6],
])
STARTS = torch.tensor([
    [0, 1, 1, 1, 4, 5, 5, 5],
    [0, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 0, 3, 3, 5, 5, 5],
], dtype=torch.int32)
ENDS = torch.tensor([
    [1, 4, 4, 4, 5, 8, 8, 8],
    [8, 8, 8, 8, 8, 8, 8, 8],
    [8, 8, 8, 8, 8, 8, 8, 8],
    [3, 3, 3, 5, 5, 8, 8, 8],
], dtype=torch.int32)


def matrix_from_ends(end):
    s = end.shape[1]
    pos = torch.arange(s)
    return ((pos[None, None, :] <= pos[None, :, None])
            & (pos[None, :, None] < end[:, None, :]))


def test_doc_mask_from_tokens_hand_written_rows():
    m = ops.doc_mask_from_tokens(TOKENS, EOS)
    assert isinstance(m, ops.DocMask)
    assert m.start.dtype == torch.int32 and m.end.dtype == torch.int32
    assert m.start.shape == TOKENS.shape and m.end.shape == TOKENS.shape
    assert torch.equal(m.start, STARTS)
    assert torch.equal(m.end, ENDS)
    pos = torch.arange(TOKENS.shape[1])
    for row in range(TOKENS.shape[0]):
        st, en = m.start[row], m.end[row]
        assert (st >= 0).all() and (st <= pos).all(), row
        assert (en > pos).all() and (en <= TOKENS.shape[1]).all(), row
        assert (st[1:] >= st[:-1]).all(), row
        assert (en[1:] >= en[:-1]).all(), row
    # both arrays describe the same boolean matrix
    assert torch.equal(reference.doc_mask_matrix(m.start),
                       matrix_from_ends(m.end))


def test_doc_mask_from_starts_matches_tokens():
    m = ops.doc_mask_from_starts(STARTS)
    assert torch.equal(m.start, STARTS)
    assert torch.equal(m.end, ENDS)
    # int64 input is accepted and narrowed
    m64 = ops.doc_mask_from_starts(STARTS.long())
    assert m64.start.dtype == torch.int32
    assert torch.equal(m64.end, ENDS)


@pytest.mark.parametrize("h,kvh", [(2, 2), (4, 2)])
def test_reference_equals_per_document_slices(h, kvh):
    torch.manual_seed(11)
    b, s, d = TOKENS.shape[0], TOKENS.shape[1], 16
    q = torch.randn(b, s, h, d)
    k = torch.randn(b, s, kvh, d)
    v = torch.randn(b, s, kvh, d)
    m = ops.doc_mask_from_tokens(TOKENS, EOS)
    o = reference.attention_causal(q, k, v, doc_mask=m)
    assert o.shape == q.shape
    for row in range(b):
        a = 0
        while a < s:
            e = int(m.end[row, a])
            o_doc = reference.attention_causal(
                q[row:row + 1, a:e], k[row:row + 1, a:e], v[row:row + 1, a:e])
            torch.testing.assert_close(o[row:row + 1, a:e], o_doc)
            a = e
    # and the dispatcher takes the reference on CPU
    torch.testing.assert_close(ops.attention_causal(q, k, v, doc_mask=m), o)
    # one document per row is the plain causal mask
    one = ops.doc_mask_from_starts(torch.zeros(b, s, dtype=torch.int32))
    torch.testing.assert_close(
        reference.attention_causal(q, k, v, doc_mask=one),
        reference.attention_causal(q, k, v))


# ---- narrow Llama: two documents in a row of 16, eos closes the first ----
BOUNDARY = 6       # first document = positions 0..5 (eos at 5)


def llama_tokens():
    g = torch.Generator().manual_seed(5)
    t = torch.randint(1, 32, (2, 16), generator=g)
    t[:, BOUNDARY - 1] = EOS
    t2 = t.clone()
    t2[:, :BOUNDARY - 1] = (t[:, :BOUNDARY - 1] % 31) + 1    # all changed
    assert (t2[:, :BOUNDARY - 1] != t[:, :BOUNDARY - 1]).all()
    assert (t2 != EOS).sum() == (t != EOS).sum()
    return t, t2


@pytest.mark.parametrize("ac", [False, True], ids=["plain", "checkpointed"])
def test_llama_second_document_ignores_the_first(narrow_model_factory, ac):
    torch.manual_seed(0)
    model = narrow_model_factory.create()
    for layer in model.layers:
        layer._ac_enabled = ac
    t, t2 = llama_tokens()

    # without the mask the second document's logits depend on the first
    assert model.doc_mask_token is None
    plain, plain2 = model(t), model(t2)
    assert not torch.allclose(plain[:, BOUNDARY:], plain2[:, BOUNDARY:])

    model.doc_mask_token = EOS
    masked, masked2 = model(t), model(t2)
    torch.testing.assert_close(masked[:, BOUNDARY:], masked2[:, BOUNDARY:])
    assert not torch.allclose(masked[:, :BOUNDARY], masked2[:, :BOUNDARY])
    # an explicit mask is the same thing
    model.doc_mask_token = None
    explicit = model(t, doc_mask=ops.doc_mask_from_tokens(t, EOS))
    torch.testing.assert_close(explicit, masked)


@pytest.mark.parametrize("ac", [False, True], ids=["plain", "checkpointed"])
def test_llama_loss_on_second_document_sends_no_gradient_to_the_first(
        narrow_model_factory, ac):
    torch.manual_seed(0)
    model = narrow_model_factory.create()
    for layer in model.layers:
        layer._ac_enabled = ac
    t, _ = llama_tokens()
    labels = torch.roll(t, -1, dims=1)
    labels[:, :BOUNDARY] = -100          # loss on the second document only

    kept = {}

    def keep(_mod, _inp, out):
        out.retain_grad()
        kept["emb"] = out

    handle = model.embedding.register_forward_hook(keep)
    try:
        def emb_grad(token):
            model.doc_mask_token = token
            model.zero_grad()
            loss = model(t, labels=labels)
            assert torch.isfinite(loss)
            loss.backward()
            return kept["emb"].grad

        g = emb_grad(EOS)
        assert torch.count_nonzero(g[:, :BOUNDARY]) == 0
        assert torch.count_nonzero(g[:, BOUNDARY:]) > 0
        assert model.layers[0].attn.qkv.weight.grad.abs().sum() > 0
        # teeth: unmasked, the first document does receive gradient
        assert torch.count_nonzero(emb_grad(None)[:, :BOUNDARY]) > 0
    finally:
        handle.remove()


def test_config_knob_defaults_off():
    from fms_fsdp_amd.config import train_config
    assert train_config().doc_mask is False


@pytest.mark.parametrize("on", [True, False], ids=["doc_mask", "default"])
def test_training_entry_passes_the_eos_token(tmp_path, monkeypatch, on):
    """cfg.doc_mask makes the wrapped model build its mask from the batch
    tokens with cfg.eos_token, every step; off, no mask is ever built."""
    import main_training_llama
    seen = []
    real = ops.doc_mask_from_tokens

    def spy(tokens, eos_token):
        seen.append(eos_token)
        return real(tokens, eos_token)

    monkeypatch.setattr(ops, "doc_mask_from_tokens", spy)
    main_training_llama.main(
        model_variant="llama2_125m", use_dummy_dataset=True, batch_size=1,
        seq_length=128, num_steps=2, report_interval=1,
        checkpoint_interval=100, mixed_precision=False,
        fsdp_activation_checkpointing=True, selective_checkpointing="1/2",
        ckpt_save_path=str(tmp_path), ckpt_load_path=str(tmp_path),
        vocab_size=256, sharding_strategy="fsdp", eos_token=7,
        **({"doc_mask": True} if on else {}))
    assert seen == ([7, 7] if on else [])
