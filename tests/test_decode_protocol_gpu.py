"""The decode-state protocol the generation loops run on (decode_begin / decode_step / decode_reorder): decode_reorder on
every kind of state -- the GRU halves, the Transformer's K/V caches, the prefix state of `ark_txf_kv_cache: 0` -- and the
prefix state through ARK.generate against the reference's tokens."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

J = [2, 0, 0]


def _sail_tiny():
    from tests.parity_util import load_golden, make_engine, weights_from
    z, cfg = load_golden("sail_tiny")
    eng = make_engine(cfg, weights_from(z, "w0/"), "f32")
    return eng, torch.randn(2, cfg["d_latent"], generator=torch.Generator().manual_seed(3)).to(eng.device)


def _tsail_l41(**over):
    from tests.test_txf_decode_gpu import _engine
    eng, _, z = _engine("t-SAIL", "f32", **over)
    return eng, z


@pytest.mark.parametrize("make", [_sail_tiny, lambda: _tsail_l41(), lambda: _tsail_l41(ark_txf_kv_cache=0)],
                         ids=["SAIL", "t-SAIL-cache", "t-SAIL-prefix"])
def test_decode_reorder_moves_whole_states_between_blocks(make):
    """3 blocks x B rows with the same latents and three different token columns for steps 0 .. 2; after
    decode_reorder(d, [2, 0, 0], 2) and one more step on a common token, block i gives the logits of block j[i] of the same
    run without the reorder -- exact fp32 on the same row count, so bit for bit"""
    eng, z = make()
    B, V = z.shape[0], eng.V
    g = torch.Generator().manual_seed(11)
    toks = torch.randint(3, V, (3, B, 3), generator=g).to(eng.device)
    assert not torch.equal(toks[0], toks[1]) and not torch.equal(toks[0], toks[2]) and not torch.equal(toks[1], toks[2])
    common = torch.randint(3, V, (B,), generator=g).to(eng.device).repeat(3)
    j = torch.tensor(J, device=eng.device)

    def run(reorder):
        d = eng.decode_begin(3 * B, z.repeat(3, 1), block=B)
        for t in range(3):
            eng.decode_step(d, toks[:, :, t].reshape(-1).contiguous(), t)
        if reorder:
            eng.decode_reorder(d, j, 2)
        return eng.decode_step(d, common, 3).clone().view(3, B, V)

    want = run(False)
    got = run(True)
    assert not torch.equal(want[0], want[2])       # the blocks did diverge: a gather that moved nothing would show
    for i, src in enumerate(J):
        assert torch.equal(got[i], want[src]), (i, src, (got[i] - want[src]).abs().max().item())


def test_tark_generates_the_reference_tokens_on_the_prefix_state():
    """`ark_txf_kv_cache: 0`: ARK.generate runs on the same decode_begin / decode_step calls, over the prefix state, and
    returns the reference's tokens (greedy, and sampling with host draws) as with the cache on"""
    from tests.test_txf_gpu import _model
    model, z, cfg = _model("tark_small", ark_txf_kv_cache=0)
    model.eval()
    assert not model.engine().kv_cache
    st = cfg["special_tokens"]
    B = z["gen_greedy"].shape[0]
    assert np.array_equal(model.generate(cfg["seq_len"], st, batch_size=B).cpu().numpy(), z["gen_greedy"])
    for i, (temp, top_p, top_k) in enumerate(z["gen_combos"]):
        torch.manual_seed(500 + i)
        got = model.generate(cfg["seq_len"], st, batch_size=B, sample=True, temperature=float(temp), top_p=float(top_p),
                             top_k=int(top_k), host_draws=True)
        assert np.array_equal(got.cpu().numpy(), z[f"gen_seq{i}"]), i
