"""One-token decoding of t-ARK / t-SAIL over per-layer K/V caches (TxfEngine.decode_begin / decode_step / decode_reorder,
csrc/attn_decode.hip): the single-query attention kernel against torch fp64, decode_step against the prefix re-run
(prefix_logits, the reference's own algorithm and the checker), generated tokens with the cache switched on and off, and the
decode state's footprint."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

B_K, H_K = 2, 4
# (dh, n_keys, scale of q): two lanes per key | a lane group's / wave's block edge | a group with idle lanes | the four-wave
# partition edge and the longest BASELINE sequence | one key row per wave instruction | q = 40 randn: scores beyond 130, past the
# range of fp32 exp unless the maximum is subtracted -- the rescale of the merge
KERNEL_CASES = [(8, 1, 1.0), (8, 2, 1.0), (8, 33, 1.0), (32, 63, 1.0), (32, 64, 1.0), (32, 65, 1.0), (96, 100, 1.0),
                (128, 255, 1.0), (128, 256, 1.0), (128, 257, 1.0), (128, 637, 1.0), (256, 5, 1.0), (256, 300, 1.0),
                (128, 637, 40.0), (8, 33, 40.0)]


@pytest.mark.parametrize("dh,n_keys,qscale", KERNEL_CASES)
def test_single_query_attention_matches_torch_fp64(dh, n_keys, qscale):
    """ark_attn_decode_fwd through the C-ABI against fp64 softmax(q K^T / sqrt(dh)) V over cache rows 0 .. n_keys-1.  The cache
    has three more rows, filled with NaN, and `out` starts as NaN: a finite result means rows beyond n_keys are never read and
    every output element is written.  Tolerance: that of the vector-unit attention test (correct fp32 arithmetic differs from
    fp64 by at most 1e-5 on the large-query shapes)."""
    from ark_amd import _lib as L
    torch.manual_seed(1000 * dh + n_keys)
    B, H = B_K, H_K
    D = H * dh
    cap = n_keys + 3
    q = (torch.randn(B, D) * qscale).cuda()
    kv = torch.randn(cap * B, 2 * D)
    kv[n_keys * B:] = float("nan")
    kv = kv.cuda()
    out = torch.full((B, D), float("nan"), device="cuda")
    L.check(L.lib().ark_attn_decode_fwd(L.ptr(q), L.ptr(kv), L.ptr(out), L.i32(B), L.i32(n_keys), L.i32(D), L.i32(H), L.cur_stream()),
            "ark_attn_decode_fwd")
    x = kv.double().view(cap, B, 2, H, dh)[:n_keys]
    k, v = x[:, :, 0], x[:, :, 1]                                        # [n_keys, B, H, dh]
    sc = torch.einsum("bhd,nbhd->bhn", q.double().view(B, H, dh), k) / math.sqrt(dh)
    if qscale > 1:
        assert sc.max().item() > 130
    want = torch.einsum("bhn,nbhd->bhd", torch.softmax(sc, -1), v).reshape(B, D)
    assert torch.isfinite(out).all()
    err = (out.double() - want).abs().max().item()
    print(f"dh={dh} n_keys={n_keys} qscale={qscale}: max abs err {err:.3e}")
    assert torch.allclose(out.double(), want, atol=3e-5, rtol=1e-4), err


def test_single_query_attention_rejects_head_widths_it_does_not_have():
    from ark_amd import _lib as L
    one = torch.zeros(4096, device="cuda")
    f = L.lib().ark_attn_decode_fwd
    for D, H in ((24, 4), (4 * 260, 4), (30, 4)):   # dh = 6 (no multiple of 4), 260 (> 256), D no multiple of the heads
        assert f(L.ptr(one), L.ptr(one), L.ptr(one), L.i32(1), L.i32(1), L.i32(D), L.i32(H), L.cur_stream()) < 0
    assert f(L.ptr(one), L.ptr(one), L.ptr(one), L.i32(1), L.i32(0), L.i32(32), L.i32(4), L.cur_stream()) < 0   # n_keys >= 1


# --------------------------------------------------------------------------------------------------------------------
_SHARED = {}


def _l41(mt):
    """the L = 41 shape of test_prefix_logits_with_flash_attention (t-SAIL: the same with d_latent 16), B = 5: config, oracle
    initialisation, token batch and latents -- built once, never written to"""
    if mt not in _SHARED:
        from oracle import sail_oracle as O
        from tests.test_configs_gpu import _cfg
        from tests.parity_util import synth_batch
        cfg = dict(_cfg(128, 16, 60, 3, 13, True), model_type=mt, dec_dropout=0.0)
        assert cfg["seq_len"] == 41 and cfg["d_latent"] == 16
        P = O.init_params(cfg, 7)
        _, seq = synth_batch(cfg, 5, seed=13, padded=True)
        z = torch.randn(5, cfg["d_latent"], generator=torch.Generator().manual_seed(5))
        _SHARED[mt] = (cfg, P, seq, z)
    return _SHARED[mt]


def _engine(mt, precision, **over):
    from ark_amd.txf_engine import TxfEngine
    cfg, P, seq, z = _l41(mt)
    eng = TxfEngine(dict(cfg, **over), torch.device("cuda:0"), precision=precision)
    eng.load_params(P)
    eng.training = False
    return eng, seq.cuda(), (z.cuda() if mt == "t-SAIL" else None)


@pytest.mark.parametrize("mt", ["t-ARK", "t-SAIL"])
def test_decode_step_matches_the_prefix_rerun_in_exact_fp32(mt):
    """feeding the tokens of a batch one position at a time, the logits of every position t + 1, t = 0 .. 39, agree with
    prefix_logits on the first t + 1 tokens within the project's f32 logits bound"""
    eng, seq, z = _engine(mt, "f32")
    B = seq.shape[0]
    d = eng.decode_begin(B, z)
    worst = 0.0
    for t in range(40):
        got = eng.decode_step(d, seq[:, t].contiguous(), t).clone()
        want = eng.prefix_logits(seq[:, :t + 1].contiguous(), z).clone()
        assert got.shape == want.shape == (B, eng.V)
        worst = max(worst, (got - want).abs().max().item())
        assert torch.allclose(got, want, rtol=3e-4, atol=3e-5), (t, (got - want).abs().max().item())
    print(f"{mt}: max |decode_step - prefix_logits| over 40 positions = {worst:.3e}")


@pytest.mark.parametrize("mt", ["t-ARK", "t-SAIL"])
def test_decode_step_matches_the_prefix_rerun_in_mixed_precision(mt):
    """16-bit products: the prefix path attends in fp16 beyond 16 positions, the cache path in fp32 -- the flash-vs-vector
    bound of test_prefix_logits_with_flash_attention"""
    eng, seq, z = _engine(mt, "mixed")
    d = eng.decode_begin(seq.shape[0], z)
    for t in range(40):
        got = eng.decode_step(d, seq[:, t].contiguous(), t)
        if t in (2, 15, 16, 39):
            got = got.float().clone()
            want = eng.prefix_logits(seq[:, :t + 1].contiguous(), z).float().clone()
            err = (got - want).abs().max().item()
            print(f"{mt} mixed t={t}: max abs diff {err:.3e} (max |logit| {want.abs().max().item():.3f})")
            assert torch.isfinite(got).all()
            assert err < 2e-2 * (want.abs().max().item() + 1.0), (t, err)


# --------------------------------------------------------------------------------------------------------------------
def test_tark_generates_the_same_tokens_with_the_cache_on_and_off():
    from tests.test_txf_gpu import _model
    got = []
    for kv in (1, 0):
        model, z, cfg = _model("tark_small", ark_txf_kv_cache=kv)
        model.eval()
        assert model.engine().kv_cache == bool(kv)
        st = cfg["special_tokens"]
        B = z["gen_greedy"].shape[0]
        greedy = model.generate(cfg["seq_len"], st, batch_size=B).cpu()
        torch.manual_seed(77)
        sampled = model.generate(cfg["seq_len"], st, batch_size=B, sample=True, top_k=3, host_draws=True).cpu()
        got.append((greedy, sampled))
    assert torch.equal(got[0][0], got[1][0])
    assert torch.equal(got[0][1], got[1][1])


@pytest.mark.parametrize("beam", [1, 2, 3])
def test_tsail_decodes_the_same_graphs_with_the_cache_on_and_off(beam):
    from kgvae.model.utils import seq_to_triples
    from tests.test_txf_gpu import _sail_model
    got = []
    for kv in (1, 0):
        model, z, cfg = _sail_model("tsail_small", ark_txf_kv_cache=kv)
        assert model.engine().kv_cache == bool(kv)
        zs = torch.from_numpy(z["dec_z"])
        got.append(model.decode_latent(zs, cfg["seq_len"], cfg["special_tokens"], seq_to_triples, cfg["ENT_BASE"], cfg["REL_BASE"],
                                       beam=beam))
    assert got[0] == got[1]


def test_beam_reorders_the_caches_and_keeps_the_tokens():
    """beam 3 at L = 41: the surviving beams are a non-identity selection at least once, so decode_reorder gathers cache
    blocks; the tokens are those of the prefix re-run"""
    on, _, z = _engine("t-SAIL", "f32")
    off, _, _ = _engine("t-SAIL", "f32", ark_txf_kv_cache=0)
    seen = []
    inner = on.decode_reorder

    def spy(d, j, t):
        seen.append(j.tolist())
        return inner(d, j, t)

    on.decode_reorder = spy
    a = on.beam_decode(z, 3)
    b = off.beam_decode(z, 3)
    assert any(j != [0, 1, 2] and len(set(j)) > 1 for j in seen), seen
    assert torch.equal(a, b)
    assert torch.equal(on.greedy_decode(z), off.greedy_decode(z))


# --------------------------------------------------------------------------------------------------------------------
def test_decode_state_has_no_quadratic_array_and_states_do_not_disturb_each_other():
    eng, seq, z = _engine("t-SAIL", "f32")
    B, H = seq.shape[0], eng.H
    eng.greedy_decode(z)
    assert "_dec_ws_cache" not in eng.__dict__        # the prefix workspace ([B, H, L, L] probabilities per layer) was never built
    sizes = []

    def walk(o):
        if torch.is_tensor(o):
            sizes.append(o.numel())
        elif isinstance(o, dict):
            for v in o.values():
                walk(v)
        elif isinstance(o, (list, tuple)):
            for v in o:
                walk(v)

    walk(eng._kv_cache_ws)
    assert sizes and not [s for s in sizes if s in (B * H * 40 * 40, B * H * 41 * 41)]
    assert all(kv.shape == (eng.seq_len * B, 2 * eng.D) and kv.dtype == torch.float32 for kv in eng._kv_cache_ws[B]["kv"])

    # two batch sizes, three steps each: alone, then interleaved
    ark, seq, _ = _engine("t-ARK", "f32")
    alone = {}
    for Bx in (3, 5):
        d = ark.decode_begin(Bx)
        alone[Bx] = [ark.decode_step(d, seq[:Bx, t].contiguous(), t).clone() for t in range(3)]
    d3 = ark.decode_begin(3)
    d5 = ark.decode_begin(5)
    assert d3 is not d5 and d3["kv"][0].data_ptr() != d5["kv"][0].data_ptr()
    for t in range(3):
        g3 = ark.decode_step(d3, seq[:3, t].contiguous(), t).clone()
        g5 = ark.decode_step(d5, seq[:5, t].contiguous(), t).clone()
        assert torch.equal(g3, alone[3][t]) and torch.equal(g5, alone[5][t]), t
