"""The fp64 statement of the per-latent beam step (tests/beam_ref.py) against a direct restatement with torch, the
input-design condition of the GPU exactness test (tests/test_beam_rows_gpu.py) and the ranking margins of its model-level
fixtures, all without a GPU.

delta = C * 2^-24 * scale with C = 184 from the kernel's own summation structure (ark_amd/csrc/beam.hip's header and the
docstring of tests/test_beam_rows_gpu.py: 92 roundings per candidate score, two candidates per comparison); the limit is
the sampler test's 1024."""
import numpy as np
import pytest
import torch

from oracle import sail_oracle as O
from tests import test_beam_rows_gpu as G
from tests.beam_ref import beam_search, beam_step

MARGIN = 1e-4   # the issue's floor for a model-level fixture


def _direct(l, s, beam, active, eos):
    logp = torch.log_softmax(torch.as_tensor(l, dtype=torch.float64)[:active], dim=-1)
    top_lp, ids = logp.topk(beam, dim=-1)
    cand = (torch.as_tensor(s, dtype=torch.float64)[:active, None] + top_lp).reshape(-1)
    order = torch.sort(cand, descending=True, stable=True).indices[:beam]
    j, k = order // beam, order % beam
    tok = ids[j, k]
    return tok.tolist(), j.tolist(), cand[order].numpy(), bool((tok == eos).all())


@pytest.mark.parametrize("V,beam", [(5, 1), (5, 5), (9, 3), (31, 4), (300, 8), (300, 2)])
def test_helper_is_log_softmax_topk_and_a_stable_sort(V, beam):
    rng = np.random.default_rng(V * 10 + beam)
    for active in sorted({1, beam}):
        for trial in range(20):
            l = (3.0 * rng.standard_normal((beam, V))).astype(np.float32)
            s = (-4.0 * rng.random(beam)).astype(np.float32)
            if trial % 4 == 0:
                l[:, 2] = 30.0         # EOS dominates every beam
            r = beam_step(l, s, beam, active, 2)
            tok, par, sc, done = _direct(l, s, beam, active, 2)
            assert r.tokens.tolist() == tok and r.parents.tolist() == par and r.done == done
            np.testing.assert_allclose(r.scores, sc, rtol=0, atol=1e-12)
            assert r.gap > 0 and r.scale >= 1.0
            if trial % 4 == 0 and active == beam:
                assert r.done


def test_helper_tie_rules_and_gaps():
    l = np.array([[0.0, 1.0, 1.0, -1.0, 1.0], [0.0, 1.0, 1.0, -1.0, 1.0]])
    r = beam_step(l, [0.0, 0.0], 2, 2, 2)
    assert r.top_idx.tolist() == [[1, 2], [1, 2]]            # equal values: lower index first
    assert r.order.tolist() == [0, 1] and r.parents.tolist() == [0, 0] and r.tokens.tolist() == [1, 2]   # equal scores: lower candidate first
    assert r.gap == 0.0
    r = beam_step(l[:1], [0.0], 2, 1, 2)
    assert r.gap == 0.0 and r.tokens.tolist() == [1, 2]
    r = beam_step(np.array([[3.0, 1.0, 0.0]]), [0.0], 2, 1, 2)
    assert abs(r.gap - 1.0) < 1e-12 and abs(r.cand_gap - 2.0) < 1e-12
    r = beam_step(np.array([[3.0, 1.0]]), [0.0], 2, 1, 2)     # V == beam: no logit is cut, one candidate gap
    assert abs(r.gap - 2.0) < 1e-12
    assert beam_step(np.array([[3.0, 1.0]]), [0.0], 1, 1, 0).done and not beam_step(np.array([[3.0, 1.0]]), [0.0], 1, 1, 1).done


def test_gpu_cases_are_mostly_unambiguous():
    """the input-design condition of the GPU exactness test, from the helper alone: in every case (shape x beam x active) at
    least 90 % of the latents have every gap above delta"""
    assert G.C <= 1024
    for V, B in G.SHAPES:
        for beam, active in G.cases(V, B):
            live = [c for c in G.case_steps(V, B, beam, active) if c is not None]
            assert live and all(delta == G.C * 2.0 ** -24 * r.scale for r, delta, _ in live)
            share = np.mean([clear for _, _, clear in live])
            assert share >= 0.9, (V, B, beam, active, share)


def _margin(next_logits, beam, cfg):
    st = cfg["special_tokens"]
    toks, m = beam_search(next_logits, beam, cfg["seq_len"] - 1, st["BOS"], st["EOS"])
    return toks, min(g for g, _, _ in m)


def _sail_next(W, cfg, zi):
    def f(prefixes):
        with torch.no_grad():
            return O.decoder_forward(W, zi.repeat(prefixes.shape[0], 1), torch.from_numpy(prefixes), cfg)[:, -1].numpy()
    return f


@pytest.mark.parametrize("name,beam", G.SAIL_PAIRS)
def test_sail_fixture_margins(name, beam):
    """every step of every latent's own search ranks its candidates (and cuts its logits) with a gap of at least 1e-4, and
    the search built from the helper is O.beam_decode on that latent alone"""
    cfg, W, zs = G.sail_fixture(name)
    worst = np.inf
    for i in range(zs.shape[0]):
        toks, m = _margin(_sail_next(W, cfg, zs[i:i + 1]), beam, cfg)
        assert toks == O.beam_decode(W, zs[i:i + 1], cfg, beam)[0].tolist()
        worst = min(worst, m)
    print(f"{name} beam {beam}: smallest margin {worst:.3e}")
    assert worst >= MARGIN


@pytest.mark.parametrize("name,beam", G.TSAIL_PAIRS)
def test_tsail_fixture_margins(name, beam):
    from tests.parity_util import load_golden
    z, cfg = load_golden(name)
    P = O.init_params(cfg, int(z["seed"]))
    zs = torch.from_numpy(z["dec_z"])
    worst = np.inf
    for i in range(zs.shape[0]):
        zi = zs[i:i + 1]

        def f(prefixes):
            with torch.no_grad():
                return O.tsail_decoder_forward(P, zi.repeat(prefixes.shape[0], 1), torch.from_numpy(prefixes), cfg)[:, -1].numpy()

        worst = min(worst, _margin(f, beam, cfg)[1])
    print(f"{name} beam {beam}: smallest margin {worst:.3e}")
    assert worst >= MARGIN
    assert any(n == "tsail_tiny_pad" for n, _ in G.TSAIL_PAIRS) and len(G.TSAIL_PAIRS) >= 2


@pytest.mark.parametrize("a,b", G.WALKS)
def test_walk_margins_and_flip_counts(a, b):
    from kgvae.experiments import interpolation as I
    cfg, W, zs = G.sail_fixture("sail_small")
    pts = G.walk_points(zs, a, b)
    worst, sets = np.inf, []
    for i in range(pts.shape[0]):
        toks, m = _margin(_sail_next(W, cfg, pts[i:i + 1]), G.WALK_BEAM, cfg)
        worst = min(worst, m)
        sets.append(set(O.seq_to_triples(toks, cfg["ENT_BASE"], cfg["REL_BASE"])))
    print(f"walk dec_z[{a}] -> dec_z[{b}]: smallest margin {worst:.3e}, flips {I.flip_stats(sets)[0]}")
    assert worst >= MARGIN
    assert I.flip_stats(sets)[0] == {(0, 1): 5, (2, 5): 7}[(a, b)]
