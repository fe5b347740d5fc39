"""The fp64 statement of the fused sampler (tests/sample_ref.py) against the oracle's and the model's filters, and the
input-design condition of the GPU exactness test (tests/test_sample_gpu.py), all without a GPU."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import sail_oracle as O
from tests.sample_ref import Row, u_hash

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (temperature, top_p, top_k): the five of test_ark_generate_distribution_and_incremental_step, then the inactive values
FILTERS = [(1.0, 0.0, 0), (0.7, 0.9, 0), (1.3, 0.0, 5), (0.8, 0.5, 7), (1.0, 0.95, 3),
           (1.0, 0.0, "V"), (1.0, 1.0, 0), (0.0, 0.0, 0), (0.0, 0.9, "V"), (1.3, 1.0, 4)]


def _logit_sets():
    """first-step logits of the two models of tests/golden/ark_sampling.npz (fp32, as the engine produces them) and random rows"""
    g = np.load(os.path.join(GOLD, "ark_sampling.npz"), allow_pickle=False)
    sets = []
    for name in ("ark_tiny", "ark_synpaths"):
        cfg = json.loads(str(g[f"{name}/cfg_json"]))
        P = O.init_params(cfg, int(g[f"{name}/seed"]))
        seq = torch.tensor([[1], [1]])
        seq = torch.cat([seq, torch.tensor([[cfg["ENT_BASE"]], [cfg["ENT_BASE"] + 1]])], 1)
        with torch.no_grad():
            lg = O.ark_forward(P, seq, cfg)
        sets.append(lg.reshape(-1, lg.shape[-1]).float())
    torch.manual_seed(1)
    sets.append((torch.randn(7, 31) * 2.5).float())
    sets.append((torch.randn(3, 300) * 3.0).float())
    return sets


LOGITS = _logit_sets()


@pytest.mark.parametrize("temperature,top_p,top_k", FILTERS)
def test_helper_distribution_is_the_oracles_and_the_models(temperature, top_p, top_k):
    from kgvae.model.models import ARK
    for lg in LOGITS:
        V = lg.shape[1]
        k = V if top_k == "V" else top_k
        want = O.sampling_distribution(lg.double(), temperature, top_p, k).numpy()
        model = ARK.filtered_probs(lg, temperature, top_p, k).numpy()
        for r in range(lg.shape[0]):
            R = Row(lg[r].numpy(), temperature, top_p, k)
            got = R.dense()
            np.testing.assert_allclose(got, want[r], rtol=0, atol=1e-12)
            np.testing.assert_allclose(got, model[r], rtol=0, atol=1e-6)
            assert abs(got.sum() - 1.0) < 1e-12


@pytest.mark.parametrize("temperature,top_p,top_k", FILTERS[:5])
def test_midpoint_draws_walk_the_oracles_sorted_filter(temperature, top_p, top_k):
    for lg in LOGITS:
        probs, sp, si = O.next_token_filter(lg.double(), temperature, top_p, top_k)
        if sp is None:
            sp, si = torch.sort(probs, dim=-1, descending=True, stable=True)
        for r in range(lg.shape[0]):
            R = Row(lg[r].numpy(), temperature, top_p, top_k)
            assert R.n_p == int((sp[r] > 0).sum())
            for j in range(R.n_p):
                assert R.token(R.midpoint_u(j)) == int(si[r, j]), (r, j)
            assert R.token(0.0) == int(si[r, 0]) and R.token(1.0 - 2.0 ** -24) in set(si[r, :R.n_p].tolist())


def test_u_hash_is_a_24_bit_counter_hash():
    a = u_hash(0, 0, 64)
    assert a.dtype == np.float32 and (a >= 0).all() and (a < 1).all()
    assert np.array_equal(a * 2.0 ** 24, np.round(a * 2.0 ** 24))
    assert np.array_equal(a, u_hash(0, 0, 64)) and np.array_equal(a[:8], u_hash(0, 0, 8))
    others = [u_hash(1, 0, 64), u_hash(0, 1, 64), u_hash(1 << 32, 0, 64), u_hash(2 ** 63 - 1, 636, 64)]
    assert all(not np.array_equal(a, b) for b in others)
    u = u_hash(7, 3, 1 << 16).astype(np.float64)
    assert abs(u.mean() - 0.5) < 0.01 and abs(np.mean(u < 0.25) - 0.25) < 0.01


def test_gpu_cases_are_mostly_unambiguous():
    """the input-design condition of the GPU exactness test, from the helper alone: in every case (shape x setting) at
    least 80 % of the rows have no cumulative mass within delta of either target"""
    from tests import test_sample_gpu as G
    assert G.C <= 1024
    for V, rows in G.SHAPES:
        for s, per in enumerate(G.case_rows(V, rows)):
            share = np.mean([c[3] for c in per])
            assert share >= 0.8, (V, rows, G.SETTINGS[s], share)
            for R, u, delta, clear in per:
                if clear:   # an unambiguous row admits the helper's token only
                    assert R.admissible(u, delta) == {R.token(u)}
                else:
                    assert R.token(u) in R.admissible(u, delta)
