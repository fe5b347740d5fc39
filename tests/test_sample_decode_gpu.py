"""Engine.sample_decode -- the sampled / greedy / forced-token generation loop over decode_begin / decode_step with the fused
sampler (csrc/sample.hip) -- and what is built on it: ARK.generate(sampler="fused"), SAIL.sample_latent,
kgvae.experiments.conditioned and the `ark_sampler` key of kgvae.experiments.train.  Tiny and small goldens only."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from tests.parity_util import load_golden
from tests.sample_ref import Row, u_hash
from tests.test_sample_gpu import C, EPS24, t32

pytestmark = pytest.mark.gpu

ALL_FOUR = ["sail_tiny", "tsail_tiny", "ark_tiny", "tark_tiny"]


def _model(name):
    from kgvae.model.models import ARK, SAIL
    z, cfg = load_golden(name)
    cfg = dict(cfg, precision="f32")
    torch.manual_seed(int(z["seed"]))
    model = (SAIL if cfg["model_type"] in ("SAIL", "t-SAIL") else ARK)(cfg).to("cuda")
    model.eval()
    return model, cfg


def _latents(cfg, B, seed=3):
    if cfg["model_type"] not in ("SAIL", "t-SAIL"):
        return None
    return torch.randn(B, cfg["d_latent"], generator=torch.Generator().manual_seed(seed)).cuda()


def _greedy_hand_loop(eng, B, z, seq_len, bos, forced):
    """the reference's greedy semantics on the bare protocol: argmax of every step's logits, forced columns overwritten"""
    d = eng.decode_begin(B, z)
    cols = [torch.full((B,), bos, dtype=torch.int64, device="cuda")]
    for t in range(seq_len - 1):
        logits = eng.decode_step(d, cols[-1].contiguous(), t)
        nxt = logits.argmax(dim=-1)
        if t + 1 in forced:
            nxt = torch.full_like(nxt, forced[t + 1])
        cols.append(nxt)
    return torch.stack(cols, 1).cpu()


def _same_up_to_the_stop(got, full, eos):
    """`got` [B, <= L] is `full` [B, L] cut at the first column where every row is EOS"""
    n = got.shape[1]
    if not torch.equal(got.cpu(), full[:, :n]):
        return False
    done = (full[:, 1:] == eos).all(dim=0)
    first = int(torch.nonzero(done)[0]) + 1 if bool(done.any()) else full.shape[1] - 1
    return n == first + 1


@pytest.mark.parametrize("name", ["ark_tiny", "tsail_tiny"])
def test_stopping_rule_does_not_depend_on_check_every(name):
    model, cfg = _model(name)
    eng, eos = model.engine(), cfg["special_tokens"]["EOS"]
    B, Lmax = 5, cfg["seq_len"] - 1
    z = _latents(cfg, B)
    for forced, width in [(None, Lmax + 1), ({4: eos}, 5), ({1: eos}, 2), ({Lmax: eos}, Lmax + 1)]:
        kw = dict(sample=True, temperature=0.9, top_p=0.95, seed=11, forced=forced, eos=eos)
        outs = [eng.sample_decode(B, z, check_every=ce, **kw).cpu() for ce in (1, 16, Lmax, 3)]
        assert all(torch.equal(outs[0], o) for o in outs[1:]), forced
        if forced is None and not bool((outs[0][:, 1:] == eos).all(dim=0).any()):
            assert outs[0].shape[1] == width
        if forced is not None and min(forced) < Lmax:
            assert outs[0].shape[1] == width and bool((outs[0][:, -1] == eos).all())


def test_seeds():
    model, cfg = _model("ark_tiny")
    st, L = cfg["special_tokens"], cfg["seq_len"]
    gen = lambda **kw: model.generate(L, st, batch_size=16, sample=True, top_p=0.9, sampler="fused", **kw).cpu()
    a = gen(seed=5)
    assert a.shape == (16, L) and bool((a[:, 0] == st["BOS"]).all())
    assert torch.equal(a, gen(seed=5)) and not torch.equal(a, gen(seed=6))
    assert not torch.equal(a[0], a[1]) or not torch.equal(a[0], a[2])      # rows draw their own u
    torch.manual_seed(77)
    b1, b2 = gen(), gen()
    torch.manual_seed(77)
    assert torch.equal(b1, gen()) and torch.equal(b2, gen()) and not torch.equal(b1, b2)
    with pytest.raises(ValueError):
        model.generate(L, st, batch_size=2, sample=True, sampler="fused", host_draws=True)
    with pytest.raises(ValueError):
        model.generate(L, st, batch_size=2, sample=True, seed=1)           # the torch sampler has no seed argument


@pytest.mark.parametrize("name", ["ark_tiny", "tark_tiny"])
@pytest.mark.parametrize("T,top_p,top_k", [(0.7, 0.9, 0), (1.3, 0.0, 5), (1.0, 0.0, 0)])
def test_every_token_is_the_helpers_token_for_that_steps_logits(name, T, top_p, top_k):
    """a second decode_begin pass fed the generated tokens recomputes every step's logits; the token at column t + 1 is the
    fp64 statement's for those logits and the counter hash's u of (seed, column, row), or admissible on an ambiguous row"""
    model, cfg = _model(name)
    eng, B, seed = model.engine(), 8, 2 ** 40 + 17
    toks = eng.sample_decode(B, None, sample=True, temperature=T, top_p=top_p, top_k=top_k, seed=seed,
                             eos=cfg["special_tokens"]["EOS"])
    d = eng.decode_begin(B)
    host = toks.cpu().numpy()
    clear_rows = 0
    for t in range(toks.shape[1] - 1):
        logits = eng.decode_step(d, toks[:, t].contiguous(), t).cpu().numpy()
        u = u_hash(seed, t + 1, B)
        for r in range(B):
            R = Row(logits[r], t32(T), top_p, top_k)
            delta = C * EPS24 * R.Z
            if R.unambiguous(u[r], delta):
                clear_rows += 1
                assert host[r, t + 1] == R.token(u[r]), (t, r)
            else:
                assert int(host[r, t + 1]) in R.admissible(u[r], delta), (t, r)
    assert clear_rows >= 0.8 * B * (toks.shape[1] - 1)


@pytest.mark.parametrize("T,top_p,top_k", [(0.7, 0.9, 0), (1.3, 0.0, 5)])
def test_empirical_distribution_of_one_position(T, top_p, top_k):
    """4096 rows, one position (every row sees the logits after BOS): each token's frequency within
    5 * sqrt(p (1 - p) / 4096) of ARK.filtered_probs -- tokens outside the kept set are never drawn"""
    from kgvae.model.models import ARK
    model, cfg = _model("ark_tiny")
    eng, n = model.engine(), 4096
    toks = eng.sample_decode(n, None, max_len=1, sample=True, temperature=T, top_p=top_p, top_k=top_k, seed=123,
                             eos=cfg["special_tokens"]["EOS"]).cpu().numpy()
    d = eng.decode_begin(2)
    logits = eng.decode_step(d, torch.full((2,), cfg["special_tokens"]["BOS"], dtype=torch.int64, device="cuda"), 0)
    p = ARK.filtered_probs(logits[:1].clone(), T, top_p, top_k)[0].double().cpu().numpy()
    freq = np.bincount(toks[:, 1], minlength=p.shape[0]) / n
    assert np.all(np.abs(freq - p) <= 5.0 * np.sqrt(p * (1.0 - p) / n)), np.abs(freq - p).max()
    assert (freq > 0).sum() >= 2


@pytest.mark.parametrize("name", ALL_FOUR)
def test_forced_tokens_in_all_four_models(name):
    model, cfg = _model(name)
    eng, st, L, B = model.engine(), cfg["special_tokens"], cfg["seq_len"], 4
    z = _latents(cfg, B)
    forced = {2: cfg["REL_BASE"], 3: cfg["ENT_BASE"] + 1}
    want = _greedy_hand_loop(eng, B, z, L, st["BOS"], forced)
    got = eng.sample_decode(B, z, sample=False, forced=forced, bos=st["BOS"], eos=st["EOS"])
    assert bool((got[:, 2] == forced[2]).all()) and bool((got[:, 3] == forced[3]).all())
    assert _same_up_to_the_stop(got, want, st["EOS"])
    free = _greedy_hand_loop(eng, B, z, L, st["BOS"], {})
    assert _same_up_to_the_stop(eng.sample_decode(B, z, sample=False, bos=st["BOS"], eos=st["EOS"]), free, st["EOS"])
    # sampled with forced columns: the forced columns hold, the draws stay reproducible
    a = eng.sample_decode(B, z, sample=True, top_p=0.9, seed=3, forced=forced, bos=st["BOS"], eos=st["EOS"])
    assert bool((a[:, 2] == forced[2]).all()) and bool((a[:, 3] == forced[3]).all())
    assert torch.equal(a, eng.sample_decode(B, z, sample=True, top_p=0.9, seed=3, forced=forced, bos=st["BOS"], eos=st["EOS"]))


@pytest.mark.parametrize("name", ["sail_tiny", "ark_tiny"])
def test_conditional_generate_equals_the_hand_loop(name):
    from kgvae.experiments import conditioned as CG
    model, cfg = _model(name)
    cfg2, resolved = CG.normalize_config(cfg)
    kind = "sail" if resolved in ("SAIL", "t-SAIL") else "ark"
    assert resolved == cfg["model_type"] and cfg2 is not cfg
    st, L, n = cfg["special_tokens"], cfg["seq_len"], 4
    vocabs = {"e2i": {f"e{i}": i for i in range(cfg["n_entities"])}, "r2i": {f"r{i}": i for i in range(cfg["n_relations"])}}
    vocabs.update(i2e={i: k for k, i in vocabs["e2i"].items()}, i2r={i: k for k, i in vocabs["r2i"].items()})
    rid, oid = CG.ids_for_condition(vocabs, cfg, "r1", "e2")
    assert (rid, oid) == (cfg["REL_BASE"] + 1, cfg["ENT_BASE"] + 2)
    torch.manual_seed(5)
    seqs = CG.conditional_generate(model, kind, cfg, rid, oid, n, "cuda")
    torch.manual_seed(5)
    z = torch.randn(n, cfg["d_latent"], device="cuda") if kind == "sail" else None
    want = _greedy_hand_loop(model.engine(), n, z, L, st["BOS"], {2: rid, 3: oid})
    assert seqs.shape == (n, L) and seqs.device.type == "cpu"
    done = (want[:, 1:] == st["EOS"]).all(dim=0)
    stop = int(torch.nonzero(done)[0]) + 1 if bool(done.any()) else L - 1
    assert torch.equal(seqs[:, :stop + 1], want[:, :stop + 1]) and bool((seqs[:, stop + 1:] == st["EOS"]).all())
    graphs = CG.to_labeled_triples(seqs, cfg, vocabs)
    assert bool((seqs[:, 2] == rid).all()) and bool((seqs[:, 3] == oid).all())
    assert len(graphs) == n and all(len(t) == 3 for g in graphs for t in g)
    with pytest.raises(KeyError):
        CG.ids_for_condition(vocabs, cfg, "no such relation", "e2")


@pytest.mark.parametrize("name", ["ark_tiny", "tark_tiny"])
def test_fused_greedy_generate_equals_the_default(name):
    model, cfg = _model(name)
    st, L = cfg["special_tokens"], cfg["seq_len"]
    assert torch.equal(model.generate(L, st, batch_size=3, sampler="fused"), model.generate(L, st, batch_size=3))


def test_train_entry_point_with_the_fused_sampler(tmp_path, monkeypatch):
    """kgvae.experiments.train on the synthetic data of test_train_entry_point_end_to_end with `ark_sampler: fused`: the
    verification's generations run on Engine.sample_decode and the run completes"""
    from ark_amd.engine import Engine
    from kgvae.experiments import train as T
    calls = []
    real = Engine.sample_decode
    monkeypatch.setattr(Engine, "sample_decode", lambda self, *a, **k: (calls.append(a[0]), real(self, *a, **k))[1])
    # the verification needs the optional intelligraphs package: stand-ins for its two entry points, so that the generation
    # in front of them runs whether or not it is installed
    graded = []
    monkeypatch.setattr(T, "get_verifier", lambda name: object())
    monkeypatch.setattr(T, "run_semantic_evaluation", lambda labels, *a, **k: (
        graded.append(len(labels)), type("Ev", (), {"organized_results": {"results": {"semantics": 50.0}}})())[1])
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "configs", "sail_syn-paths.yaml")))
    cfg.update(model_type="ARK", d_model=64, num_epochs=1, batch_size=64, save_every=1, compression_log_every=1, verify_every=1,
               num_generated_latent_graphs=100, learning_rate=1e-3, ark_sampler="fused",
               synthetic_sizes={"n_train": 256, "n_val": 64, "n_test": 64})
    cpath = tmp_path / "c.yaml"
    yaml.safe_dump(cfg, open(cpath, "w"))
    T.main(["--config", str(cpath), "--checkpoint-dir", str(tmp_path / "ck")])
    assert calls == [50, 50] and graded == [100]
    run = os.listdir(tmp_path / "ck")[0]
    rows = [json.loads(l) for l in open(tmp_path / "ck" / run / "metrics.jsonl")]
    assert any("verification/validity_rate" in r for r in rows)
