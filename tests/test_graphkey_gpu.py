"""Graph keys on the device: ark_graph_canon and ark_graph_pair_stats (ark_amd/csrc/graphkey.hip) against the plain restatement
of tests/graphkey_ref.py (itself pinned to canonical_graph_string by tests/test_graphkey_cpu.py), bit for bit, on both sides of
the wave / workgroup path switch; the key sets of ark_amd.graphs against Python sets of strings; and what is built on them:
graph_stats of all model kinds, SAIL.reconstruction_rate, the two interpolation statistics and the training loop's
`device_graph_stats` key.  Every comparison is one of exact integers."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from tests import graphkey_ref as R

pytestmark = pytest.mark.gpu

EOS = 2
ALPHABET = [EOS, 3, 4, 5, 1000, 1001]          # few tokens: duplicates, early stops and all-equal lists in every batch
ROW_LENS = [1, 3, 4, 11, 190, 193, 194, 197, 638, 3074]      # cap 0, 0, 1, 3, 63, 64, 64, 65, 212, 1024
_REF = {}


def _rows(row_len, B, with_lens, wide=False):
    """(toks [B, row_len] numpy, lens or None, the restatement's outputs); computed once per case and shared"""
    k = (row_len, B, with_lens, wide)
    if k not in _REF:
        rng = np.random.default_rng(1000 * row_len + 10 * B + with_lens)
        if wide:
            top = (1 << 21) - 1
            toks = rng.choice([EOS, top, top - 1, top - 2, top - 3, 7], size=(B, row_len), p=[.02, .3, .2, .2, .2, .08])
        else:
            toks = rng.choice(ALPHABET, size=(B, row_len), p=[.01 if row_len > 100 else .06] + [(.99 if row_len > 100 else .94) / 5] * 5)
        toks = toks.astype(np.int64)
        if B > 1:
            toks[1] = toks[1, min(1, row_len - 1)]                  # an all-equal row
        lens = None
        if with_lens:
            lens = rng.integers(0, row_len + 3, size=B).astype(np.int64)       # (values past row_len: the whole row)
            special = [0, 1, 5, 6, row_len, 3 * (row_len // 6) + 3]               # empty, BOS only, cuts inside a slot
            for i in range(B):
                if i < len(special) or B == 1:
                    lens[i] = special[(i + row_len) % len(special)]
        _REF[k] = (toks, lens, R.canon_ref(toks, lens, EOS))
    return _REF[k]


def _device_rows(toks, pad=5):
    """the rows as a [B, row_len] view of a wider buffer (ld > row_len) whose padding columns hold tokens that must not be read"""
    B, row_len = toks.shape
    buf = torch.full((B, row_len + pad), 4, dtype=torch.int64, device="cuda")
    buf[:, :row_len] = torch.from_numpy(toks).cuda()
    return buf[:, :row_len]


def _check_batch(batch, ref):
    canon, n, nset, key, _ = ref
    assert batch.canon.dtype == torch.int64 and batch.key.dtype == torch.int64
    assert batch.n.dtype == torch.int32 and batch.nset.dtype == torch.int32
    assert np.array_equal(batch.n.cpu().numpy(), n)
    assert np.array_equal(batch.nset.cpu().numpy(), nset)
    assert np.array_equal(batch.canon.cpu().numpy(), canon)
    assert np.array_equal(batch.key.cpu().numpy(), key)


@pytest.mark.parametrize("with_lens", [False, True])
@pytest.mark.parametrize("B", [1, 5, 64])
@pytest.mark.parametrize("row_len", ROW_LENS)
def test_canon_equals_the_restatement(row_len, B, with_lens):
    from ark_amd import graphs as G
    toks, lens, ref = _rows(row_len, B, with_lens)
    assert ref[0].shape[1] == G.row_cap(row_len)
    view = _device_rows(toks)
    assert view.stride(0) > row_len
    batch = G.canon(view, None if lens is None else torch.from_numpy(lens).cuda(), eos=EOS)
    _check_batch(batch, ref)


@pytest.mark.parametrize("row_len", [11, 193, 197])
def test_canon_full_width_tokens(row_len):
    from ark_amd import graphs as G
    toks, lens, ref = _rows(row_len, 5, False, wide=True)
    assert int(ref[0].max()) > (1 << 62)            # the packed word is used to its last bits
    _check_batch(G.canon(_device_rows(toks), None, eos=EOS, vocab=1 << 21), ref)


def test_canon_refuses_more_than_1024_triples_and_writes_nothing():
    from ark_amd import graphs as G
    from ark_amd._lib import ArkError
    B, row_len = 2, 3077
    toks = torch.full((B, row_len), 5, dtype=torch.int64, device="cuda")
    outs = (torch.full((B, 1025), 77, dtype=torch.int64, device="cuda"), torch.full((B,), 77, dtype=torch.int32, device="cuda"),
            torch.full((B,), 77, dtype=torch.int32, device="cuda"), torch.full((B, 2), 77, dtype=torch.int64, device="cuda"))
    assert G.canon_raw(toks, None, EOS, *outs) == -2          # ARK_ERR_SHAPE
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == 77).all())
    with pytest.raises(ArkError):
        G.canon(toks)


@pytest.mark.parametrize("with_lens", [False, True])
@pytest.mark.parametrize("row_len,B", [(1, 5), (4, 5), (11, 64), (193, 64), (197, 5), (638, 64), (3074, 5)])
def test_pair_stats_equal_python_sets(row_len, B, with_lens):
    from ark_amd import graphs as G
    toks, lens, ref = _rows(row_len, B, with_lens)
    batch = G.canon(_device_rows(toks), None if lens is None else torch.from_numpy(lens).cuda(), eos=EOS)
    rng = np.random.default_rng(row_len)
    P = 41
    ia, ib = rng.integers(0, B, size=P), rng.integers(0, B, size=P)
    ia[:5] = ib[:5]                                                # a graph against itself
    empty = np.flatnonzero(ref[1] == 0)
    if len(empty):                                                 # one side empty, both sides empty
        ia[5:8] = empty[0]
        ib[8:10] = empty[-1]
        ia[10] = ib[10] = empty[0]
    inter, da, db = (x.cpu().numpy() for x in G.pair_stats(batch, ia, ib))
    w_inter, w_da, w_db = R.pair_ref(toks, lens, ia, ib, EOS)
    assert np.array_equal(inter, w_inter) and np.array_equal(da, w_da) and np.array_equal(db, w_db)
    assert inter.dtype == np.int32
    assert np.array_equal(da, ref[2][ia])                          # nset is the same count


def test_pair_stats_refuses_rows_that_are_not_there():
    from ark_amd import graphs as G
    from ark_amd._lib import ArkError
    toks, _, _ = _rows(11, 5, False)
    batch = G.canon(_device_rows(toks))
    for ia, ib in (([5], [0]), ([0], [-1])):
        with pytest.raises(ArkError):
            G.pair_stats(batch, ia, ib)


def _graph_rows(graphs, W):
    rows = []
    for g in graphs:
        row = [1] + [t for tr in g for t in tr] + [EOS]
        rows.append(row + [0] * (W - len(row)))
    return np.array(rows, dtype=np.int64)


@pytest.mark.parametrize("T", [5, 80])                              # the wave path and the workgroup path
def test_unique_and_novel_equal_python_sets_of_strings(T):
    from ark_amd import graphs as G
    import random
    rng = random.Random(T)
    W = 2 + 3 * T
    pool = [[(rng.randrange(3, 9), 1000 + rng.randrange(3), rng.randrange(3, 9)) for _ in range(rng.randrange(0, T + 1))]
            for _ in range(40)]
    gen = [rng.sample(g, len(g)) for g in (rng.choice(pool[:30]) for _ in range(200))]      # planted duplicates, shuffled
    train = [rng.sample(g, len(g)) for g in pool[20:]]                                         # shares pool[20:30] with them
    gen_rows, train_rows = _graph_rows(gen, W), _graph_rows(train, W)
    gen_s = R.canon_ref(gen_rows, None, EOS)[4]
    train_s = set(R.canon_ref(train_rows, None, EOS)[4])
    batch = G.canon(torch.from_numpy(gen_rows).cuda())
    train_keys = G.canon(torch.from_numpy(train_rows).cuda()).key
    assert len(set(gen_s)) < len(gen_s)
    assert G.unique_count(batch) == len(set(gen_s))
    first = [s not in gen_s[:i] for i, s in enumerate(gen_s)]
    assert G.unique_mask(batch).cpu().tolist() == first
    novel = [s not in train_s for s in gen_s]
    assert 0 < sum(novel) < len(novel)
    assert G.novel_mask(batch, train_keys).cpu().tolist() == novel
    out = G.summary(batch, train_keys)
    assert out == {"n": 200, "unique": len(set(gen_s)), "unique_rate": len(set(gen_s)) / 200, "novel": sum(novel),
                   "novel_rate": sum(novel) / 200, "empty": sum(len(g) == 0 for g in gen),
                   "mean_triples": sum(len(g) for g in gen) / 200}
    assert set(G.summary(batch)) == {"n", "unique", "unique_rate", "empty", "mean_triples"}


# ---------------------------------------------------------------------------------------------------------------- models
def _host_stats(toks, lens, cfg, train_strings=None):
    """the numbers of graph_stats from the same tokens, the host way: seq_to_triples per row, strings, sets"""
    from kgvae.model.utils import canonical_graph_string, seq_to_triples
    toks = toks.cpu()
    lens = [toks.shape[1]] * toks.shape[0] if lens is None else lens.cpu().tolist()
    graphs = [seq_to_triples(row[:n], cfg["special_tokens"], cfg["ENT_BASE"], cfg["REL_BASE"]) for row, n in zip(toks, lens)]
    strings = [canonical_graph_string(g) for g in graphs]
    N = len(graphs)
    out = {"n": N, "unique": len(set(strings)), "unique_rate": len(set(strings)) / N}
    if train_strings is not None:
        out["novel"] = sum(s not in train_strings for s in strings)
        out["novel_rate"] = out["novel"] / N
    out["empty"] = sum(len(g) == 0 for g in graphs)
    out["mean_triples"] = sum(len(g) for g in graphs) / N
    return out, strings


def _model(name):
    from tests.test_sample_decode_gpu import _model as build
    return build(name)


@pytest.mark.parametrize("name,beam,per_latent", [("sail_tiny", 1, False), ("sail_tiny", 3, True), ("sail_small", 2, False),
                                                  ("tsail_tiny", 2, True)])
def test_sail_graph_stats_equal_the_host_recomputation(name, beam, per_latent):
    from ark_amd import graphs as G
    model, cfg = _model(name)
    st = cfg["special_tokens"]
    z = torch.randn(48, cfg["d_latent"], generator=torch.Generator().manual_seed(4)).cuda()
    z[7] = z[3]                                                      # two latents, one graph
    toks, lens = model.decode_latent_tokens(z, cfg["seq_len"], st, beam=beam, per_latent=per_latent)
    assert toks.is_cuda and (lens is None) == (not per_latent)
    want, strings = _host_stats(toks, lens, cfg)
    got = model.graph_stats(48, cfg["seq_len"], st, beam=beam, per_latent=per_latent, z=z)
    assert got == {k: want[k] for k in ("n", "unique", "unique_rate", "empty", "mean_triples")}
    assert got["unique"] < 48
    # novelty against a "training split" that holds every second generated graph
    train_strings = set(strings[::2])
    train_keys = G.canon(toks[::2].contiguous(), None if lens is None else lens[::2], eos=st["EOS"]).key
    want, _ = _host_stats(toks, lens, cfg, train_strings)
    assert model.graph_stats(48, cfg["seq_len"], st, beam=beam, per_latent=per_latent, z=z, train_keys=train_keys) == want
    # the same tokens as the parsed-list interface decodes
    from kgvae.model.utils import canonical_graph_string, seq_to_triples
    lists = model.decode_latent(z, cfg["seq_len"], st, seq_to_triples, cfg["ENT_BASE"], cfg["REL_BASE"], beam=beam, per_latent=per_latent)
    assert [canonical_graph_string(g) for g in lists] == strings
    # without z: num_samples fresh latents
    assert model.graph_stats(5, cfg["seq_len"], st, beam=1)["n"] == 5


@pytest.mark.parametrize("name", ["ark_tiny", "tark_tiny"])
def test_ark_graph_stats_equal_the_host_recomputation(name):
    model, cfg = _model(name)
    st = cfg["special_tokens"]
    kw = dict(sample=True, temperature=1.3, top_k=5, sampler="fused", seed=11)
    toks = model.generate(cfg["seq_len"], st, batch_size=40, **kw)
    want, strings = _host_stats(toks, None, cfg, set())
    from ark_amd import graphs as G
    none = torch.empty(0, 2, dtype=torch.int64, device="cuda")
    assert model.graph_stats(40, cfg["seq_len"], st, train_keys=none, **kw) == want
    train_keys = G.canon(toks[:10].contiguous(), eos=st["EOS"]).key
    want, _ = _host_stats(toks, None, cfg, set(strings[:10]))
    got = model.graph_stats(40, cfg["seq_len"], st, train_keys=train_keys, **kw)
    assert got == want and got["novel"] <= 30
    two = model.graph_stats(40, cfg["seq_len"], st, batch_size=20, **kw)          # batches of 20: seeds 11 and 12
    rows = torch.cat([model.generate(cfg["seq_len"], st, batch_size=20, **dict(kw, seed=11 + i)) for i in range(2)])
    assert two == {k: v for k, v in _host_stats(rows, None, cfg)[0].items()}


def _trained(name):
    """a GRU SAIL golden with its trained weights"""
    from tests.test_beam_rows_gpu import _sail
    model, cfg, _ = _sail(name)
    return model, cfg


@pytest.mark.parametrize("name,beam", [("sail_small", 1), ("sail_small_pad", 3), ("tsail_tiny_pad", 1)])
def test_reconstruction_rate_equals_its_host_restatement(name, beam):
    from kgvae.model.utils import canonical_graph_string, seq_to_triples
    from tests.parity_util import load_golden
    model, cfg = _trained(name) if name.startswith("sail") else _model(name)
    z, _ = load_golden(name)
    st = cfg["special_tokens"]
    triples = torch.from_numpy(z["triples"]).cuda()
    eps = torch.randn(triples.shape[0], cfg["d_latent"], generator=torch.Generator().manual_seed(2)).cuda()
    zz, _, _ = model.encode(triples, eps)
    decoded = model.beam_generate(cfg["seq_len"], st, seq_to_triples, zz, cfg["ENT_BASE"], cfg["REL_BASE"], beam=beam)
    pad = cfg.get("pad_eid")
    inputs = [[tuple(t) for t in g if pad is None or t[0] != pad] for g in triples.cpu().tolist()]
    same = [canonical_graph_string(a) == canonical_graph_string(b) for a, b in zip(decoded, inputs)]
    assert model.reconstruction_rate(triples, cfg["seq_len"], st, beam=beam, eps=eps) == sum(same) / len(same)
    # a decoder cannot be asked to fail, so the comparison itself is checked on rows made from the inputs: rate 1
    from ark_amd import graphs as G
    seq = torch.from_numpy(z["seq"]).cuda()
    assert torch.equal(G.canon(seq, eos=st["EOS"]).key, model._triple_keys(triples, st))


@pytest.mark.parametrize("beam", [1, 3])
def test_interpolation_statistics_are_the_same_from_device_counts(beam, capsys):
    from kgvae.experiments import interpolation as I
    model, cfg = _trained("sail_small")
    capsys.readouterr()
    out = {}
    for device_stats in (False, True):
        torch.manual_seed(7)
        a = I.latent_smoothness_score_autoreg(model, steps=6, epsilon=0.6, n_anchors=2, n_dirs=2, beam=beam, device_stats=device_stats)
        b = I.latent_flip_rate_autoreg(model, steps=9, epsilon=0.5, n_anchors=2, n_dirs=3, beam=beam, device_stats=device_stats)
        out[device_stats] = (a, b, capsys.readouterr().out)
    assert out[True] == out[False]
    assert out[True][1][0] > 0          # some step flips the graph: the comparison is not one of constants


def test_train_logs_generation_rates_only_when_asked(tmp_path):
    from kgvae.experiments import train as T
    base = yaml.safe_load(open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "configs", "sail_syn-paths.yaml")))
    base.update(model_type="SAIL", d_model=64, num_epochs=2, batch_size=64, save_every=2, compression_log_every=2,
                learning_rate=1e-3, synthetic_sizes={"n_train": 512, "n_val": 128, "n_test": 64}, verify_every=1,
                num_generated_latent_graphs=300)
    for tag, extra in (("on", {"device_graph_stats": True}), ("off", {})):
        cpath = tmp_path / f"{tag}.yaml"
        yaml.safe_dump(dict(base, **extra), open(cpath, "w"))
        ck = tmp_path / f"ck_{tag}"
        T.main(["--config", str(cpath), "--checkpoint-dir", str(ck)])
        run = ck / os.listdir(ck)[0]
        rows = [json.loads(line) for line in open(run / "metrics.jsonl")]
        gen = [r for r in rows if any(k.startswith("generation/") for k in r)]
        if tag == "on":
            assert len(gen) == 2
            for r in gen:
                assert set(r) == {"generation/unique_rate", "generation/novel_rate"}
                assert 0.0 <= r["generation/unique_rate"] <= 1.0 and 0.0 <= r["generation/novel_rate"] <= 1.0
        else:
            assert gen == []
        assert len([r for r in rows if "train/loss" in r]) == 2
