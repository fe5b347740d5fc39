"""The nearest reference graph on the device: ark_graph_nearest (ark_amd/csrc/graphkey.hip) through ark_amd.graphs.nearest
against the plain restatement of tests/graphnear_ref.py (itself pinned to interpolation.jaccard by tests/test_graphnear_cpu.py),
integer for integer, on both sides of the switches between its three kernels and for every split of the reference axis; and
what is built on it: nearest_summary, dataset_canon, graph_stats of both model kinds and the training loop's
`device_graph_nearest` key.  Rows come from small pools of triples, so ties for the best reference and fractional J are the
rule (tests/test_graphnear_cpu.py::test_the_row_recipe_gives_ties_and_fractions)."""
import json
import math
import os

import numpy as np
import pytest
import torch
import yaml

from tests import graphnear_ref as N

pytestmark = pytest.mark.gpu

EOS = N.EOS
# (cap, pool, NQ, NR): both caps <= 8 take the lane-per-pair kernel with the lists in registers, caps up to 64 the one with a
# linear merge in LDS, 65 and above the wave-per-row kernel (65: two elements per lane); 212 is the wd-articles cap, 1024 the
# limit (and the 4-query tile)
SHAPES = [(1, 4, 33, 70), (3, 12, 65, 130), (8, 24, 64, 257), (9, 24, 40, 100), (64, 160, 20, 70), (65, 160, 20, 70),
          (212, 500, 9, 40), (1024, 2500, 5, 12)]
_CASES = {}


def _case(cap, pool, nq, nr, capr=None, wide=False):
    """(query token rows, reference token rows, their sets, the restatement's answer); computed once and shared"""
    k = (cap, pool, nq, nr, capr, wide)
    if k not in _CASES:
        qt, _ = N.pool_rows(cap, pool, nq, seed=10 * cap + 1, wide=wide)
        rt, _ = N.pool_rows(cap if capr is None else capr, pool, nr, seed=10 * cap + 2, wide=wide)
        if cap >= 64 and capr is None:          # large lists hardly ever tie by chance: plant ties
            rt[nr - 1] = rt[3]                  # a reference row again at a higher index
            rt[5] = rt[nr - 2] = qt[1]          # a query among the references, twice
        qs, rs = N.row_sets(qt), N.row_sets(rt)
        _CASES[k] = (qt, rt, qs, rs, N.nearest_ref(qs, rs))
    return _CASES[k]


def _batch(toks):
    from ark_amd import graphs as G
    return G.canon(torch.from_numpy(np.ascontiguousarray(toks)).cuda(), eos=EOS)


def _host(near):
    return tuple(x.cpu().numpy() for x in near)


def _assert_equal(near, want):
    got = _host(near)
    for name, g, w in zip(("idx", "inter", "dq", "dr"), got, want):
        assert g.dtype == np.int32
        assert np.array_equal(g, w), (name, g.tolist(), w.tolist())


@pytest.mark.parametrize("cap,pool,nq,nr", SHAPES)
def test_nearest_equals_the_restatement(cap, pool, nq, nr):
    from ark_amd import graphs as G
    qt, rt, qs, rs, want = _case(cap, pool, nq, nr)
    near = G.nearest(_batch(qt), _batch(rt))
    assert isinstance(near, G.Nearest) and all(x.is_cuda for x in near)
    _assert_equal(near, want)
    if cap >= 64:
        assert want[0][1] == 5                  # the planted copy of query 1: the lower of its two rows
        assert want[1][1] == want[2][1] == want[3][1]


@pytest.mark.parametrize("capq,capr", [(3, 8), (8, 9), (64, 23), (65, 8), (9, 212)])
def test_nearest_with_different_caps(capq, capr):
    from ark_amd import graphs as G
    qt, rt, qs, rs, want = _case(capq, 24, 37, 90, capr=capr)
    qb, rb = _batch(qt), _batch(rt)
    assert qb.canon.shape[1] == capq and rb.canon.shape[1] == capr
    _assert_equal(G.nearest(qb, rb), want)


@pytest.mark.parametrize("cap", [8, 23, 65])
def test_nearest_on_full_width_tokens(cap):
    from ark_amd import graphs as G
    qt, rt, qs, rs, want = _case(cap, 160, 20, 70, wide=True)
    assert max(max(s) for s in rs if s) > (1 << 62)          # the packed word is used to its last bits
    _assert_equal(G.nearest(_batch(qt), _batch(rt)), want)


@pytest.mark.parametrize("cap,pool,nq,nr", [(8, 24, 64, 257), (212, 500, 9, 40), (9, 24, 40, 100), (64, 160, 20, 70)])
def test_the_result_does_not_depend_on_the_strips(cap, pool, nq, nr):
    from ark_amd import graphs as G
    qt, rt, qs, rs, want = _case(cap, pool, nq, nr)
    qb, rb = _batch(qt), _batch(rt)
    for strips in (1, 2, 7, 0):
        _assert_equal(G.nearest(qb, rb, strips=strips), want)
    for strips in (1, 3):
        _assert_equal(G.nearest(qb, qb, exclude_self=True, strips=strips), N.nearest_ref(qs, qs, exclude_self=True))


def _rows_of(graphs, cap):
    toks = np.full((len(graphs), 3 * cap + 1), EOS, dtype=np.int64)
    toks[:, 0] = N.BOS
    for b, g in enumerate(graphs):
        flat = [t for tr in g for t in tr]
        toks[b, 1:1 + len(flat)] = flat
    return toks


@pytest.mark.parametrize("cap", [3, 9, 65])
def test_empty_graphs_follow_the_jaccard_conventions(cap):
    from ark_amd import graphs as G
    a, b, c = (5, 1000, 6), (7, 1001, 8), (9, 1002, 9)
    queries = [[], [a], [], [b, a], [c]]
    for refs in ([[b], [], [a], []], [[b], [a, b]], [[], []]):
        qt, rt = _rows_of(queries, cap), _rows_of(refs, cap)
        want = N.nearest_ref(N.row_sets(qt), N.row_sets(rt))
        got = _host(G.nearest(_batch(qt), _batch(rt)))
        _assert_equal(G.nearest(_batch(qt), _batch(rt)), want)
        for q, g in enumerate(queries):
            i, inter, dq, dr = (int(x[q]) for x in got)
            assert dq == len(g)
            if not g:                           # an empty query: J = 1 with the first empty reference, else J = 0 at row 0
                assert i == (refs.index([]) if [] in refs else 0) and inter == 0 and dr == len(refs[i])
            j = G.jaccard_from_counts(inter, dq, dr)
            assert j == (1.0 if not g and not refs[i] else 0.0 if not g or not refs[i] else inter / (dq + dr - inter))
    # a query that shares nothing with any reference: J = 0 everywhere, the first row wins
    got = _host(G.nearest(_batch(_rows_of([[c], [c, c]], cap)), _batch(_rows_of([[a, b], [b], [a]], cap))))
    assert [x.tolist() for x in got] == [[0, 0], [0, 0], [1, 1], [2, 2]]


@pytest.mark.parametrize("cap", [8, 23, 65])
def test_exclude_self(cap):
    from ark_amd import graphs as G
    qt = _case(cap, 24 if cap == 8 else 160, 64, 257)[0].copy()
    own = [(40 + k, 1003, 41 + k) for k in range(3)]          # triples of no pool: rows 9 and 50 equal each other alone
    qt[9] = qt[50] = _rows_of([own], cap)[0]
    qt[20] = qt[4]
    sets = N.row_sets(qt)
    want = N.nearest_ref(sets, sets, exclude_self=True)
    batch = _batch(qt)
    near = G.nearest(batch, batch, exclude_self=True)
    _assert_equal(near, want)
    idx, inter, dq, dr = _host(near)
    assert not (idx == np.arange(len(sets))).any()
    assert idx[9] == 50 and idx[50] == 9 and inter[9] == dq[9] == dr[9] == 3
    assert inter[4] == dq[4] == dr[4] and inter[20] == dq[20] == dr[20] and idx[20] <= 4
    plain = _host(G.nearest(batch, batch))
    assert np.array_equal(plain[1], plain[2]) and np.array_equal(plain[2], plain[3])          # every row finds itself or a twin
    assert (plain[0] <= np.arange(len(sets))).all()
    # one row against itself: nothing is admissible
    one = _batch(qt[9:10])
    assert [x.tolist() for x in _host(G.nearest(one, one, exclude_self=True))] == [[-1], [-1], [3], [-1]]
    assert [x.tolist() for x in _host(G.nearest(one, one))] == [[0], [3], [3], [3]]


def test_no_references_and_no_queries():
    from ark_amd import graphs as G
    qt = _case(3, 12, 65, 130)[0]
    batch = _batch(qt)
    none = G.canon(torch.empty(0, qt.shape[1], dtype=torch.int64, device="cuda"), eos=EOS)
    idx, inter, dq, dr = _host(G.nearest(batch, none))
    assert (idx == -1).all() and (inter == -1).all() and (dr == -1).all()
    assert np.array_equal(dq, batch.nset.cpu().numpy())
    empty = G.nearest(none, batch)
    assert all(x.shape == (0,) and x.dtype == torch.int32 and x.is_cuda for x in empty)
    assert G.nearest_summary(empty)["n"] == 0


@pytest.mark.parametrize("wide_side", ["queries", "references"])
def test_more_than_1024_triples_are_refused_and_nothing_is_written(wide_side):
    from ark_amd import graphs as G
    from ark_amd._lib import ArkError

    def batch(cap):
        return G.GraphBatch(torch.full((2, cap), -1, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"),
                            torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, 2, dtype=torch.int64, device="cuda"))
    q, r = (batch(1025), batch(4)) if wide_side == "queries" else (batch(4), batch(1025))
    outs = [torch.full((2,), 77, dtype=torch.int32, device="cuda") for _ in range(4)]
    assert G.nearest_raw(q, r, False, 0, *outs) == -2          # ARK_ERR_SHAPE
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == 77).all())
    with pytest.raises(ArkError):
        G.nearest(q, r)


@pytest.mark.parametrize("cap,pool,nq,nr", [(3, 12, 65, 130), (9, 24, 40, 100), (64, 160, 20, 70)])
def test_summary_equals_the_host_recomputation(cap, pool, nq, nr):
    """integers exactly; the mean within 1e-9 (float64 rounding over <= 10^4 terms in [0, 1] stays below 2e-12)"""
    from ark_amd import graphs as G
    qt, rt, qs, rs, want = _case(cap, pool, nq, nr)
    near = G.nearest(_batch(qt), _batch(rt))
    got, ref = G.nearest_summary(near), N.summary_ref(*want)
    assert set(got) == {"n", "mean_jaccard", "hist", "copied", "copied_rate"}
    assert got["n"] == ref["n"] == nq and got["hist"] == ref["hist"] and len(got["hist"]) == 11 and sum(got["hist"]) == nq
    assert got["copied"] == ref["copied"] == got["hist"][10] and got["copied_rate"] == ref["copied_rate"]
    assert abs(got["mean_jaccard"] - ref["mean_jaccard"]) <= 1e-9
    assert 0 < got["copied"] < nq                             # some J = 1, some below
    j = G.jaccard_tensor(near)
    assert j.dtype == torch.float64 and j.is_cuda
    assert j.cpu().tolist() == [G.jaccard_from_counts(int(a), int(b), int(c)) for a, b, c in zip(*want[1:])]
    # rows without a reference are NaN in the tensor and left out of the summary
    qb = _batch(qt[:1])
    lone = G.nearest(qb, qb, exclude_self=True)
    assert math.isnan(float(G.jaccard_tensor(lone)[0]))
    s = G.nearest_summary(lone)
    assert s["n"] == 0 and s["hist"] == [0] * 11 and s["copied"] == 0 and s["copied_rate"] == 0.0 and math.isnan(s["mean_jaccard"])


# ---------------------------------------------------------------------------------------------------------------- models
def _model(name):
    from tests.test_sample_decode_gpu import _model as build
    return build(name)


def _train_rows(toks, lens, cfg):
    """a "training split" of generated rows: every second one, plus three of the others with one token of their first triple
    replaced -> (token rows on the device, their lens or None)"""
    rows = toks[1::2].clone()
    n = _parsed_sizes(toks[1::2], None if lens is None else lens[1::2], cfg)
    pick = [i for i in range(rows.shape[0]) if n[i] >= 1][:3]
    assert pick
    altered = rows[pick]
    altered[:, 3] = torch.where(altered[:, 3] == cfg["ENT_BASE"], altered[:, 3] + 1, torch.full_like(altered[:, 3], cfg["ENT_BASE"]))
    train = torch.cat([toks[::2], altered])
    return train, (None if lens is None else torch.cat([lens[::2], lens[1::2][pick]]))


def _sets(toks, lens, cfg):
    from kgvae.model.utils import seq_to_triples
    toks = toks.cpu()
    lens = [toks.shape[1]] * toks.shape[0] if lens is None else lens.cpu().tolist()
    return [set(seq_to_triples(row[:n], cfg["special_tokens"], cfg["ENT_BASE"], cfg["REL_BASE"])) for row, n in zip(toks, lens)]


def _parsed_sizes(toks, lens, cfg):
    return [len(s) for s in _sets(toks, lens, cfg)]


def _check_stats(stats, base, toks, lens, train, train_lens, cfg):
    gen, tr = _sets(toks, lens, cfg), _sets(train, train_lens, cfg)
    ref = N.summary_ref(*N.nearest_ref(gen, tr))
    other = N.summary_ref(*N.nearest_ref(gen, gen, exclude_self=True))
    print("copied_rate", ref["copied_rate"], "nearest_train_jaccard", ref["mean_jaccard"], "nearest_other", other["mean_jaccard"])
    assert set(stats) == set(base) | {"nearest_train_jaccard", "nearest_train_hist", "copied_rate", "nearest_other_jaccard"}
    assert {k: stats[k] for k in base} == base
    assert stats["nearest_train_hist"] == ref["hist"] and stats["copied_rate"] == ref["copied_rate"]
    assert abs(stats["nearest_train_jaccard"] - ref["mean_jaccard"]) <= 1e-9
    assert abs(stats["nearest_other_jaccard"] - other["mean_jaccard"]) <= 1e-9
    assert 0.0 < stats["copied_rate"] < 1.0


@pytest.mark.parametrize("name,beam,per_latent", [("sail_tiny", 1, False), ("sail_small", 2, True)])
def test_sail_graph_stats_with_the_nearest_training_graph(name, beam, per_latent):
    from ark_amd import graphs as G
    model, cfg = _model(name)
    st = cfg["special_tokens"]
    z = torch.randn(48, cfg["d_latent"], generator=torch.Generator().manual_seed(4)).cuda()
    toks, lens = model.decode_latent_tokens(z, cfg["seq_len"], st, beam=beam, per_latent=per_latent)
    train, train_lens = _train_rows(toks, lens, cfg)
    train_graphs = G.canon(train, train_lens, eos=st["EOS"])
    kw = dict(beam=beam, per_latent=per_latent, z=z)
    base = model.graph_stats(48, cfg["seq_len"], st, **kw)
    assert set(base) == {"n", "unique", "unique_rate", "empty", "mean_triples"}          # without the new arguments: as before
    assert set(model.graph_stats(48, cfg["seq_len"], st, train_keys=train_graphs.key, **kw)) == set(base) | {"novel", "novel_rate"}
    stats = model.graph_stats(48, cfg["seq_len"], st, train_graphs=train_graphs, diversity=True, **kw)
    _check_stats(stats, base, toks, lens, train, train_lens, cfg)
    only = model.graph_stats(48, cfg["seq_len"], st, train_graphs=train_graphs, **kw)
    assert set(only) == set(base) | {"nearest_train_jaccard", "nearest_train_hist", "copied_rate"}


def test_ark_graph_stats_with_the_nearest_training_graph():
    from ark_amd import graphs as G
    model, cfg = _model("ark_tiny")
    st = cfg["special_tokens"]
    kw = dict(sample=True, temperature=1.3, top_k=5, sampler="fused", seed=11)
    toks = model.generate(cfg["seq_len"], st, batch_size=40, **kw)
    train, _ = _train_rows(toks, None, cfg)
    train_graphs = G.canon(train, eos=st["EOS"])
    base = model.graph_stats(40, cfg["seq_len"], st, **kw)
    assert set(base) == {"n", "unique", "unique_rate", "empty", "mean_triples"}
    stats = model.graph_stats(40, cfg["seq_len"], st, train_graphs=train_graphs, diversity=True, **kw)
    _check_stats(stats, base, toks, None, train, None, cfg)


@pytest.mark.parametrize("use_padding", [False, True])
def test_dataset_canon_keys_are_dataset_keys(use_padding):
    from ark_amd import graphs as G
    from tests.test_graphkey_cpu import _dataset
    ds = _dataset(use_padding, permute=True)
    keys = G.dataset_keys(ds, "cuda")
    for chunk in (16384, 4):
        batch = G.dataset_canon(ds, "cuda", chunk=chunk)
        assert torch.equal(batch.key, keys)
        assert batch.n.cpu().tolist() == [len(g) for g in ds.graphs]
        assert batch.canon.shape == (len(ds), G.row_cap(ds.seq_len))
    # every graph of the split is its own nearest graph's equal
    near = G.nearest(batch, batch)
    assert G.nearest_summary(near)["copied_rate"] == 1.0
    if use_padding:                             # chunks of different widths (no fixed seq_len) are padded to one cap
        ds.seq_len = None
        ragged = G.dataset_canon(ds, "cuda", chunk=2)
        assert torch.equal(ragged.key, keys) and ragged.canon.shape[1] == 4
        assert torch.equal(ragged.canon, batch.canon[:, :4]) and bool((batch.canon[:, 4:] == -1).all())


def test_train_logs_the_nearest_training_graph_only_when_asked(tmp_path):
    from kgvae.experiments import train as T
    base = yaml.safe_load(open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "configs", "sail_syn-paths.yaml")))
    base.update(model_type="SAIL", d_model=64, num_epochs=2, batch_size=64, save_every=2, compression_log_every=2,
                learning_rate=1e-3, synthetic_sizes={"n_train": 512, "n_val": 128, "n_test": 64}, verify_every=1,
                num_generated_latent_graphs=300)
    two = {"generation/unique_rate", "generation/novel_rate"}
    cases = (("both", {"device_graph_stats": True, "device_graph_nearest": True},
              two | {"generation/nearest_train_jaccard", "generation/copied_rate"}),
             ("stats", {"device_graph_stats": True}, two))
    for tag, extra, keys in cases:
        cpath = tmp_path / f"{tag}.yaml"
        yaml.safe_dump(dict(base, **extra), open(cpath, "w"))
        ck = tmp_path / f"ck_{tag}"
        T.main(["--config", str(cpath), "--checkpoint-dir", str(ck)])
        run = ck / os.listdir(ck)[0]
        rows = [json.loads(line) for line in open(run / "metrics.jsonl")]
        gen = [r for r in rows if any(k.startswith("generation/") for k in r)]
        assert len(gen) == 2
        for r in gen:
            assert set(r) == keys
            assert all(0.0 <= r[k] <= 1.0 for k in keys)
