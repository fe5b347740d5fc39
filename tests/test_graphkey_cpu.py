"""Host side of the graph keys (ark_amd/graphs.py, ark_amd/csrc/graphkey.hip), no GPU needed:
  * the plain restatement the GPU tests compare the kernels with (tests/graphkey_ref.py) is pinned to canonical_graph_string:
    two rows have equal restated keys exactly when their strings are equal;
  * the integer-to-number derivations behind pair_stats are pinned to interpolation's jaccard / flip_stats / jaccard_stats /
    overlap_stats on hand-made sets;
  * dataset_keys' row builder is pinned to triples_to_seq and leaves every generator where it was."""
import itertools
import random

import numpy as np
import torch

from ark_amd import graphs as G
from kgvae.experiments import interpolation as I
from kgvae.model.utils import GraphSeqDataset, canonical_graph_string, seq_to_triples, triples_to_seq
from tests import graphkey_ref as R

EOS = 2


def _fixture_rows():
    """token rows by construction: K base graphs, each several times with its triples shuffled; variants that differ only in
    a doubled triple; rows with an EOS inside a slot, EOS at a slot boundary, and empty rows"""
    rng = random.Random(5)
    ents, rels = [3, 4, 5, 6, 7], [1000, 1001, 1002]
    W = 1 + 3 * 6 + 1
    rows = []

    def emit(triples, tail_eos=True):
        body = [t for tr in triples for t in tr]
        row = [1] + body + ([EOS] if tail_eos else [])
        rows.append(row + [0] * (W - len(row)))

    bases = []
    for k in range(6):
        bases.append([(rng.choice(ents), rng.choice(rels), rng.choice(ents)) for _ in range(2 + k % 4)])
    for g in bases:
        for _ in range(4):                       # the same graph, shuffled: equal strings
            emit(rng.sample(g, len(g)))
        emit(g + [g[0]])                         # a doubled triple: another list, another string
        emit([g[0]] + g)                         # the same doubled triple elsewhere: equal to the previous one
    mid = [(3, EOS, 4), (5, 1000, EOS)]          # EOS inside a slot is an ordinary token
    emit(mid)
    emit(mid[::-1])
    emit([(3, 1000, 4)] + [(EOS, 1001, 5)])      # EOS at a slot boundary ends the list: == [(3, 1000, 4)] alone
    emit([(3, 1000, 4)])
    emit([])                                     # empty rows
    emit([(EOS, 1000, 3)])
    rows.append([1] + [0] * (W - 1))             # PAD tokens are ordinary tokens: no EOS, six (0, 0, 0) slots
    return np.array(rows, dtype=np.int64)


def test_restated_keys_are_equal_exactly_when_the_strings_are():
    rows = _fixture_rows()
    canon, n, nset, key, strings = R.canon_ref(rows, None, EOS)
    shared = sum(strings.count(s) > 1 for s in strings)
    assert 2 * shared >= len(strings), (shared, len(strings))          # the equality direction is not vacuous
    assert len(set(strings)) > 8                                       # nor the inequality direction
    keys = [tuple(k) for k in key.tolist()]
    for a, b in itertools.combinations(range(len(rows)), 2):
        assert (keys[a] == keys[b]) == (strings[a] == strings[b]), (a, b, strings[a], strings[b])
    # the lists themselves: ascending, duplicates kept, -1 behind them
    for b in range(len(rows)):
        assert list(canon[b, :n[b]]) == sorted(canon[b, :n[b]]) and (canon[b, n[b]:] == -1).all()
        assert nset[b] == len(set(canon[b, :n[b]].tolist()))
    assert n[-1] == 6 and nset[-1] == 1 and n[-2] == 0 and n[-3] == 0
    # the vectorised numpy fold is the scalar definition
    for b in range(len(rows)):
        assert tuple(R.to_i64(k) for k in R.key_of([int(x) for x in canon[b, :n[b]]])) == keys[b]


def test_key_definition_is_pinned():
    """stored keys stay valid: the two seeds, the splitmix64 finaliser and the closing mix with n"""
    assert R.mix(0) == 0 and R.mix(1) == 0x5692161D100B05E5
    assert R.mix(R.SEED0) == 0xE220A8397B1DCDAF          # splitmix64's first output from state 0
    assert int(R.mix_np(np.uint64(1))) == R.mix(1) and int(R.mix_np(np.uint64(R.M64))) == R.mix(R.M64)
    assert R.key_of([]) == (R.mix(R.SEED0), R.mix(R.SEED1))
    p = (5 << 42) | (1000 << 21) | 7
    assert R.key_of([p]) == (R.mix(R.mix(R.SEED0 ^ p) ^ 1), R.mix(R.mix(R.SEED1 ^ p) ^ 1))
    assert R.key_of([p, p]) != R.key_of([p])


def test_lengths_cut_rows_as_the_parser_does():
    rows = _fixture_rows()[:8]
    for lens in ([0] * 8, [1] * 8, [3, 4, 5, 6, 7, 8, 9, 10], [100] * 8, [-3] * 8):
        canon, n, _, _, strings = R.canon_ref(rows, lens, EOS)
        for b in range(8):
            cut = rows[b][:max(0, min(lens[b], rows.shape[1]))]
            assert strings[b] == str(sorted(R.row_graph(cut, None, EOS)))
            assert n[b] == min(len(R.row_graph(rows[b], None, EOS)), max(0, (min(lens[b], rows.shape[1]) - 1) // 3))


SETS = [set(), {(1, 2, 3)}, {(1, 2, 3), (4, 5, 6)}, {(4, 5, 6)}, {(1, 2, 3), (4, 5, 6), (7, 8, 9)}, {(9, 9, 9)}]


def _counts(a, b):
    return len(a & b), len(a), len(b)


def test_jaccard_and_equality_from_counts():
    for a in SETS:
        for b in SETS:
            assert G.jaccard_from_counts(*_counts(a, b)) == I.jaccard(a, b), (a, b)
            assert G.sets_equal(*_counts(a, b)) == (a == b), (a, b)
    assert G.jaccard_from_counts(0, 0, 0) == 1.0 and G.jaccard_from_counts(0, 0, 2) == 0.0 == G.jaccard_from_counts(0, 3, 0)


def test_walk_statistics_from_counts():
    rng = random.Random(2)
    walks = [[rng.choice(SETS) for _ in range(9)] for _ in range(20)] + [[SETS[0]] * 4, [SETS[2]] * 5, SETS[:], [SETS[1]]]
    for sets in walks:
        prev = [_counts(c, p) for p, c in zip(sets, sets[1:])]
        anchor = [_counts(c, sets[0]) for c in sets[1:]]
        assert G.flip_stats_from_equal([G.sets_equal(*t) for t in prev]) == I.flip_stats(sets)
        assert G.jaccard_stats_from_counts(prev, anchor) == I.jaccard_stats(sets)
    # overlap_stats divides by the LIST lengths (duplicates counted)
    lists = [[(1, 2, 3), (1, 2, 3), (4, 5, 6)], [], [(4, 5, 6)], [(1, 2, 3), (7, 8, 9)], [(1, 2, 3), (4, 5, 6)]]
    want = I.overlap_stats(lists)
    got = [G.overlap_from_counts(len(set(p) & set(c)), len(p), len(set(lists[0]) & set(c)), len(lists[0]))
           for p, c in zip(lists, lists[1:])]
    assert got == want


def test_walk_pairs_order():
    ia, ib = G.walk_pairs(2, 3)
    assert ia.tolist() == [1, 2, 3, 5, 6, 7] * 2
    assert ib.tolist() == [0, 1, 2, 4, 5, 6] + [0, 0, 0, 4, 4, 4]


def _dataset(use_padding, permute):
    rng = random.Random(3)
    sizes = [0, 1, 3, 4, 2, 4] if use_padding else [3] * 6
    graphs = [[(rng.randrange(9), rng.randrange(4), rng.randrange(9)) for _ in range(T)] for T in sizes]
    return GraphSeqDataset(graphs, None, None, permute=permute, use_padding=use_padding, pad_eid=9, pad_rid=4, max_triples=4,
                           ent_base=3, rel_base=3 + 10, seq_len=2 + 3 * 4 + (0 if use_padding else 3))


def test_dataset_rows_are_triples_to_seq_and_draw_nothing():
    for use_padding in (False, True):
        ds = _dataset(use_padding, permute=True)
        random.seed(11)
        torch.manual_seed(11)
        np.random.seed(11)
        before = (random.getstate(), torch.get_rng_state().clone(), np.random.get_state()[1].copy())
        rows, lens = G.dataset_rows(ds)
        sub, _ = G.dataset_rows(ds, [4, 1])
        assert random.getstate() == before[0]
        assert torch.equal(torch.get_rng_state(), before[1])
        assert (np.random.get_state()[1] == before[2]).all()
        for i, g in enumerate(ds.graphs):
            want = triples_to_seq(g, ds.special_tokens, ds.ent_base, ds.rel_base, ds.seq_len)
            assert rows[i].tolist() == want.tolist(), i
            assert lens[i] == 3 * len(g) + 2
        assert sub.tolist() == rows[[4, 1]].tolist()
        # the restated key of a row is the key of the stored graph, whatever order an epoch would draw
        parsed = [seq_to_triples(rows[i][:lens[i]].tolist(), ds.special_tokens, ds.ent_base, ds.rel_base) for i in range(len(ds))]
        assert [canonical_graph_string(g) for g in parsed] == [canonical_graph_string(g) for g in ds.graphs]
        _, _, _, key, _ = R.canon_ref(rows, lens, ds.special_tokens["EOS"])
        _, _, _, key_full, _ = R.canon_ref(rows, None, ds.special_tokens["EOS"])
        assert (key == key_full).all()


def test_canon_refuses_a_vocabulary_that_does_not_pack():
    import pytest
    from ark_amd._lib import ArkError
    with pytest.raises(ArkError):
        G.canon(torch.zeros(1, 4, dtype=torch.int64), vocab=(1 << 21) + 1)
