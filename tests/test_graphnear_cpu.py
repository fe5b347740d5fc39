"""Host side of the nearest-graph search (ark_amd.graphs.nearest, ark_graph_nearest), no GPU needed:
  * the plain restatement the GPU tests compare the kernel with (tests/graphnear_ref.py) is pinned to interpolation.jaccard on
    what seq_to_triples parses;
  * the histogram bin computed on the integers is floor(10 J) in exact arithmetic;
  * the cross-multiplied comparison of the restatement orders fractions as fractions.Fraction does;
  * the row recipe of the GPU tests yields what the tests rely on: ties for the best reference and fractional J."""
import itertools
from fractions import Fraction

import numpy as np

from kgvae.experiments import interpolation as I
from kgvae.model.utils import seq_to_triples
from tests import graphnear_ref as N


def _direct(qrows, rrows, exclude_self):
    """idx by interpolation.jaccard on the parsed triples, the first maximum winning (floats: correctly rounded quotients of
    integers below 2^11 are equal exactly when the fractions are)"""
    parse = lambda rows: [set(seq_to_triples([int(x) for x in row], {"EOS": N.EOS}, 3, 1000)) for row in rows]
    qs, rs = parse(qrows), parse(rrows)
    idx = []
    for q, a in enumerate(qs):
        js = [(I.jaccard(a, b), -r) for r, b in enumerate(rs) if not (exclude_self and r == q)]
        idx.append(-max(js)[1] if js else -1)
    return idx, qs, rs


def test_restatement_is_the_argmax_of_interpolation_jaccard():
    for cap, pool, nq, nr in ((1, 4, 20, 30), (3, 12, 40, 60), (8, 24, 30, 50)):
        qrows, qsets = N.pool_rows(cap, pool, nq, seed=cap)
        rrows, rsets = N.pool_rows(cap, pool, nr, seed=100 + cap)
        assert qsets == N.row_sets(qrows)
        for exclude_self in (False, True):
            refs = (qrows, qsets) if exclude_self else (rrows, rsets)
            idx, inter, dq, dr = N.nearest_ref(qsets, refs[1], exclude_self)
            want, qs, rs = _direct(qrows, refs[0], exclude_self)
            assert idx.tolist() == want
            for q in range(nq):
                assert (inter[q], dq[q], dr[q]) == (len(qs[q] & rs[idx[q]]), len(qs[q]), len(rs[idx[q]]))
    one = N.nearest_ref([{1}, set()], [{1}], exclude_self=True)
    assert [x.tolist() for x in one] == [[-1, 0], [-1, 0], [1, 0], [-1, 1]]
    none = N.nearest_ref([{1}, set()], [])
    assert [x.tolist() for x in none] == [[-1, -1], [-1, -1], [1, 0], [-1, -1]]


def test_histogram_bin_is_floor_of_ten_j():
    assert N.hist_bin(0, 0, 0) == 10 and N.hist_bin(0, 0, 5) == 0 and N.hist_bin(0, 4, 0) == 0
    for dq, dr in itertools.product(range(1, 14), repeat=2):
        for inter in range(0, min(dq, dr) + 1):
            j = Fraction(inter, dq + dr - inter)
            assert N.hist_bin(inter, dq, dr) == (10 if j == 1 else int(10 * j)), (inter, dq, dr)
    # the largest lists: all unions up to 2048, vectorised
    union = np.arange(1, 2049)[:, None]
    inter = np.arange(0, 2049)[None, :]
    ok = inter <= union
    bins = (10 * inter) // union
    assert ((bins == 10) == (inter == union))[ok].all()
    assert ((bins * union <= 10 * inter) & (10 * inter < (bins + 1) * union))[ok].all()


def test_cross_multiplication_orders_fractions_exactly():
    fracs = [(n, d) for d in range(1, 41) for n in range(0, d + 1)] + [(1023, 2048), (1024, 2047), (511, 1024), (1, 2)]
    for (a, b), (c, d) in itertools.product(fracs, repeat=2):
        assert (a * d > c * b) == (Fraction(a, b) > Fraction(c, d))
    assert 1024 * 2048 < 2 ** 31          # the kernel's products fit its 32-bit integers


def test_the_row_recipe_gives_ties_and_fractions():
    for cap, pool, nq, nr in ((3, 12, 65, 130), (8, 24, 64, 257), (9, 24, 40, 100)):
        _, qsets = N.pool_rows(cap, pool, nq, seed=1)
        _, rsets = N.pool_rows(cap, pool, nr, seed=2)
        idx, inter, dq, dr = N.nearest_ref(qsets, rsets)
        best = [Fraction(*N.frac(inter[q], dq[q], dr[q])) for q in range(nq)]
        tied = sum(sum(Fraction(*N.frac(len(a & b), len(a), len(b))) == best[q] for b in rsets) > 1 for q, a in enumerate(qsets))
        fractional = sum(0 < j < 1 for j in best)
        assert 4 * tied >= nq and 4 * fractional >= nq, (cap, tied, fractional)
