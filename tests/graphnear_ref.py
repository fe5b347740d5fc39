"""Plain Python statement of ark_graph_nearest (ark_amd/csrc/graphkey.hip): two nested loops over Python sets of packed
triples, the Jaccard index kept as (num, den) and compared by cross-multiplication, the first index winning; and the rows
the tests feed it: token rows drawn from a small pool of triples, so that ties and fractional J are common."""
import numpy as np

EOS = 2
BOS = 1


def frac(inter, dq, dr):
    """J as (num, den): (1, 1) for two empty sets, else (inter, |union|)"""
    union = dq + dr - inter
    return (1, 1) if union == 0 else (inter, union)


def nearest_ref(qsets, rsets, exclude_self=False):
    """-> (idx, inter, dq, dr) int32 [len(qsets)]: per query set the first reference set with the largest J; -1 in idx,
    inter, dr for a query without an admissible reference"""
    out = np.full((4, len(qsets)), -1, dtype=np.int32)
    for q, a in enumerate(qsets):
        out[2, q] = len(a)
        best = None
        for r, b in enumerate(rsets):
            if exclude_self and r == q:
                continue
            inter = len(a & b)
            num, den = frac(inter, len(a), len(b))
            if best is None or num * best[1] > best[0] * den:          # strictly larger only: the first index wins
                best = (num, den)
                out[0, q], out[1, q], out[3, q] = r, inter, len(b)
    return tuple(out)


def hist_bin(inter, dq, dr):
    """the histogram bin of a row of a Nearest, on the integers"""
    num, den = frac(inter, dq, dr)
    return 10 if num == den else (10 * num) // den


def summary_ref(idx, inter, dq, dr):
    """nearest_summary on the host: exact integers, the mean in Python floats"""
    from ark_amd.graphs import jaccard_from_counts
    rows = [(int(i), int(a), int(b)) for k, i, a, b in zip(idx, inter, dq, dr) if k >= 0]
    hist = [0] * 11
    for t in rows:
        hist[hist_bin(*t)] += 1
    n = len(rows)
    mean = sum(jaccard_from_counts(*t) for t in rows) / n if n else float("nan")
    return {"n": n, "mean_jaccard": mean, "hist": hist, "copied": hist[10], "copied_rate": hist[10] / max(1, n)}


def pack(triple):
    return (int(triple[0]) << 42) | (int(triple[1]) << 21) | int(triple[2])


def pool_rows(cap, pool, rows, seed, wide=False):
    """(toks [rows, 3 * cap + 1] int64, sets): row b holds n_b triples, n_b uniform in 0 .. cap, each drawn uniformly (with
    repeats) from `pool` distinct token triples, in drawn order, then EOS.  sets[b] = the packed values as a Python set.
    wide: the tokens are 2^21 - 1 and its neighbours, so the packed words use their top bits."""
    rng = np.random.default_rng(seed)
    if wide:
        alphabet = np.array([(1 << 21) - 1 - k for k in range(6)], dtype=np.int64)
    else:
        alphabet = np.arange(3, 3 + max(6, int(np.ceil(pool ** (1 / 3))) + 2), dtype=np.int64)
    # (the pool depends on its size alone: queries and references of a case draw from the same triples)
    codes = np.random.default_rng(pool).choice(len(alphabet) ** 3, size=pool, replace=False)
    A = len(alphabet)
    triples = np.stack([alphabet[codes // (A * A)], alphabet[(codes // A) % A], alphabet[codes % A]], axis=1)
    toks = np.full((rows, 3 * cap + 1), EOS, dtype=np.int64)
    toks[:, 0] = BOS
    sets = []
    for b in range(rows):
        n = int(rng.integers(0, cap + 1))
        pick = triples[rng.integers(0, pool, size=n)]
        toks[b, 1:1 + 3 * n] = pick.reshape(-1)
        sets.append({pack(t) for t in pick})
    return toks, sets


def row_sets(toks):
    """the sets of packed triples seq_to_triples reads from token rows"""
    from kgvae.model.utils import seq_to_triples
    return [{pack(t) for t in seq_to_triples([int(x) for x in row], {"EOS": EOS}, 0, 0)} for row in np.asarray(toks)]
