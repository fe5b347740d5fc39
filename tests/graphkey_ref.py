"""Plain Python / numpy statement of ark_graph_canon and ark_graph_pair_stats (ark_amd/csrc/graphkey.hip): the parse is the
real kgvae.model.utils.seq_to_triples, the order is Python's sorted() on the (h, r, t) id triples, the key fold is numpy
uint64 arithmetic."""
import numpy as np

from kgvae.model.utils import canonical_graph_string, seq_to_triples

SEED0, SEED1 = 0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F
M64 = (1 << 64) - 1
ENT_BASE, REL_BASE = 3, 1000      # any bases: subtracting them is monotone and the pack adds them back


def mix(x):
    """the splitmix64 finaliser on a Python int"""
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def mix_np(x):
    """the same on numpy uint64 (wrapping products)"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(30))
        x = x * np.uint64(0xBF58476D1CE4E5B9)
        x = x ^ (x >> np.uint64(27))
        x = x * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return x


def row_graph(row, length=None, eos=2):
    """the graph seq_to_triples reads from row[:length]"""
    row = list(int(t) for t in row)
    if length is not None:
        row = row[:max(0, int(length))]
    return seq_to_triples(row, {"EOS": eos}, ENT_BASE, REL_BASE)


def pack(graph):
    """sorted(graph) packed from the raw tokens, as Python ints"""
    return [((h + ENT_BASE) << 42) | ((r + REL_BASE) << 21) | (t + ENT_BASE) for h, r, t in sorted(graph)]


def key_of(packed):
    """the key of ONE sorted packed list, on Python ints (test_graphkey_cpu pins it to fold_keys)"""
    out = []
    for seed in (SEED0, SEED1):
        h = seed
        for p in packed:
            h = mix(h ^ p)
        out.append(mix(h ^ len(packed)))
    return tuple(out)


def fold_keys(canon, n):
    """keys [B, 2] int64 of all rows at once: step i of the fold for every row that has an i-th triple, in numpy uint64"""
    u = np.ascontiguousarray(canon).view(np.uint64)
    n = np.asarray(n, dtype=np.int64)
    key = np.zeros((len(n), 2), dtype=np.uint64)
    for c, seed in enumerate((SEED0, SEED1)):
        h = np.full(len(n), seed, dtype=np.uint64)
        for i in range(int(n.max()) if len(n) else 0):
            h = np.where(i < n, mix_np(h ^ u[:, i]), h)
        key[:, c] = mix_np(h ^ n.astype(np.uint64))
    return key.view(np.int64)


def to_i64(u):
    return u - (1 << 64) if u >= (1 << 63) else u


def canon_ref(toks, lens=None, eos=2):
    """-> (canon [B, cap] int64, n [B] int32, nset [B] int32, key [B, 2] int64, strings [B]) for token rows `toks` [B, row_len]
    (numpy), lens [B] or None"""
    toks = np.asarray(toks)
    B, row_len = toks.shape
    cap = max(0, (row_len - 1) // 3)
    canon = np.full((B, cap), -1, dtype=np.int64)
    n = np.zeros(B, dtype=np.int32)
    nset = np.zeros(B, dtype=np.int32)
    strings = []
    for b in range(B):
        length = None if lens is None else min(int(lens[b]), row_len)
        g = row_graph(toks[b], length, eos)
        p = pack(g)
        canon[b, :len(p)] = [to_i64(x) for x in p]
        n[b] = len(p)
        nset[b] = len(set(p))
        strings.append(canonical_graph_string(g))
    return canon, n, nset, fold_keys(canon, n), strings


def pair_ref(toks, lens, ia, ib, eos=2):
    """(inter, da, db) of Python sets of the parsed graphs"""
    toks = np.asarray(toks)
    sets = [set(row_graph(toks[b], None if lens is None else min(int(lens[b]), toks.shape[1]), eos)) for b in range(toks.shape[0])]
    inter = np.array([len(sets[a] & sets[b]) for a, b in zip(ia, ib)], dtype=np.int32)
    da = np.array([len(sets[a]) for a in ia], dtype=np.int32)
    db = np.array([len(sets[b]) for b in ib], dtype=np.int32)
    return inter, da, db
