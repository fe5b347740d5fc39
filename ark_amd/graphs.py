"""Canonical graphs on the device (csrc/graphkey.hip): what `seq_to_triples` + `canonical_graph_string` + Python sets do per
row on the host, for whole batches of token rows that stay on the device.

    canon(toks, lens, eos)        -> GraphBatch(canon, n, nset, key)      ark_graph_canon
    unique_count / unique_mask / novel_mask                                a few torch ops on the [N, 2] keys
    pair_stats(batch, ia, ib)     -> (inter, da, db) int32                 ark_graph_pair_stats
    dataset_keys(dataset, device) -> keys of a GraphSeqDataset split; dataset_canon(...) -> its GraphBatch
    nearest(queries, refs)        -> Nearest(idx, inter, dq, dr) int32     ark_graph_nearest: the reference with the largest
                                     Jaccard index per query; jaccard_tensor / nearest_summary turn it into numbers

Two rows have the same key exactly when `canonical_graph_string` of their parsed graphs is the same string (up to a 2^-128
collision of the two 64-bit folds): the key is a function of the sorted list of triples, duplicates kept.  The key's
definition is fixed (include/ark_amd.h), so keys can be stored and compared across runs.

The integer-to-number derivations (jaccard_from_counts, flip_stats_from_equal, overlap_from_counts) are plain Python on the
three integers of a pair, written so that they return bit for bit what kgvae.experiments.interpolation's jaccard /
flip_stats / jaccard_stats / overlap_stats return on the sets themselves.  This module depends on the library only, not on
an engine."""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L

GraphBatch = namedtuple("GraphBatch", "canon n nset key")

TOKEN_BITS = 21
MAX_VOCAB = 1 << TOKEN_BITS      # three tokens of a triple share one 63-bit word


def row_cap(row_len):
    """slots of a row of row_len tokens"""
    return max(0, (int(row_len) - 1) // 3)


def canon_raw(toks, lens, eos, canon_out, n_out, nset_out, key_out):
    """ark_graph_canon on the current stream into caller-owned outputs; returns the library's code (0, or ARK_ERR_*)"""
    B, row_len = toks.shape
    ld = int(toks.stride(0)) if B > 1 else row_len
    return int(L.lib().ark_graph_canon(L.ptr(toks), L.i64(ld), L.i32(B), L.i32(row_len), L.ptr(lens), L.i64(eos),
                                       L.ptr(canon_out), L.ptr(n_out), L.ptr(nset_out), L.ptr(key_out), L.cur_stream()))


def canon(toks, lens=None, eos=2, vocab=None):
    """token rows `toks` [B, row_len] (int64, on the device, unit column stride, any row stride) -> GraphBatch:
    canon [B, cap] int64 sorted packed triples then -1, n [B] int32 triples, nset [B] int32 distinct triples, key [B, 2]
    int64.  `lens` [B] (optional, what beam_decode_rows returns) cuts row b at lens[b].  `vocab`: the vocabulary the tokens
    come from, refused above 2^21 (a triple's three tokens are packed into one word)."""
    if vocab is not None and int(vocab) > MAX_VOCAB:
        raise L.ArkError(f"graph keys pack three tokens of at most {TOKEN_BITS} bits: a vocabulary of {vocab} does not fit")
    if toks.dim() != 2 or toks.dtype != torch.int64 or not toks.is_cuda:
        raise L.ArkError("canon: toks must be a [B, row_len] int64 tensor on the device")
    B, row_len = toks.shape
    if row_len < 1:
        raise L.ArkError("canon: a row holds at least its first token")
    if (row_len > 1 and toks.stride(1) != 1) or (B > 1 and toks.stride(0) < row_len):
        toks = toks.contiguous()
    cap = row_cap(row_len)
    dev = toks.device
    out = GraphBatch(torch.empty(B, cap, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
                     torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, 2, dtype=torch.int64, device=dev))
    if B == 0:
        return out
    if lens is not None:
        lens = lens.to(device=dev, dtype=torch.int64).contiguous()
        if lens.numel() != B:
            raise L.ArkError(f"canon: {lens.numel()} lengths for {B} rows")
    L.check(canon_raw(toks, lens, eos, *out), "ark_graph_canon")
    return out


def _groups(keys):
    """[N, 2] int64 -> (order, start): `order` sorts the rows by (column 0, column 1), stably; start[i] is true where
    sorted row i differs from sorted row i - 1"""
    o1 = torch.sort(keys[:, 1], stable=True).indices
    order = o1[torch.sort(keys[o1, 0], stable=True).indices]
    s = keys[order]
    start = torch.ones(s.shape[0], dtype=torch.bool, device=keys.device)
    if s.shape[0] > 1:
        start[1:] = (s[1:] != s[:-1]).any(dim=1)
    return order, start


def unique_count(batch):
    """number of distinct graphs of the batch == len({canonical_graph_string(g)})"""
    keys = batch.key if isinstance(batch, GraphBatch) else batch
    if keys.shape[0] == 0:
        return 0
    return int(_groups(keys)[1].sum())


def unique_mask(batch):
    """[N] bool: true at the FIRST row of every distinct graph"""
    keys = batch.key if isinstance(batch, GraphBatch) else batch
    mask = torch.zeros(keys.shape[0], dtype=torch.bool, device=keys.device)
    if keys.shape[0]:
        order, start = _groups(keys)     # (stable sorts: the first row of a group is its lowest row index)
        mask[order[start]] = True
    return mask


def novel_mask(batch, train_keys):
    """[N] bool: true where the row's graph is not among the graphs `train_keys` [M, 2] were made from"""
    keys = batch.key if isinstance(batch, GraphBatch) else batch
    N, M = keys.shape[0], train_keys.shape[0]
    if N == 0 or M == 0:
        return torch.ones(N, dtype=torch.bool, device=keys.device)
    order, start = _groups(torch.cat([train_keys.to(keys.device), keys]))
    gid = torch.empty(M + N, dtype=torch.int64, device=keys.device)
    gid[order] = torch.cumsum(start.to(torch.int64), 0) - 1
    seen = torch.zeros(M + N, dtype=torch.bool, device=keys.device)
    seen[gid[:M]] = True
    return ~seen[gid[M:]]


def pair_stats(batch, ia, ib):
    """for every pair q of rows (ia[q], ib[q]) of the batch: (inter, da, db) int32 [P] on the device -- distinct triples
    common to both graphs, distinct triples of either.  ark_graph_pair_stats, one wave per pair."""
    dev = batch.canon.device
    ia = torch.as_tensor(ia, device=dev).to(torch.int32).contiguous()
    ib = torch.as_tensor(ib, device=dev).to(torch.int32).contiguous()
    P, rows = ia.numel(), batch.n.numel()
    if ib.numel() != P:
        raise L.ArkError("pair_stats: ia and ib differ in length")
    out = tuple(torch.empty(P, dtype=torch.int32, device=dev) for _ in range(3))
    if P == 0:
        return out
    if rows == 0 or int(torch.min(ia.min(), ib.min())) < 0 or int(torch.max(ia.max(), ib.max())) >= rows:
        raise L.ArkError(f"pair_stats: a row index outside 0 .. {rows - 1}")
    c = batch.canon.contiguous()
    L.check(L.lib().ark_graph_pair_stats(L.ptr(c), L.ptr(batch.n), L.i32(rows), L.i32(c.shape[1]), L.ptr(ia), L.ptr(ib), L.i32(P),
                                         L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), L.cur_stream()), "ark_graph_pair_stats")
    return out


# ------------------------------------------------------------------------------------------- from the integers to the numbers
def sets_equal(inter, da, db):
    return inter == da == db


def jaccard_from_counts(inter, da, db):
    """interpolation.jaccard(a, b) from |a & b|, |a|, |b|"""
    if da == 0 and db == 0:
        return 1.0
    if da == 0 or db == 0:
        return 0.0
    return inter / (da + db - inter)


def flip_stats_from_equal(equal):
    """interpolation.flip_stats(sets) from equal[s] = (sets[s + 1] == sets[s])"""
    flips, basins, run, last_flip = 0, [], 1, False
    for same in equal:
        if not same:
            flips += 1
            basins.append(run)
            run, last_flip = 1, True
        else:
            run, last_flip = run + 1, False
    if not last_flip and run > 0:
        basins.append(run)
    return flips, basins


def jaccard_stats_from_counts(prev, anchor):
    """interpolation.jaccard_stats(sets) from per step (inter, d_step, d_previous) and (inter, d_step, d_anchor)"""
    return [(jaccard_from_counts(*p), jaccard_from_counts(*a)) for p, a in zip(prev, anchor)]


def overlap_from_counts(inter_prev, n_prev, inter_anchor, n_anchor):
    """one step of interpolation.overlap_stats: the denominators are the LIST lengths n of the previous graph / the anchor"""
    return inter_prev / max(1, n_prev), inter_anchor / max(1, n_anchor)


def walk_pairs(n_walks, steps):
    """row indices of the pairs of n_walks walks of steps + 1 consecutive rows each, walk by walk, step by step:
    (step, previous) then (step, anchor) -> (ia, ib) of length 2 * n_walks * steps: the first half are the consecutive pairs"""
    w = np.arange(n_walks)[:, None] * (steps + 1)
    s = np.arange(1, steps + 1)[None, :]
    cur = (w + s).reshape(-1)
    return np.concatenate([cur, cur]), np.concatenate([cur - 1, np.broadcast_to(w, (n_walks, steps)).reshape(-1)])


# ------------------------------------------------------------------------------------------- rows of a dataset split
def dataset_rows(dataset, indices=None):
    """(rows [N, W] int64, lens [N] int64) as numpy: row i = [BOS, (ENT_BASE + h, REL_BASE + r, ENT_BASE + t) per stored
    triple of graph i in its stored order, EOS, PAD ...] == triples_to_seq(dataset.graphs[i], ...), W = dataset.seq_len (or
    the longest graph's 3 T + 2 without one); lens = 3 T + 2.  Built from the split's stored triples: no permutation is
    drawn and no generator is touched (tensorize() and __getitem__ redraw the per-epoch permutations)."""
    base, ln = dataset._base_arrays()
    if indices is not None:
        idx = np.asarray(indices, dtype=np.int64)
        base, ln = base[idx], ln[idx]
    n, T = base.shape[0], base.shape[1]
    st = dataset.special_tokens
    tmax = int(ln.max()) if n else 0
    W = int(dataset.seq_len) if dataset.seq_len is not None else 3 * tmax + 2
    if 3 * tmax + 2 > W:
        raise ValueError(f"a graph of {tmax} triples does not fit a sequence of {W} tokens")
    rows = np.full((n, W), st["PAD"], dtype=np.int64)
    rows[:, 0] = st["BOS"]
    keep = min(T, (W - 1) // 3)
    body = (base[:, :keep] + np.array([dataset.ent_base, dataset.rel_base, dataset.ent_base], dtype=np.int64)).reshape(n, 3 * keep)
    valid = np.arange(3 * keep)[None, :] < (3 * ln)[:, None]
    rows[:, 1:1 + 3 * keep] = np.where(valid, body, st["PAD"])
    rows[np.arange(n), 1 + 3 * ln] = st["EOS"]
    return rows, 3 * ln + 2


def dataset_keys(dataset, device, chunk=16384):
    """keys [N, 2] of the graphs of a GraphSeqDataset split, on `device`"""
    n = len(dataset)
    eos = dataset.special_tokens["EOS"]
    out = []
    for i0 in range(0, n, chunk):
        rows, lens = dataset_rows(dataset, np.arange(i0, min(n, i0 + chunk)))
        vocab = int(rows.max()) + 1
        out.append(canon(torch.from_numpy(rows).to(device), torch.from_numpy(lens).to(device), eos=eos, vocab=vocab).key)
    return torch.cat(out) if out else torch.empty(0, 2, dtype=torch.int64, device=device)


def dataset_canon(dataset, device, chunk=16384):
    """GraphBatch of the graphs of a GraphSeqDataset split, on `device`: the sibling of dataset_keys that keeps the sorted
    lists (what `nearest` compares against).  Built from dataset_rows: no permutation is drawn and no generator is touched.
    Chunks whose rows differ in width are padded with -1 to one cap."""
    n = len(dataset)
    eos = dataset.special_tokens["EOS"]
    parts = []
    for i0 in range(0, n, chunk):
        rows, lens = dataset_rows(dataset, np.arange(i0, min(n, i0 + chunk)))
        vocab = int(rows.max()) + 1
        parts.append(canon(torch.from_numpy(rows).to(device), torch.from_numpy(lens).to(device), eos=eos, vocab=vocab))
    if not parts:
        return GraphBatch(torch.empty(0, 0, dtype=torch.int64, device=device), torch.empty(0, dtype=torch.int32, device=device),
                          torch.empty(0, dtype=torch.int32, device=device), torch.empty(0, 2, dtype=torch.int64, device=device))
    cap = max(p.canon.shape[1] for p in parts)
    lists = [p.canon if p.canon.shape[1] == cap else torch.nn.functional.pad(p.canon, (0, cap - p.canon.shape[1]), value=-1)
             for p in parts]
    return GraphBatch(torch.cat(lists), torch.cat([p.n for p in parts]), torch.cat([p.nset for p in parts]),
                      torch.cat([p.key for p in parts]))


# ------------------------------------------------------------------------------------------- the nearest graph of another batch
Nearest = namedtuple("Nearest", "idx inter dq dr")


def nearest_raw(queries, refs, exclude_self, strips, idx, inter, dq, dr):
    """ark_graph_nearest on the current stream into caller-owned outputs (its scratch is allocated here); returns the
    library's code (0, or ARK_ERR_*)"""
    qc, rc = queries.canon.contiguous(), refs.canon.contiguous()
    qn, rn = queries.n.contiguous(), refs.n.contiguous()
    NQ, NR, capq, capr = qc.shape[0], rc.shape[0], qc.shape[1], rc.shape[1]
    size = L.lib().ark_graph_nearest_scratch_bytes
    size.restype = ctypes.c_long
    nbytes = int(size(L.i32(NQ), L.i32(NR), L.i32(capq), L.i32(capr), L.i32(strips)))
    scratch = torch.empty(nbytes // 4, dtype=torch.int32, device=qc.device) if nbytes else None
    return int(L.lib().ark_graph_nearest(L.ptr(qc), L.ptr(qn), L.i32(NQ), L.i32(capq), L.ptr(rc), L.ptr(rn), L.i32(NR),
                                         L.i32(capr), L.i32(1 if exclude_self else 0), L.i32(strips), L.ptr(idx), L.ptr(inter),
                                         L.ptr(dq), L.ptr(dr), L.ptr(scratch), L.i64(nbytes), L.cur_stream()))


def nearest(queries, refs, exclude_self=False, strips=0):
    """for every graph of `queries` the graph of `refs` (two GraphBatches on one device; their caps may differ) with the
    largest Jaccard index over the sets of distinct triples -> Nearest(idx, inter, dq, dr), int32 [NQ] on the device:
    the reference's row (the lowest among equally near ones), |Q & R|, |Q|, |R|.  J follows jaccard_from_counts: 1 for two
    empty graphs, 0 when exactly one is empty; fractions are compared exactly.  exclude_self: row q of `refs` is skipped
    for query q (a batch against itself).  A query without an admissible reference gets idx = inter = dr = -1.  `strips`
    forces the split of the reference axis (0: chosen by the library); the result does not depend on it."""
    dev = queries.canon.device
    NQ = int(queries.n.numel())
    if max(queries.canon.shape[1], refs.canon.shape[1]) > 1024:
        raise L.ArkError("nearest: a graph list holds at most 1024 triples")
    if refs.canon.device != dev:
        raise L.ArkError("nearest: queries and references live on different devices")
    out = Nearest(*(torch.empty(NQ, dtype=torch.int32, device=dev) for _ in range(4)))
    if NQ == 0:
        return out
    L.check(nearest_raw(queries, refs, exclude_self, strips, *out), "ark_graph_nearest")
    return out


def jaccard_tensor(near):
    """float64 [NQ] on the device: jaccard_from_counts of every row of a Nearest; NaN where idx == -1"""
    inter, dq, dr = near.inter.double(), near.dq.double(), near.dr.double()
    union = dq + dr - inter
    j = torch.where(union == 0, torch.ones_like(union), inter / union.clamp(min=1.0))
    return torch.where(near.idx < 0, torch.full_like(j, float("nan")), j)


def nearest_summary(near):
    """the statistics of a Nearest (one host read): {"n": rows with a nearest reference, "mean_jaccard": their mean J (NaN
    without any), "hist": 11 counts, "copied": hist[10], "copied_rate": copied / n}.  The bin of a row is computed on the
    integers: 10 when J = 1, else (10 * inter) // (dq + dr - inter), so bin b < 10 holds b / 10 <= J < (b + 1) / 10.
    `copied` counts SET equality of the distinct triples; key equality (novel_mask) also tells duplicate triples apart, so a
    generated graph that repeats a triple of a training graph is copied here and novel there."""
    ok = near.idx >= 0
    inter, dq, dr = near.inter.long(), near.dq.long(), near.dr.long()
    union = dq + dr - inter
    bins = torch.where(union == 0, torch.full_like(union, 10), (10 * inter) // union.clamp(min=1))
    hist = torch.bincount(bins[ok], minlength=11)[:11].double()
    j = jaccard_tensor(near)
    vals = torch.cat([ok.sum().double().view(1), torch.where(ok, j, torch.zeros_like(j)).sum().view(1), hist]).tolist()
    n = int(vals[0])
    hist = [int(v) for v in vals[2:]]
    return {"n": n, "mean_jaccard": vals[1] / n if n else float("nan"), "hist": hist, "copied": hist[10],
            "copied_rate": hist[10] / max(1, n)}


def summary(batch, train_keys=None, train_graphs=None, diversity=False):
    """the statistics of a batch of generated graphs.  With `train_graphs` (a GraphBatch, e.g. dataset_canon(train split)) also
    how near the batch is to it: nearest_train_jaccard (the mean J of every graph's nearest training graph),
    nearest_train_hist (11 bins of it) and copied_rate (nearest_summary); with `diversity` nearest_other_jaccard, the mean J
    of every graph's nearest OTHER graph of the batch."""
    N = int(batch.n.numel())
    uniq = unique_count(batch)
    head = torch.stack([(batch.n == 0).sum().double(), batch.n.double().sum()])
    if train_keys is not None:
        head = torch.cat([head, novel_mask(batch, train_keys).sum().double().view(1)])
    vals = head.tolist()
    out = {"n": N, "unique": uniq, "unique_rate": uniq / max(1, N)}
    if train_keys is not None:
        out["novel"] = int(vals[2])
        out["novel_rate"] = int(vals[2]) / max(1, N)
    out["empty"] = int(vals[0])
    out["mean_triples"] = vals[1] / max(1, N)
    if train_graphs is not None:
        ns = nearest_summary(nearest(batch, train_graphs))
        out["nearest_train_jaccard"] = ns["mean_jaccard"]
        out["nearest_train_hist"] = ns["hist"]
        out["copied_rate"] = ns["copied_rate"]
    if diversity:
        out["nearest_other_jaccard"] = nearest_summary(nearest(batch, batch, exclude_self=True))["mean_jaccard"]
    return out
