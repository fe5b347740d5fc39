"""fp64 statement of one per-latent beam step (ark_beam_step_rows, ark_amd/csrc/beam.hip) for ONE latent, and the search built
from it.  Nothing else: no shapes, no tolerances, no GPU.

    per beam j < active:  logp = l - max l - log(sum exp(l - max l));  its `beam` best entries, descending value, lower
                          index first among equal values
    candidate c = j * beam + k:  scores[j] + logp of the beam's k-th entry
    kept: the `beam` best candidates, descending score, lower c first among equal scores
    done: every kept token is EOS
"""
import numpy as np


class Step:
    """top_idx / top_logp [active, beam]; cand [active * beam] (fp64 scores); order (kept candidate indices, [beam]); tokens,
    parents, scores of the kept slots; done; gap (the smallest difference between consecutive entries of the orders that are
    cut: per beam the beam-th against the beam+1-th logit, and the kept candidates against each other and the next one;
    inf where there is nothing to cut); scale = max(1, max over the candidates of |scores[j]| + |logp|)"""


def beam_step(logits, scores, beam, active, eos):
    """logits [>= active, V] and scores [>= active] of one latent (any float type; taken as fp64)"""
    l = np.asarray(logits, dtype=np.float64)[:active]
    s = np.asarray(scores, dtype=np.float64)[:active]
    V = l.shape[1]
    assert 1 <= beam <= V and active in (1, beam)
    mx = l.max(axis=1, keepdims=True)
    logp = (l - mx) - np.log(np.exp(l - mx).sum(axis=1, keepdims=True))
    order = np.argsort(-l, axis=1, kind="stable")          # raw logits: log-softmax is monotone
    r = Step()
    r.top_idx = order[:, :beam]
    r.top_logp = np.take_along_axis(logp, r.top_idx, axis=1)
    gap = np.inf
    if V > beam:
        sl = np.take_along_axis(l, order[:, :beam + 1], axis=1)
        gap = float((sl[:, beam - 1] - sl[:, beam]).min())
    r.cand = (s[:, None] + r.top_logp).reshape(-1)
    co = np.argsort(-r.cand, kind="stable")
    r.order = co[:beam]
    cut = r.cand[co[:beam + 1]]
    if cut.size > 1:
        gap = min(gap, float((cut[:-1] - cut[1:]).min()))
    r.cand_gap = float((cut[:-1] - cut[1:]).min()) if cut.size > 1 else np.inf
    r.gap = gap
    r.parents = r.order // beam
    r.tokens = r.top_idx.reshape(-1)[r.order]
    r.scores = r.cand[r.order]
    r.done = bool((r.tokens == eos).all())
    r.scale = max(1.0, float((np.abs(s)[:, None] + np.abs(r.top_logp)).max()))
    return r


def beam_search(next_logits, beam, max_len, bos, eos):
    """one latent's own beam search, the reference's loop (kgvae/model/models.py:282-300) on a batch of one: next_logits(
    prefixes [n, t + 1] int64 numpy) -> logits [n, V] of the next position.  -> (tokens of the best beam, a list whose
    length is the sequence's; per step (gap, cand_gap, scale))"""
    seqs = np.full((1, 1), bos, dtype=np.int64)
    scores = np.zeros(1)
    margins = []
    for _ in range(max_len):
        n = seqs.shape[0]
        r = beam_step(next_logits(seqs), scores, beam, n, eos)
        margins.append((r.gap, r.cand_gap, r.scale))
        seqs = np.concatenate([seqs[r.parents], r.tokens[:, None]], axis=1)
        scores = r.scores
        if r.done:
            break
    return seqs[0].tolist(), margins
