"""The one pair of generation loops (Engine.greedy_decode / beam_decode) is written against the state protocol
decode_begin / decode_step / decode_reorder.  Here the shared beam loop runs on the CPU over a fake engine and is compared
with the list formulation of the reference's rule (models.py:282-300): per-beam candidate lists, batch-mean ranking, stable
descending sort -- which re-runs every prefix from a fresh state and never reorders one."""
import pytest
import torch

from ark_amd.engine import Engine

V, B, MAX_LEN, BOS, EOS = 7, 3, 6, 1, 2
TABLE_ROWS = 4093
SEED = 37   # (chosen on the CPU so that, for every beam > 1 and table, skipping the reorder changes the returned tokens)


class FakeEngine(Engine):
    """the three calls on the CPU: a row's logits are a row of a fixed seeded table, picked by a hash of (row within its
    block, the row's whole prefix) -- a wrong reorder changes what follows.  mode "eos3": every row puts all its mass on
    EOS at step 3; "never": EOS is never the choice; "plain": the table as it is."""

    def __init__(self, mode):
        self.mt, self.seq_len, self.device, self.mode = "SAIL", MAX_LEN + 1, torch.device("cpu"), mode
        self.table = torch.randn(TABLE_ROWS, V, generator=torch.Generator().manual_seed(SEED))
        self.reorders = []

    def decode_begin(self, rows, z=None, block=None):
        return {"prefix": [[] for _ in range(rows)], "block": block or rows}

    def decode_step(self, d, cur, t):
        out = []
        for r, (pre, tok) in enumerate(zip(d["prefix"], cur.tolist())):
            assert len(pre) == t
            pre.append(tok)
            h = r % d["block"]
            for x in pre:
                h = (h * 31 + x + 1) % TABLE_ROWS
            out.append(self.table[h])
        logits = torch.stack(out)
        if self.mode == "eos3" and t == 3:
            logits[:, EOS] += 50.0
        if self.mode == "never":
            logits[:, EOS] -= 50.0
        return logits

    def decode_reorder(self, d, j, t):
        self.reorders.append(j.tolist())
        blk = d["block"]
        d["prefix"] = [list(d["prefix"][src * blk + b]) for src in j.tolist() for b in range(blk)]


class NoReorder(FakeEngine):
    def decode_reorder(self, d, j, t):
        pass


def list_beam(eng, z, beam, max_len, bos, eos):
    """the reference's batch-shared beam, stated with lists (one fresh state per prefix, stepped through all of it)"""
    rows = z.shape[0]

    def prefix_logits(s):
        d = eng.decode_begin(rows, z)
        for t in range(s.shape[1]):
            logits = eng.decode_step(d, s[:, t], t)
        return logits

    beams = [(torch.full((rows, 1), bos, dtype=torch.int64), torch.zeros(rows))]
    for _ in range(max_len):
        cand = []
        for s, lp in beams:
            logp = torch.log_softmax(prefix_logits(s).float(), dim=-1)
            top_lp, ids = logp.topk(beam, dim=-1)
            for k in range(beam):
                cand.append((torch.cat([s, ids[:, k:k + 1]], 1), lp + top_lp[:, k]))
        means = torch.stack([c[1].mean() for c in cand])
        order = torch.sort(means, descending=True, stable=True).indices[:beam].tolist()
        beams = [cand[i] for i in order]
        if all(bool((s[:, -1] == eos).all()) for s, _ in beams):
            break
    return beams[0][0]


@pytest.mark.parametrize("beam", [1, 2, 3, 4])
@pytest.mark.parametrize("mode", ["plain", "eos3", "never"])
def test_shared_beam_loop_matches_the_list_formulation(mode, beam):
    z = torch.zeros(B, 1)
    eng = FakeEngine(mode)
    got = eng.beam_decode(z, beam, max_len=MAX_LEN, bos=BOS, eos=EOS)
    want = list_beam(FakeEngine(mode), z, beam, MAX_LEN, BOS, EOS)
    assert torch.equal(got, want), (got, want)
    if mode == "eos3":      # the early break: BOS + steps 0 .. 3
        assert got.shape == (B, 5) and bool((got[:, -1] == EOS).all())
    if mode == "never":
        assert got.shape == (B, MAX_LEN + 1) and not bool((got == EOS).any())
    if beam > 1:            # the seed makes the reorder matter: a non-identity selection that keeps one beam twice ...
        assert any(j != list(range(beam)) and len(set(j)) < beam for j in eng.reorders), eng.reorders
        stale = NoReorder(mode).beam_decode(z, beam, max_len=MAX_LEN, bos=BOS, eos=EOS)
        assert not torch.equal(stale, want)   # ... and states left in place give other tokens
