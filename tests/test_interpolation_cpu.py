"""kgvae.experiments.interpolation without a GPU: a fake model whose decode_latent maps a latent to a triple set
deterministically and records its calls.  Each of the four analyses must return what a plain one-point-at-a-time restatement
of its definition returns under the same torch seed, and must decode all its points in one call (random_steps: two)."""
import torch

from kgvae.experiments import interpolation as I

Z = 6
CFG = {"seq_len": 11, "special_tokens": {"PAD": 0, "BOS": 1, "EOS": 2}, "ENT_BASE": 3, "REL_BASE": 20, "d_latent": Z}
I2E = {i: f"e{i}" for i in range(7)}
I2R = {i: f"r{i}" for i in range(4)}


def graph_of(z):
    """a coarse function of the latent: 0 to 3 triples, constant on cells of width 0.5, so walks of small steps have basins"""
    q = torch.floor(z.double() * 2.0).long().tolist()
    n = abs(q[0]) % 4
    return [(abs(q[1 + i]) % 7, abs(q[2 + i] + q[0]) % 4, abs(q[3 + i]) % 7) for i in range(n)]


class FakeModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.config = dict(CFG)
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.calls = []

    def decode_latent(self, z, seq_len, special_tokens, seq_to_triples, ent_base, rel_base, beam=4, per_latent=False):
        assert z.dim() == 2 and z.shape[1] == Z and callable(seq_to_triples)
        assert (seq_len, special_tokens, ent_base, rel_base) == (CFG["seq_len"], CFG["special_tokens"], 3, 20)
        self.calls.append((z.shape[0], beam, per_latent))
        return [graph_of(row) for row in z]


def one(z):
    return set(graph_of(z))


def unit(v):
    return v / v.norm().clamp_min(1e-12)


def test_jaccard_edge_cases():
    assert I.jaccard(set(), set()) == 1.0
    assert I.jaccard({(1, 2, 3)}, set()) == 0.0 and I.jaccard(set(), {(1, 2, 3)}) == 0.0
    assert I.jaccard({1, 2, 3}, {2, 3, 4}) == 0.5 and I.jaccard({1}, {1}) == 1.0


def test_flip_stats_trailing_basin_rule():
    a, b = {(0, 0, 0)}, {(1, 1, 1)}
    assert I.flip_stats([a, a, a]) == (0, [3])
    assert I.flip_stats([a, a, b]) == (1, [2])               # the last step flipped: the new basin is not recorded
    assert I.flip_stats([a, b, b, a, a]) == (2, [1, 2, 2])
    assert I.flip_stats([a]) == (0, [1])


def test_line_points_are_the_reference_expression():
    torch.manual_seed(0)
    z0, d = torch.randn(Z), torch.randn(Z)
    pts = I.line_points(z0, d, 5, 0.07)
    assert pts.shape == (6, Z) and torch.equal(pts[0], z0)
    for s in range(6):
        assert torch.equal(pts[s], z0 + (s * 0.07) * d)


def test_decode_to_triple_set_is_one_latent():
    m = FakeModel()
    z = torch.arange(Z, dtype=torch.float32)
    assert I.decode_to_triple_set(m, z, 11, CFG["special_tokens"], 3, 20, beam=2) == one(z)
    assert m.calls == [(1, 2, True)]


def test_flip_rate_equals_its_restatement_in_one_call():
    for steps, eps, na, nd in ((30, 0.05, 5, 4), (7, 0.3, 2, 3), (1, 0.5, 1, 1)):
        m = FakeModel()
        torch.manual_seed(11)
        got = I.latent_flip_rate_autoreg(m, steps=steps, epsilon=eps, n_anchors=na, n_dirs=nd, beam=3, device="cpu")
        assert m.calls == [(na * nd * (steps + 1), 3, True)]
        torch.manual_seed(11)
        flips = total = 0
        basins = []
        for _ in range(na):
            z0 = torch.randn(Z)
            for _ in range(nd):
                d = unit(torch.randn(Z))
                prev, run, last = one(z0), 1, False
                for s in range(1, steps + 1):
                    cur = one(z0 + (s * eps) * d)
                    total += 1
                    if cur != prev:
                        flips += 1
                        basins.append(run)
                        run, last = 1, True
                    else:
                        run, last = run + 1, False
                    prev = cur
                if not last and run > 0:
                    basins.append(run)
        assert got == (flips / max(1, total), sum(basins) / max(1, len(basins)))
        assert 0 < flips < total or steps == 1


def test_smoothness_score_equals_its_restatement_in_one_call():
    for steps, eps, na, nd in ((10, 0.1, 3, 3), (4, 0.6, 2, 1)):
        m = FakeModel()
        torch.manual_seed(5)
        got = I.latent_smoothness_score_autoreg(m, steps=steps, epsilon=eps, n_anchors=na, n_dirs=nd, beam=2, device="cpu")
        assert m.calls == [(na * nd * (steps + 1), 2, True)]
        torch.manual_seed(5)
        tl = tg = 0.0
        n = 0
        for _ in range(na):
            z0 = torch.randn(Z)
            anchor = one(z0)
            for _ in range(nd):
                d = unit(torch.randn(Z))
                prev = anchor
                for s in range(1, steps + 1):
                    cur = one(z0 + (s * eps) * d)
                    tl += I.jaccard(cur, prev)
                    tg += I.jaccard(cur, anchor)
                    n += 1
                    prev = cur
        assert got == (tl / max(1, n), tg / max(1, n))


def _labels(graph):
    return [(I2E[h], I2R[r], I2E[t]) for h, r, t in graph]


def test_line_check_equals_its_restatement_in_one_call(capsys):
    m = FakeModel()
    torch.manual_seed(3)
    got = I.smoothness_line_check_autoreg(m, I2E, I2R, steps=10, epsilon=0.2, device="cpu", beam=3)
    assert m.calls == [(11, 3, True)]
    torch.manual_seed(3)
    z0 = torch.randn(Z)
    d = unit(torch.randn(Z))
    anchor = _labels(graph_of(z0))
    prev, tl, tg = anchor, 0.0, 0.0
    for s in range(1, 11):
        g = _labels(graph_of(z0 + (s * 0.2) * d))
        tl += len(set(prev) & set(g)) / max(1, len(prev))
        tg += len(set(anchor) & set(g)) / max(1, len(anchor))
        prev = g
    assert got == (tl / 10, tg / 10)
    out = capsys.readouterr().out
    assert f"Avg local smoothness over 10 steps: {tl / 10:.2f}" in out and f"Avg global overlap over 10 steps : {tg / 10:.2f}" in out


def test_random_steps_equals_its_restatement_in_two_calls(capsys):
    m = FakeModel()
    torch.manual_seed(9)
    overlaps, denom = I.random_steps_latent_autoreg(m, I2E, I2R, n_directions=6, epsilon=1.2, device="cpu")
    assert m.calls == [(1, 3, True), (6, 3, True)]
    torch.manual_seed(9)
    z0 = torch.randn(Z)
    dirs = torch.randn(6, Z)
    dirs = dirs / dirs.norm(dim=1, keepdim=True).clamp_min(1e-12)
    ref = _labels(graph_of(z0))
    want = [len(set(ref) & set(_labels(graph_of(z0 + 1.2 * dirs[i])))) for i in range(6)]
    assert denom == max(1, len(ref)) and overlaps == want
    out = capsys.readouterr().out
    assert out.count("# Overlapping triples with z₀:") == 6
