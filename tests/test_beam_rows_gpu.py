"""Per-latent beam search on the device: ark_beam_step_rows and ark_beam_gather_rows (ark_amd/csrc/beam.hip) through the C-ABI
against the fp64 statement of their contract (tests/beam_ref.py) and torch.take_along_dim, Engine.beam_decode_rows against the
one-latent-at-a-time searches it replaces, and the latent-space walks of kgvae.experiments.interpolation on top of it.

Exactness bound of the step kernel.  The per-beam cut compares raw logits and is exact.  A candidate's score is known to
the kernel to within 92 * 2^-24 * scale, scale = max(1, max over the latent's candidates of |score_j| + |logp|), from the
kernel's own summation structure: the sum Z of a row is a per-thread partial of at most 64 terms (V <= 65 536 over 1024
threads) + a 6-level wave butterfly + a 4-level butterfly over the 16 wave partials = 74 roundings, + 2 for expf (1 ulp),
+ 12 for the one rounding of expf's argument (it moves Z by u * E_p|l - max| <= u * ln 65 536 = 11.1 u), so log Z is off by
88 u + 2 u |log Z| (logf, 1 ulp); l - max, the subtraction of log Z and the addition of the beam's score are one rounding
each: 88 + 2 |log Z| + |l - max| + |logp| + |score| <= 88 + 4 (|s_j| + |logp|) <= 92 * scale.  Two candidates are ranked
apart for certain when their scores differ by more than twice that: C = 184, delta = C * 2^-24 * scale (the limit is 1024).

A latent is unambiguous when every gap of the orders the step cuts exceeds delta (beam_ref.Step.gap).  On those the kernel
must return the helper's tokens, parents and done flag exactly and its scores to within delta; on the others the kept set
may differ by candidates whose scores lie within delta of the cut, in either order.  At least 90 % of the latents of every
case are unambiguous -- asserted from the helper alone in tests/test_beam_rows_cpu.py.

Model-level margins (oracle, CPU, asserted in tests/test_beam_rows_cpu.py): sail_tiny 1.4e-4, sail_small 3.7e-4, sail_small_pad
2.1e-4 (beam 2) / 1.3e-4 (beam 4); t-SAIL pairs below >= 1e-4; the two walks 3.1e-4 and 3.7e-4."""
import zlib

import numpy as np
import pytest
import torch

from tests.beam_ref import beam_step

pytestmark = pytest.mark.gpu

C = 184
EPS24 = 2.0 ** -24
EOS = 2
BEAMS = (1, 2, 3, 4, 8)
# V: the issue's eight and 512, the last V of the one-wave-per-latent path (512 | 513 is the kernel's only path switch);
# B 1 / 3 / 50: a single latent, a ragged workgroup of the 4-latents-per-workgroup path, many workgroups
SHAPES = [(V, B) for V in (7, 64, 65, 512, 513, 2051) for B in (1, 3, 50)] + [(V, B) for V in (8193, 24101, 60943) for B in (1, 3)]
N_HEAD = 24
PAD = 3
# With 1 or 3 latents a single ambiguous latent takes a case below 90 %: where the first draw of the input design has one,
# the next draw that has none is used (the condition itself is asserted on the CPU, tests/test_beam_rows_cpu.py)
SALT = {(65, 3, 8, 8): 1, (512, 1, 4, 4): 1, (2051, 3, 8, 8): 1}
SAIL_PAIRS = [("sail_tiny", 2), ("sail_tiny", 3), ("sail_tiny", 4), ("sail_small", 2), ("sail_small", 3), ("sail_small", 4),
              ("sail_small_pad", 2), ("sail_small_pad", 4)]
TSAIL_PAIRS = [("tsail_tiny", 4), ("tsail_small", 3), ("tsail_tiny_pad", 2)]
WALKS = [(0, 1), (2, 5)]          # straight lines dec_z[a] -> dec_z[b] of sail_small, 8 steps, beam 3
WALK_STEPS, WALK_BEAM = 8, 3


def make_case(V, B, beam, active):
    """-> (logits float32 [beam * B, V], scores float32 [beam, B], done bool [B]).  V <= 2051: 3 * randn; above: randn with 24
    head tokens at 10 + 4 * rand placed at indices 0, V - 1 and 22 random others.  Scores -6 * rand (zeros at active = 1, the
    first step).  With B >= 3 latent 1 is already done"""
    rng = np.random.default_rng(zlib.crc32(f"beam {V} {B} {beam} {active} {SALT.get((V, B, beam, active), 0)}".encode()))
    rows = beam * B
    if V <= 2051:
        x = (3.0 * rng.standard_normal((rows, V))).astype(np.float32)
    else:
        x = rng.standard_normal((rows, V)).astype(np.float32)
        for r in range(rows):
            idx = np.concatenate([[0, V - 1], 1 + rng.choice(V - 2, N_HEAD - 2, replace=False)])
            x[r, idx] = (10.0 + 4.0 * rng.random(N_HEAD)).astype(np.float32)
    s = (-6.0 * rng.random((beam, B))).astype(np.float32) if active > 1 else np.zeros((beam, B), dtype=np.float32)
    done = np.zeros(B, dtype=bool)
    if B >= 3:
        done[1] = True
    return x, s, done


def cases(V, B):
    return [(beam, active) for beam in BEAMS if beam <= V for active in sorted({1, beam})]


def case_steps(V, B, beam, active):
    """[(Step, delta, unambiguous)] of the latents of a case that are not done, by the helper alone"""
    x, s, done = make_case(V, B, beam, active)
    xl = x.reshape(beam, B, V)
    out = []
    for b in range(B):
        if done[b]:
            out.append(None)
            continue
        r = beam_step(xl[:, b], s[:, b], beam, active, EOS)
        delta = C * EPS24 * r.scale
        out.append((r, delta, r.gap > delta))
    return out


def run_step(x, s, done, beam, active, V, t=4, eos=EOS):
    """one launch -> dict of numpy outputs; x [beam * B, ld] with ld >= V"""
    from ark_amd.engine import beam_step_rows
    B = s.shape[1]
    xd = torch.as_tensor(x).cuda()
    o = {"scores": torch.as_tensor(s).cuda().clone(), "done": torch.as_tensor(done.astype(np.int32)).cuda(),
         "len": torch.full((B,), -7, dtype=torch.int32, device="cuda"),
         "tok": torch.full((beam, B), -7, dtype=torch.int64, device="cuda"),
         "nxt": torch.full((beam * B,), -7, dtype=torch.int64, device="cuda"),
         "parent": torch.full((beam, B), -7, dtype=torch.int32, device="cuda")}
    beam_step_rows(xd, o["scores"], o["done"], o["len"], o["tok"], o["nxt"], o["parent"], t, active, eos, V=V)
    return {k: v.cpu().numpy() for k, v in o.items()}


def padded(x):
    """[rows, V + PAD] with large values behind every row: ld > V, and a read past V would win every beam"""
    return np.concatenate([x, np.full((x.shape[0], PAD), 1e30, dtype=np.float32)], axis=1)


def check_latent(got, b, r, delta, clear, beam, t, what):
    tok, par, sc = got["tok"][:, b], got["parent"][:, b], got["scores"][:, b].astype(np.float64)
    assert np.array_equal(got["nxt"].reshape(beam, -1)[:, b], tok), what
    if clear:
        assert tok.tolist() == r.tokens.tolist() and par.tolist() == r.parents.tolist(), (what, tok, par, r.tokens, r.parents)
        assert np.abs(sc - r.scores).max() <= delta, (what, sc, r.scores, delta)
        assert bool(got["done"][b]) == r.done, what
    else:
        # every kept slot is one of the helper's candidates with its score, the slots descend, and no candidate left out
        # beats a kept one, all to within delta
        index = {(int(j), int(tk)): float(r.cand[j * beam + k]) for j in range(r.top_idx.shape[0]) for k, tk in enumerate(r.top_idx[j])}
        kept = [(int(p), int(k)) for p, k in zip(par, tok)]
        assert len(set(kept)) == beam and all(c in index for c in kept), (what, kept)
        assert all(abs(index[c] - v) <= delta for c, v in zip(kept, sc)), what
        assert all(sc[i] >= sc[i + 1] - delta for i in range(beam - 1)), what
        rest = [v for c, v in index.items() if c not in kept]
        assert not rest or max(rest) <= sc.min() + delta, what
        if all(k == EOS for _, k in kept):
            assert got["done"][b] == 1, what
    if got["done"][b]:
        assert got["len"][b] == t + 2, what
    else:
        assert got["len"][b] == -7, what


@pytest.mark.parametrize("V,B", SHAPES)
def test_step_equals_the_fp64_statement(V, B):
    for beam, active in cases(V, B):
        x, s, done = make_case(V, B, beam, active)
        steps = case_steps(V, B, beam, active)
        xp = padded(x)
        got = run_step(xp, s, done, beam, active, V)
        again = run_step(xp, s, done, beam, active, V)
        assert all(np.array_equal(got[k], again[k]) for k in got), "two launches on the same inputs differ"
        live = [c for c in steps if c is not None]
        share = np.mean([c[2] for c in live])
        print(f"V={V} B={B} beam={beam} active={active}: unambiguous share {share:.3f}")
        assert share >= 0.9
        for b, c in enumerate(steps):
            what = (V, B, beam, active, b)
            if c is None:      # done before the step: nothing of it is rewritten
                assert got["done"][b] == 1 and got["len"][b] == -7, what
                assert (got["tok"][:, b] == -7).all() and (got["parent"][:, b] == -7).all(), what
                assert (got["nxt"].reshape(beam, B)[:, b] == -7).all(), what
                assert got["scores"][:, b].tobytes() == s[:, b].tobytes(), what
            else:
                check_latent(got, b, c[0], c[1], c[2], beam, 4, what)


EDGE_V = [65, 513, 40000]   # the wave path, the block path, the block path with ~40 elements per thread


@pytest.mark.parametrize("V", EDGE_V)
def test_equal_logits_go_to_the_lower_index_first(V):
    """duplicated logits straddling the per-beam cut: at active = 1 the kept tokens are the duplicates of lower index, in index
    order, exactly (the cut compares raw logits); identical rows with identical scores at active = beam: the candidates tie
    bit for bit, and the lower candidate index j * beam + k goes first"""
    dup = sorted([V - 1, 3, V // 2, 17, V - 9])
    for beam in (2, 3, 4, 8):
        x = (np.random.default_rng(beam).standard_normal((beam, V)) - 20.0).astype(np.float32)
        x[:, V // 3] = 2.0
        x[:, dup] = 1.0
        n_other = max(0, beam - 6)              # beam 8: two more distinct entries below the duplicates
        for i in range(n_other):
            x[:, 40 + i] = 0.5 - 0.25 * i
        s = np.zeros((beam, 1), dtype=np.float32)
        got = run_step(padded(x), s, np.zeros(1, dtype=bool), beam, 1, V)
        want = ([V // 3] + dup + [40 + i for i in range(n_other)])[:beam]
        assert got["tok"][:, 0].tolist() == want and got["parent"][:, 0].tolist() == [0] * beam, (beam, got["tok"][:, 0])
        r = beam_step(x, s[:, 0], beam, 1, EOS)
        assert r.tokens.tolist() == want
        x[:] = x[0]                             # every beam the same row, the same score
        s[:] = -1.5
        got = run_step(padded(x), s, np.zeros(1, dtype=bool), beam, beam, V)
        r = beam_step(x, s[:, 0], beam, beam, EOS)
        assert r.tokens.tolist() == [V // 3] * beam and r.parents.tolist() == list(range(beam))
        assert got["tok"][:, 0].tolist() == r.tokens.tolist() and got["parent"][:, 0].tolist() == r.parents.tolist()
        assert len(set(got["scores"][:, 0].tolist())) == 1


@pytest.mark.parametrize("V", EDGE_V)
def test_all_kept_tokens_eos_sets_done_and_len(V):
    for beam, active in ((1, 1), (3, 3), (8, 8), (3, 1)):
        B = 3
        x, s, _ = make_case(V if V <= 2051 else 2051, B, beam, active)
        x = np.concatenate([x, np.zeros((x.shape[0], V - x.shape[1]), dtype=np.float32)], axis=1)[:, :V].copy()
        xl = x.reshape(beam, B, V)
        xl[:, 0, EOS] = 60.0                    # latent 0: EOS dominates every beam -> the kept candidates are (j, 0), all EOS
        xl[0, 2, EOS] = 60.0                    # latent 2: one beam only
        done = np.zeros(B, dtype=bool)
        got = run_step(padded(x), s, done, beam, active, V, t=6)
        for b in range(B):
            r = beam_step(xl[:, b], s[:, b], beam, active, EOS)
            assert bool(got["done"][b]) == r.done, (V, beam, active, b)
            assert got["tok"][:, b].tolist() == r.tokens.tolist(), (V, beam, active, b)
            assert got["len"][b] == (8 if r.done else -7)
        want0 = beam == 1 or active == beam     # (at active = 1 with beam > 1 only the first kept token is EOS)
        assert bool(got["done"][0]) == want0 and bool(got["done"][2]) == (beam == 1)


def test_step_argument_errors():
    from ark_amd._lib import ArkError
    x = np.zeros((16, 16), dtype=np.float32)
    ok = dict(done=np.zeros(2, dtype=bool))
    run_step(x, np.zeros((8, 2), dtype=np.float32), ok["done"], 8, 8, 16)
    with pytest.raises(ArkError):
        run_step(x, np.zeros((8, 2), dtype=np.float32), ok["done"], 8, 8, 17)             # ld < V
    with pytest.raises(ArkError):
        run_step(x[:, :4], np.zeros((8, 2), dtype=np.float32), ok["done"], 8, 8, 4)       # V < beam
    with pytest.raises(ArkError):
        run_step(np.zeros((18, 16), dtype=np.float32), np.zeros((9, 2), dtype=np.float32), ok["done"], 9, 9, 16)   # beam > 8
    with pytest.raises(ArkError):
        run_step(np.zeros((2, 65537), dtype=np.float32), np.zeros((2, 1), dtype=np.float32), np.zeros(1, dtype=bool), 2, 2, 65537)
    with pytest.raises(ArkError):
        run_step(x, np.zeros((8, 2), dtype=np.float32), ok["done"], 8, 3, 16)             # active is 1 or beam


# ---------------------------------------------------------------------------------------------------------------- reorder
def _parents(kind, beam, B, rng):
    if kind == "identity":
        p = np.tile(np.arange(beam)[:, None], (1, B))
    elif kind == "reversal":
        p = np.tile(np.arange(beam)[::-1][:, None], (1, B))
    else:                       # repeats; every third latent keeps the identity
        p = rng.integers(0, beam, (beam, B))
        p[:, ::3] = np.arange(beam)[:, None]
        p[1, -1] = p[0, -1]
    return np.ascontiguousarray(p).astype(np.int32)


@pytest.mark.parametrize("beam", [2, 3, 8])
@pytest.mark.parametrize("B", [1, 3, 50])
def test_gather_rows_equals_take_along_dim(beam, B):
    from ark_amd.engine import beam_gather_rows
    rng = np.random.default_rng(100 * beam + B)
    for width in (16, 64, 1024, 2048):
        for outer in (1, 5, 41):
            x = torch.randn(outer + 1, beam, B, width, device="cuda")      # one more outer block: must stay as it is
            for kind in ("repeats", "identity", "reversal"):
                p = torch.as_tensor(_parents(kind, beam, B, rng)).cuda()
                want = x.clone()
                want[:outer] = torch.take_along_dim(x[:outer], p.long()[None, :, :, None], 1)
                got = x.clone()
                beam_gather_rows(got[:outer], p)
                assert torch.equal(got, want), (beam, B, width, outer, kind)


def test_gather_rows_odd_width_and_errors():
    from ark_amd._lib import ArkError
    from ark_amd.engine import beam_gather_rows
    x = torch.randn(3, 3, 5, 7, device="cuda")
    p = torch.as_tensor(_parents("repeats", 3, 5, np.random.default_rng(0))).cuda()
    want = torch.take_along_dim(x, p.long()[None, :, :, None], 1)
    beam_gather_rows(x, p)
    assert torch.equal(x, want)
    with pytest.raises(ArkError):
        beam_gather_rows(torch.zeros(1, 9, 2, 4, device="cuda"), torch.zeros(9, 2, dtype=torch.int32, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------- models
_ORACLE = {}


def sail_fixture(name):
    """(cfg, trained weights, dec_z) of a SAIL golden"""
    from tests.parity_util import load_golden, weights_from
    z, cfg = load_golden(name)
    return cfg, weights_from(z, f"w{len(z['losses'])}/"), torch.from_numpy(z["dec_z"])


def oracle_rows(name, beam, zs=None, key=None):
    """O.beam_decode one latent at a time -> list of token lists; computed once per (fixture, beam, latents)"""
    from oracle import sail_oracle as O
    k = (name, beam, key)
    if k not in _ORACLE:
        cfg, W, dec_z = sail_fixture(name)
        zs = dec_z if zs is None else zs
        _ORACLE[k] = [O.beam_decode(W, zs[i:i + 1], cfg, beam)[0].tolist() for i in range(zs.shape[0])]
    return _ORACLE[k]


def _sail(name):
    from kgvae.model.models import SAIL
    cfg, W, zs = sail_fixture(name)
    model = SAIL(dict(cfg, precision="f32")).to("cuda")
    model.load_state_dict(W)
    model.eval()
    return model, cfg, zs


def _assert_rows(toks, lens, want, eos):
    toks, lens = toks.cpu(), lens.cpu().tolist()
    for i, row in enumerate(want):
        assert lens[i] == len(row), (i, lens[i], len(row))
        assert toks[i, :lens[i]].tolist() == row, (i, toks[i].tolist(), row)
        assert (toks[i, lens[i]:] == eos).all()


@pytest.mark.parametrize("name,beam", SAIL_PAIRS)
def test_sail_rows_equal_the_oracle_one_latent_at_a_time(name, beam):
    from kgvae.model.utils import seq_to_triples
    model, cfg, zs = _sail(name)
    want = oracle_rows(name, beam)
    eng = model.engine()
    st = cfg["special_tokens"]
    toks, lens = eng.beam_decode_rows(zs.cuda(), beam, max_len=cfg["seq_len"] - 1, bos=st["BOS"], eos=st["EOS"])
    assert toks.shape == (zs.shape[0], cfg["seq_len"])
    _assert_rows(toks, lens, want, st["EOS"])
    again, _ = eng.beam_decode_rows(zs.cuda(), beam, max_len=cfg["seq_len"] - 1, bos=st["BOS"], eos=st["EOS"], check_every=1)
    assert torch.equal(toks, again), "the result depends on check_every"
    tri = model.decode_latent(zs, cfg["seq_len"], st, seq_to_triples, cfg["ENT_BASE"], cfg["REL_BASE"], beam=beam, per_latent=True)
    assert tri == [seq_to_triples(torch.tensor(row), st, cfg["ENT_BASE"], cfg["REL_BASE"]) for row in want]


@pytest.mark.parametrize("name", ["sail_tiny", "sail_small"])
def test_beam_one_is_greedy_up_to_each_rows_own_stop(name):
    from kgvae.model.utils import seq_to_triples
    model, cfg, zs = _sail(name)
    eng = model.engine()
    st = cfg["special_tokens"]
    toks, lens = eng.beam_decode_rows(zs.cuda(), 1, max_len=cfg["seq_len"] - 1, bos=st["BOS"], eos=st["EOS"])
    greedy = eng.greedy_decode(zs.cuda(), max_len=cfg["seq_len"] - 1, bos=st["BOS"], eos=st["EOS"]).cpu()
    toks, lens = toks.cpu(), lens.cpu().tolist()
    for i in range(zs.shape[0]):
        n = min(lens[i], greedy.shape[1])
        assert toks[i, :n].tolist() == greedy[i, :n].tolist()
        hit = (greedy[i, 1:] == st["EOS"]).nonzero()
        assert lens[i] == (int(hit[0]) + 2 if hit.numel() else cfg["seq_len"])
    tri = model.decode_latent(zs, cfg["seq_len"], st, seq_to_triples, cfg["ENT_BASE"], cfg["REL_BASE"], beam=1, per_latent=True)
    for i in range(zs.shape[0]):
        assert [tri[i]] == model.decode_latent(zs[i:i + 1], cfg["seq_len"], st, seq_to_triples, cfg["ENT_BASE"], cfg["REL_BASE"], beam=1)


@pytest.mark.parametrize("kv_cache", [1, 0])
@pytest.mark.parametrize("name,beam", TSAIL_PAIRS)
def test_tsail_rows_equal_the_devices_one_latent_at_a_time(name, beam, kv_cache):
    from tests.test_txf_gpu import _sail_model
    model, z, cfg = _sail_model(name, ark_txf_kv_cache=kv_cache)
    model.eval()
    eng = model.engine()
    assert eng.kv_cache == bool(kv_cache)
    zs = torch.from_numpy(z["dec_z"]).cuda()
    st = cfg["special_tokens"]
    kw = dict(max_len=cfg["seq_len"] - 1, bos=st["BOS"], eos=st["EOS"])
    want = [eng.beam_decode(zs[i:i + 1], beam, **kw)[0].tolist() for i in range(zs.shape[0])]
    toks, lens = eng.beam_decode_rows(zs, beam, **kw)
    _assert_rows(toks, lens, want, st["EOS"])


def test_rows_reject_what_the_kernel_does_not_take():
    from ark_amd._lib import ArkError
    model, cfg, zs = _sail("sail_tiny")
    eng = model.engine()
    for beam in (0, 9):
        with pytest.raises(ArkError):
            eng.beam_decode_rows(zs.cuda(), beam)
    with pytest.raises(ArkError):
        eng.beam_decode_rows(zs.cuda(), 2, max_len=cfg["seq_len"])


# ---------------------------------------------------------------------------------------------------------------- walks
def walk_points(zs, a, b):
    from kgvae.experiments import interpolation as I
    return I.line_points(zs[a], zs[b] - zs[a], WALK_STEPS, 1.0 / WALK_STEPS)


@pytest.mark.parametrize("a,b", WALKS)
def test_walk_statistics_equal_the_oracles(a, b):
    from oracle import sail_oracle as O
    from kgvae.experiments import interpolation as I
    from kgvae.model.utils import seq_to_triples
    model, cfg, zs = _sail("sail_small")
    st = cfg["special_tokens"]
    pts = walk_points(zs, a, b)
    assert pts.shape == (WALK_STEPS + 1, zs.shape[1])
    rows = oracle_rows("sail_small", WALK_BEAM, pts, key=("walk", a, b))
    want = [set(tuple(map(int, t)) for t in O.seq_to_triples(row, cfg["ENT_BASE"], cfg["REL_BASE"])) for row in rows]
    got = I.decode_points(model, pts, cfg["seq_len"], st, cfg["ENT_BASE"], cfg["REL_BASE"], beam=WALK_BEAM)
    assert got == want
    flips, basins = I.flip_stats(got)
    assert (flips, basins) == I.flip_stats(want)
    assert flips == {(0, 1): 5, (2, 5): 7}[(a, b)]
    assert I.jaccard_stats(got) == I.jaccard_stats(want)
    assert got == [set(tuple(map(int, t)) for t in seq_to_triples(torch.tensor(row), st, cfg["ENT_BASE"], cfg["REL_BASE"])) for row in rows]
