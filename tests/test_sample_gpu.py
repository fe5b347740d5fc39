"""ark_sample_rows (ark_amd/csrc/sample.hip) through the C-ABI against the fp64 statement of its contract (tests/sample_ref.py).

Exactness bound.  A token is decided by comparing cumulative masses with two targets, top_p * Z_k and u * S; the kernel
knows a cumulative mass to within delta = C * 2^-24 * Z.  C from the kernel's own summation structure: one mass sum is a
per-thread partial of at most 64 terms (V <= 65 536 over 1024 threads) + a 6-level wave butterfly + a 4-level butterfly
over the 16 wave partials = 74 roundings; no select pass carries a residual into the next (every pass of a descent compares
a FRESH sum with the same target), so what accumulates is one sum per quantity: Z_k, the mass the nucleus descent compares,
S, and the mass the draw's descent compares = 4 * 74 = 296; + 8 for the two target products, the tie ordinal's
subtraction / division and the (m + 1) * w products; + 32 for expf and the one fp32 rounding of its argument at
|arg| <= 30.  C = 336 (the limit is 1024).

On a row where no cumulative mass lies within delta of either target (unambiguous) the kernel must return the helper's
token; on the others a token whose interval, widened by delta, contains the target under a cut that delta admits.  At
least 80 % of the rows of every case are unambiguous -- asserted here and, from the helper alone, in test_sample_cpu.py."""
import zlib

import numpy as np
import pytest
import torch

from tests.sample_ref import Row, u_hash

pytestmark = pytest.mark.gpu

C = 336
EPS24 = 2.0 ** -24
U_MAX = np.float32(1.0 - EPS24)
SETTINGS = [(0.0, 0, 1.0), (0.9, 0, 1.0), (0.0, 5, 1.3), (0.5, 7, 0.8), (0.95, 3, 1.0), (0.9, 0, 0.7)]   # (top_p, top_k, T)
# V: the issue's seven, one value each side of the kernel's path switches (512 | 513, 8192 | 8193, 32768 | 32769) and the
# largest it takes; rows 1 / 3 / 50: a single row, a ragged workgroup of the 4-rows-per-workgroup path, many workgroups
SHAPES = [(V, r) for V in (7, 64, 65, 130, 512, 513) for r in (1, 3, 50)] + [(2051, 3), (2051, 50)] + \
         [(V, 3) for V in (8192, 8193, 24101, 32768, 32769, 60943)] + [(65536, 1)]
N_HEAD = 24
# With 1 or 3 rows a single ambiguous row takes a case below 80 %: where the first draw of the input design has one, the
# next draw that has none is used (the condition itself is asserted on the CPU, tests/test_sample_cpu.py)
SALT = {(65536, 1): 1}


def t32(T):
    """the temperature the kernel receives (a C float), as the helper's double"""
    return float(np.float32(T))


def make_case(V, rows):
    """-> (logits float32 [rows, V], u float32 [rows, len(SETTINGS)]).  V <= 2051: 3 * randn; above: randn with 24 head
    tokens at 10 + 4 * rand placed at indices 0, V - 1 and 22 random others"""
    rng = np.random.default_rng(zlib.crc32(f"sample {V} {rows} {SALT.get((V, rows), 0)}".encode()))
    if V <= 2051:
        x = (3.0 * rng.standard_normal((rows, V))).astype(np.float32)
    else:
        x = rng.standard_normal((rows, V)).astype(np.float32)
        for r in range(rows):
            idx = np.concatenate([[0, V - 1], 1 + rng.choice(V - 2, N_HEAD - 2, replace=False)])
            x[r, idx] = (10.0 + 4.0 * rng.random(N_HEAD)).astype(np.float32)
    u = (rng.integers(0, 1 << 24, (rows, len(SETTINGS))).astype(np.float64) * EPS24).astype(np.float32)
    return x, u


def case_rows(V, rows):
    """per setting: [(Row, u, delta, unambiguous)] of the case, by the helper alone"""
    x, u = make_case(V, rows)
    out = []
    for s, (top_p, top_k, T) in enumerate(SETTINGS):
        per = []
        for r in range(rows):
            R = Row(x[r], t32(T), top_p, top_k)
            delta = C * EPS24 * R.Z
            per.append((R, u[r, s], delta, R.unambiguous(u[r, s], delta)))
        out.append(per)
    return out


def run(x, V, u=None, top_p=0.0, top_k=0, T=1.0, sample=True, forced=-1, stride=3, with_out2=True, seed=0, draw=0, u_out=None):
    """one launch on logits x [rows, >= V] (numpy or device tensor) -> tokens (numpy int64 [rows])"""
    from ark_amd.engine import sample_rows
    xd = torch.as_tensor(x).cuda() if not torch.is_tensor(x) else x
    rows = xd.shape[0]
    buf = torch.full((rows, stride), -7, dtype=torch.int64, device="cuda")
    out2 = torch.full((rows,), -7, dtype=torch.int64, device="cuda") if with_out2 else None
    ud = None if u is None else torch.as_tensor(np.asarray(u, dtype=np.float32)).cuda()
    sample_rows(xd, buf[:, stride - 1], V=V, sample=sample, temperature=T, top_p=top_p, top_k=top_k, seed=seed, draw=draw,
                u_in=ud, u_out=u_out, forced=forced, out2=out2)
    got = buf.cpu().numpy()
    assert (got[:, :stride - 1] == -7).all(), "the kernel wrote outside out[row * out_stride]"
    if with_out2:
        assert np.array_equal(out2.cpu().numpy(), got[:, stride - 1]), "out2 differs from out"
    return got[:, stride - 1]


def padded(x, extra=3):
    """[rows, V + extra] with large values behind every row: ld > V, and a read past V would win every draw"""
    return np.concatenate([x, np.full((x.shape[0], extra), 1e30, dtype=np.float32)], axis=1)


@pytest.mark.parametrize("V,rows", SHAPES)
def test_tokens_equal_the_fp64_statement(V, rows):
    x, _ = make_case(V, rows)
    xd = torch.as_tensor(padded(x)).cuda()
    for s, per in enumerate(case_rows(V, rows)):
        top_p, top_k, T = SETTINGS[s]
        got = run(xd, V, [c[1] for c in per], top_p, top_k, T, stride=1 + s % 3, with_out2=bool(s % 2))
        again = run(xd, V, [c[1] for c in per], top_p, top_k, T)
        assert np.array_equal(got, again), "two launches on the same inputs differ"
        share = np.mean([c[3] for c in per])
        print(f"V={V} rows={rows} (top_p, top_k, T)={SETTINGS[s]}: unambiguous share {share:.3f}")
        assert share >= 0.8
        for r, (R, u, delta, clear) in enumerate(per):
            if clear:
                assert got[r] == R.token(u), (V, rows, SETTINGS[s], r, int(got[r]), R.token(u), float(u))
            else:
                assert int(got[r]) in R.admissible(u, delta), (V, rows, SETTINGS[s], r, int(got[r]), float(u))


EDGE_V = [65, 2051, 40000]   # the wave path, a block path, the block path that keeps half of the weights in LDS


def _edge_row(V, hot, seed=0):
    """background far below (weights ~ 1e-9 of the top) with the given {index: logit} on top"""
    x = (np.random.default_rng(seed).standard_normal(V) - 20.0).astype(np.float32)
    for i, v in hot.items():
        x[i] = v
    return x


@pytest.mark.parametrize("V", EDGE_V)
def test_u_extremes(V):
    """u = 0 returns the largest weight (lowest index among equals), u = 1 - 2^-24 a kept token"""
    x, _ = make_case(V, 8)
    x[1, V - 1] = x[1, 3] = x[1].max() + 1.0   # a tie for the largest weight
    for top_p, top_k, T in SETTINGS:
        got = run(padded(x), V, np.zeros(8), top_p, top_k, T)
        assert np.array_equal(got, x.argmax(axis=1)), (top_p, top_k, T)
        got = run(padded(x), V, np.full(8, U_MAX), top_p, top_k, T)
        for r in range(8):
            assert int(got[r]) in set(Row(x[r], t32(T), top_p, top_k).kept().tolist()), (top_p, top_k, T, r)


@pytest.mark.parametrize("V", EDGE_V)
def test_equal_weights_go_to_the_lower_index_first(V):
    """duplicated logits straddling the top-k boundary and the nucleus cut: the kept duplicates are the lower indices, and
    the draw walks them in index order (u at the midpoint of every kept position's interval)"""
    dup = sorted([V - 1, 3, V // 2, 17, V - 9])
    ln2 = float(np.log(2.0))
    x = _edge_row(V, {V // 3: 2.0, **{i: 2.0 - ln2 for i in dup}})          # weights 1 and 5 x 0.5
    # cumulative masses 1, 1.5, 2, 2.5, 3, 3.5: top_p 0.55 -> target 1.925, 3 kept; 0.7 -> 2.45, 4 kept; top-k 3 (Z_k = 2) with
    # top_p 0.8 -> 1.6, the cut and the top-k boundary coincide
    for top_p, top_k, n_kept in [(0.0, 3, 3), (0.55, 0, 3), (0.7, 0, 4), (0.8, 3, 3), (0.0, 0, None)]:
        R = Row(x, 1.0, top_p, top_k)
        if n_kept is not None:
            assert R.n_p == n_kept and R.kept().tolist() == [V // 3] + dup[:n_kept - 1]
        n = min(R.n_p, 6)
        u = [R.midpoint_u(j) for j in range(n)]
        got = run(padded(np.tile(x, (n, 1))), V, u, top_p, top_k, 1.0)
        assert got.tolist() == R.order[:n].tolist(), (top_p, top_k)
        got = run(padded(x[None]), V, [U_MAX], top_p, top_k, 1.0)
        if n_kept is not None:
            assert int(got[0]) == R.kept()[-1], (top_p, top_k)   # (the last kept duplicate: its interval is 0.5 / S wide)


@pytest.mark.parametrize("V", EDGE_V)
def test_single_finite_entry_and_forced_token(V):
    x = np.full((5, V), -np.inf, dtype=np.float32)
    where = [0, V - 1, V // 2, 63, 64 % V]
    for r, i in enumerate(where):
        x[r, i] = -3.0 + r
    for top_p, top_k, T in SETTINGS:
        for u in (0.0, 0.5, float(U_MAX)):
            assert run(padded(x, 1), V, np.full(5, u), top_p, top_k, T).tolist() == where
    y, u = make_case(V, 5)
    for tok in (0, V - 1):
        assert run(padded(y), V, u[:, 0], 0.9, 5, 0.7, forced=tok).tolist() == [tok] * 5
        assert run(padded(y), V, None, sample=False, forced=tok, with_out2=False).tolist() == [tok] * 5


@pytest.mark.parametrize("V,rows", [(7, 3), (130, 50), (2051, 5), (24101, 3), (60943, 3)])
def test_greedy_is_ark_argmax_rows(V, rows):
    from ark_amd import _lib as L
    from ark_amd.engine import _call
    x, _ = make_case(V, rows)
    x = np.round(x * 2.0) / 2.0          # half-integer logits: the maximum is tied in most rows
    xd = torch.as_tensor(padded(x.astype(np.float32))).cuda()
    want = torch.full((rows,), -7, dtype=torch.int64, device="cuda")
    _call("ark_argmax_rows", L.ptr(xd), L.i64(xd.stride(0)), L.ptr(want), L.i32(rows), L.i32(V), L.cur_stream())
    got = run(xd, V, None, 0.9, 5, 0.7, sample=False)
    assert np.array_equal(got, want.cpu().numpy()) and np.array_equal(got, x.argmax(axis=1))


@pytest.mark.parametrize("V", EDGE_V)
def test_inactive_filters_are_no_ops(V):
    x, u = make_case(V, 6)
    xd = torch.as_tensor(padded(x)).cuda()
    base = run(xd, V, u[:, 0])
    for kw in [dict(top_k=V), dict(top_k=V + 5), dict(top_k=-1), dict(top_p=1.0), dict(top_p=1.5), dict(top_p=-0.1), dict(T=0.0)]:
        assert np.array_equal(run(xd, V, u[:, 0], **kw), base), kw


def test_counter_hash_equals_its_numpy_statement():
    rows = 50
    x, _ = make_case(130, rows)
    xd = torch.as_tensor(x).cuda()
    seen = set()
    for seed in (0, 2 ** 63 - 1):
        for draw in (0, 1, 636):
            u_out = torch.full((rows,), -1.0, device="cuda")
            tok = run(xd, 130, None, 0.9, 0, 1.0, seed=seed, draw=draw, u_out=u_out)
            want = u_hash(seed, draw, rows)
            got = u_out.cpu().numpy()
            assert got.tobytes() == want.tobytes(), (seed, draw)
            assert (got >= 0).all() and (got < 1).all()
            assert np.array_equal(tok, run(xd, 130, want, 0.9, 0, 1.0)), "the hash's u and the same u passed in give other tokens"
            seen.add(got.tobytes())
    assert len(seen) == 6
    assert 0.3 < float(np.mean(u_hash(12345, 7, 4096))) < 0.7


def test_argument_errors():
    from ark_amd._lib import ArkError
    x = torch.zeros(2, 16, device="cuda")
    with pytest.raises(ArkError):
        run(x, 17)                      # ld < V
    with pytest.raises(ArkError):
        run(x, 16, forced=16)           # forced token outside the vocabulary
    with pytest.raises(ArkError):
        run(x, 16, T=-1.0)
    with pytest.raises(ArkError):
        run(torch.zeros(1, 65537, device="cuda"), 65537)
