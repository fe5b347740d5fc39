"""The memory-bound kernels that move embedding rows (ark_amd/csrc/embed.hip, the token gathers of gemm16.hip and the
t-SAIL gather / pool / broadcast-attention helpers of txf.hip) against plain CPU torch, one entry point at a time.

Gathers and 16-bit copies are checked for bit equality.  Every reduction (pool, scatter-add) is checked twice:

A. exact: values k/64 with |k| <= 256 and scales in {1, 1/2, 1/4, 1/8}: every term is a multiple of 2^-9, and while
   (items per output element) * 4 * 2^9 < 2^24 every partial sum is an fp32 number whatever order the adds land in, so
   the result must EQUAL the fp64 sum.  The precondition is asserted on the CPU: an fp32 sum in forward and in reversed
   item order both equal the fp64 sum bit for bit.  Where a pool divides by a count that is no power of two the sum is
   still exact and g = fl32(sum * fl32(1/cnt)) is one rounding of an exact product, hence still order-independent.
B. bounded: randn values, true 1/max(cnt, 1), and per element |err| <= (n + 2) * 2^-24 * sum|terms|, n = the number of
   terms that reach the element (+1 where a scale multiplies them, +1 for a value already in the destination).

The *_case functions build inputs and references on the CPU only (no GPU needed to run their precondition asserts).
"""
import ctypes

import pytest
import torch

from ark_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U = 2.0 ** -24
HP_DROP_STEP = 12            # ARK_HP_DROP_STEP of include/ark_amd.h
F16, BF16 = L.PREC_F16, L.PREC_BF16
FILL = 0.5                   # dyadic pre-fill of accumulated destinations


@pytest.fixture(autouse=True)
def _needs_gpu(cuda):
    pass


# ---------------------------------------------------------------------------------------------------------------------
# CPU helpers
def gen(seed):
    return torch.Generator().manual_seed(seed)


def dyadic(g, *shape):
    return torch.randint(-256, 257, shape, generator=g).float() / 64.0


def cast16(x, prec):
    """the library's 16-bit cast of an fp32 tensor: round to nearest even; F16 saturates at +-65504"""
    return x.clamp(-65504.0, 65504.0).half() if prec == F16 else x.bfloat16()


def dt16(prec):
    return torch.float16 if prec == F16 else torch.bfloat16


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    iv = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[a.element_size()]
    return torch.equal(a.view(iv), b.view(iv))


def pow2_below(n):
    """largest power of two <= n (n >= 1)"""
    return 1 << (int(n).bit_length() - 1)


def scatter_seq(dst0, ids, rows, dtype, reverse=False):
    """dst0[ids[i]] += rows[i], one item at a time in (reversed) item order, in `dtype`; ids < 0 are skipped"""
    out = dst0.to(dtype).clone()
    rows = rows.to(dtype)
    idl = ids.tolist()
    for i in (range(len(idl) - 1, -1, -1) if reverse else range(len(idl))):
        if idl[i] >= 0:
            out[idl[i]] += rows[i]
    return out


def scatter_ref(kind, dst0, ids, rows64, scaled):
    """reference of dst0[ids[i]] += rows[i].  exact: (fp32 result, None) after asserting the order-independence
    precondition; bounded: (fp64 result, per-element bound)"""
    ok = ids >= 0
    ref = dst0.double().clone().index_add_(0, ids[ok], rows64[ok])
    if kind == "exact":
        for rev in (False, True):
            assert torch.equal(scatter_seq(dst0, ids, rows64, torch.float32, rev).double(), ref), "inputs are not exact in fp32"
        return ref.float(), None
    sabs = dst0.double().abs().index_add_(0, ids[ok], rows64[ok].abs())
    n = torch.bincount(ids[ok], minlength=dst0.shape[0]).double() + 1 + (1 if scaled else 0)
    return ref, (n[:, None] + 2) * U * sabs


def assert_close(kind, out, ref, bound, what):
    out = out.cpu()
    if kind == "exact":
        assert torch.equal(out, ref), (what, (out.double() - ref.double()).abs().max().item())
        return
    err = (out.double() - ref).abs()
    bad = err > bound
    assert not bad.any(), (what, int(bad.sum()), err[bad].max().item(), bound[bad].min().item())


def new_hyper():
    """16 float slots holding arbitrary int32 bit patterns, the dropout draw counter at 41"""
    h = torch.arange(16, dtype=torch.int32) * 1000003 + 17
    h[HP_DROP_STEP] = 41
    d = torch.zeros(16, device=DEV)
    d.view(torch.int32).copy_(h)
    return d, h


def assert_ticks(hyper_d, before, launches):
    want = before.clone()
    want[HP_DROP_STEP] += launches
    assert torch.equal(hyper_d.view(torch.int32).cpu(), want)


def call(name, *args):
    rc = getattr(L.lib(), name)(*args, L.cur_stream())
    torch.cuda.synchronize()
    return rc


def f16_specials(W, row):
    """entries that only a saturating F16 cast survives (65520 rounds to inf under round-to-nearest-even)"""
    W[row, 0], W[row, 1], W[row, 2], W[row, 3] = 1e5, -1e5, 65520.0, -65520.0


# ---------------------------------------------------------------------------------------------------------------------
# 1 / 2. encoder pool: g[b] = sum over live triples of [E[h] | R[r] | E[t]] / max(cnt, 1)
N_ENT, N_REL = 23, 7


def graph_kinds(B, pad):
    """per graph: no padding / a padded tail / all padding / padding anywhere; a batch of two is run twice"""
    if not pad:
        return [["none"] * B]
    if B >= 3:
        return [["none", "tail", "all"] + ["mix"] * (B - 3)]
    return [["none", "tail"], ["tail", "all"]]


def pool_case(kind, B, T, D, pad, kinds, seed):
    g = gen(seed)
    pad_rid = N_REL - 1 if pad else -1
    tri = torch.stack([torch.randint(0, N_ENT, (B, T), generator=g),
                       torch.randint(0, N_REL - 1 if pad else N_REL, (B, T), generator=g),
                       torch.randint(0, N_ENT, (B, T), generator=g)], -1)
    if pad:
        for b, k in enumerate(kinds):
            live = T if k == "none" else 0 if k == "all" else pow2_below(max(T - 1, 1))   # 1 / cnt a power of two
            dead = torch.arange(live, T) if k != "mix" else torch.randperm(T, generator=g)[live:]
            tri[b, dead, 1] = pad_rid
    if kind == "exact":
        E, R = dyadic(g, N_ENT, D), dyadic(g, N_REL, D)
        E[int(tri[0, 0, 2])] = 0.0                      # an all-zero source row
    else:
        E, R = torch.randn(N_ENT, D, generator=g), torch.randn(N_REL, D, generator=g)
        if kinds[0] == "none":                          # graph 0, triple 0 is live: F16 saturation reaches g
            E[int(tri[0, 0, 0]), 0], R[int(tri[0, 0, 1]), 1], E[int(tri[0, 0, 2]), 2] = 1e5, -1e5, 65520.0
    X = torch.cat([E[tri[..., 0]], R[tri[..., 1]], E[tri[..., 2]]], -1)        # [B, T, 3D]
    live = (tri[..., 1] != pad_rid) if pad else torch.ones(B, T, dtype=torch.bool)
    cnt = live.sum(1) if pad else torch.full((B,), T)
    w = 1.0 / cnt.clamp(min=1).float()                                          # fp32 division, as the kernel's
    Xl = X * live[..., None]
    s, sabs = Xl.double().sum(1), Xl.double().abs().sum(1)
    ref = s * w.double()[:, None]
    c = dict(tri=tri, E=E, R=R, pad_rid=pad_rid, w=w, cnt=cnt, kinds=kinds, B=B, T=T, D=D, kind=kind)
    if kind == "exact":
        for order in (range(T), range(T - 1, -1, -1)):
            acc = torch.zeros(B, 3 * D)
            for t in order:
                acc = acc + Xl[:, t]
            assert torch.equal(acc.double(), s), "inputs are not exact in fp32"
        c["g"], c["bound"] = ref.float(), None          # one rounding of an exact product: order-independent
    else:
        c["g"], c["bound"] = ref, (live.sum(1).double() + 1 + 2)[:, None] * U * sabs * w.double()[:, None]
    return c


def check_pool(c, g, ic, g16a=None, pa=None, g16b=None, pb=None, what=""):
    assert_close(c["kind"], g, c["g"], c["bound"], ("g", what))
    assert torch.equal(ic.cpu(), c["w"]), ("inv_cnt", what)
    for b, k in enumerate(c["kinds"]):
        if k == "all":
            assert ic[b].item() == 1.0 and not g[b].cpu().any(), ("all-padding graph", what)
    for g16, p in ((g16a, pa), (g16b, pb)):
        if g16 is not None:
            assert same_bits(g16.cpu(), cast16(g.cpu(), p)), ("16-bit copy", p, what)


def pool_buffers(c):
    B, D = c["B"], c["D"]
    return (torch.full((B, 3 * D), 7.0, device=DEV), torch.full((B,), -1.0, device=DEV))


POOL_BODY = [(3, 1, 4), (5, 7, 12), (4, 19, 200), (2, 9, 344), (2, 8, 688)]


@pytest.mark.parametrize("kind", ["exact", "bounded"])
@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("B,T,D", POOL_BODY)
def test_enc_pool_fwd(B, T, D, pad, kind):
    """ark_enc_pool_fwd / ark_enc_pool_fwd16: one workgroup per graph, two float4 columns per thread (344 -> 258 columns: a
    second column for threads 0, 1 only; 688 -> a second trip of the 512-column loop), triples 8 at a time"""
    for n, kinds in enumerate(graph_kinds(B, pad)):
        c = pool_case(kind, B, T, D, pad, kinds, seed=100 + B * T + D + n)
        tri, E, R = c["tri"].to(DEV), c["E"].to(DEV), c["R"].to(DEV)
        g, ic = pool_buffers(c)
        rc = call("ark_enc_pool_fwd", L.ptr(tri), L.ptr(E), L.ptr(R), L.ptr(g), L.ptr(ic), L.i32(B), L.i32(T), L.i32(D),
                  L.i64(c["pad_rid"]))
        L.check(rc, "ark_enc_pool_fwd")
        check_pool(c, g, ic, what="fp32")
        for pa, pb, with_b in ((F16, BF16, True), (BF16, BF16, True), (F16, BF16, False)):
            g, ic = pool_buffers(c)
            ga = torch.zeros(B, 3 * D, device=DEV, dtype=dt16(pa))
            gb = torch.zeros(B, 3 * D, device=DEV, dtype=dt16(pb)) if with_b else None
            rc = call("ark_enc_pool_fwd16", L.ptr(tri), L.ptr(E), L.ptr(R), L.ptr(g), L.ptr(ic), L.ptr(ga), L.i32(pa), L.ptr(gb),
                      L.i32(pb), L.i32(B), L.i32(T), L.i32(D), L.i64(c["pad_rid"]))
            L.check(rc, "ark_enc_pool_fwd16")
            check_pool(c, g, ic, ga, pa, gb, pb, what=(pa, pb, with_b))
            if kind == "bounded" and T == 1 and pa == F16 and kinds[0] == "none":
                assert (g[0].abs() > 65504).any() and torch.isfinite(ga.float()).all()     # the cast did saturate


def test_enc_pool_fwd_rejects_odd_width():
    c = pool_case("exact", 2, 3, 8, False, ["none"] * 2, seed=1)
    tri, E, R = c["tri"].to(DEV), c["E"].to(DEV), c["R"].to(DEV)
    g, ic = torch.full((2, 18), 7.0, device=DEV), torch.full((2,), -1.0, device=DEV)
    ga = torch.zeros(2, 18, device=DEV, dtype=torch.float16)
    rc = call("ark_enc_pool_fwd", L.ptr(tri), L.ptr(E), L.ptr(R), L.ptr(g), L.ptr(ic), L.i32(2), L.i32(3), L.i32(6), L.i64(-1))
    assert rc < 0
    rc = call("ark_enc_pool_fwd16", L.ptr(tri), L.ptr(E), L.ptr(R), L.ptr(g), L.ptr(ic), L.ptr(ga), L.i32(F16), L.ptr(None),
              L.i32(BF16), L.i32(2), L.i32(3), L.i32(6), L.i64(-1))
    assert rc < 0
    assert (g == 7.0).all() and (ic == -1.0).all() and not ga.any()


# ---- 2. the pool and the decoder's token gather in one launch
POOL_SPLIT = [(3, 32, 64), (2, 45, 88), (2, 33, 344),     # T >= 32: 64-column workgroups x four wave quarters
              (3, 7, 12),                                   # short graphs: one workgroup per graph
              (3, 2400, 4)]                                 # the staged ids would not fit the LDS budget: one workgroup again
TOK_HALF = [(1, 4), (7, 12), (10, 128)]
VOCAB = 37


def tok_case(B, Lq, D, seed, ld_extra=1):
    """seq [B, Lq + ld_extra] with one shared token in column 0, a token table with the F16 edge values in that token's row"""
    g = gen(seed)
    seq = torch.randint(0, VOCAB, (B, Lq + ld_extra), generator=g)
    seq[0 if ld_extra == 0 else slice(None), 0] = 5
    Wt = torch.randn(VOCAB, D, generator=g)
    f16_specials(Wt, 5)
    Wp = torch.randn(Lq + 3, D, generator=g)
    ids_tm = seq[:, :Lq].t().reshape(-1)                  # row (t, b) = t * B + b
    return dict(seq=seq, Wt=Wt, Wp=Wp, ids_tm=ids_tm, x=Wt[ids_tm], xp=Wt[ids_tm] + Wp[:Lq].repeat_interleave(B, 0))


@pytest.mark.parametrize("kind", ["exact", "bounded"])
@pytest.mark.parametrize("Lq,Dd", TOK_HALF)
@pytest.mark.parametrize("B,T,D", POOL_SPLIT)
def test_pool_gather_fwd16(B, T, D, Lq, Dd, kind):
    """ark_pool_gather_fwd16: pool half on the split path (88 -> 66 columns: two live lanes in the second column block,
    T = 45 -> wave quarters 12/12/12/9) and on the one-workgroup path; token half in its three modes; the dropout tick"""
    tk = tok_case(B, Lq, Dd, seed=7 + Lq)
    seq, Wt = tk["seq"].to(DEV), tk["Wt"].to(DEV)
    hyper, before = new_hyper()
    ticks = 0
    for pad in (False, True):
        for n, kinds in enumerate(graph_kinds(B, pad)):
            c = pool_case(kind, B, T, D, pad, kinds, seed=200 + B * T + D + n)
            tri, E, R = c["tri"].to(DEV), c["E"].to(DEV), c["R"].to(DEV)
            for mode, pa, pb in (("x+tm", F16, BF16), ("x", BF16, BF16), ("tm", F16, BF16)):
                g, ic = pool_buffers(c)
                ga = torch.zeros(B, 3 * D, device=DEV, dtype=dt16(pa))
                gb = torch.zeros(B, 3 * D, device=DEV, dtype=dt16(pb))
                xa = torch.full((Lq * B, Dd), 3.0, device=DEV, dtype=dt16(pa))
                xb = torch.full((Lq * B, Dd), 3.0, device=DEV, dtype=dt16(pb))
                tm = torch.full((Lq * B,), -9, device=DEV, dtype=torch.int32)
                tick = mode != "x"
                rc = call("ark_pool_gather_fwd16", L.ptr(tri), L.ptr(E), L.ptr(R), L.ptr(g), L.ptr(ic), L.ptr(ga), L.i32(pa),
                          L.ptr(gb), L.i32(pb), L.i32(B), L.i32(T), L.i32(D), L.i64(c["pad_rid"]), L.ptr(seq), L.i64(Lq + 1),
                          L.ptr(Wt), L.ptr(xa if mode != "tm" else None), L.ptr(xb if mode != "tm" else None), L.i32(Lq),
                          L.i32(Dd), L.ptr(tm if mode != "x" else None), L.ptr(hyper if tick else None))
                L.check(rc, "ark_pool_gather_fwd16")
                ticks += 1 if tick else 0
                assert_ticks(hyper, before, ticks)
                check_pool(c, g, ic, ga, pa, gb, pb, what=(mode, pad, kinds))
                if mode == "tm":
                    assert (xa == 3.0).all() and (xb == 3.0).all()
                else:
                    assert same_bits(xa.cpu(), cast16(tk["x"], pa)) and same_bits(xb.cpu(), cast16(tk["x"], pb)), mode
                if mode == "x":
                    assert (tm == -9).all()
                else:
                    assert torch.equal(tm.cpu(), tk["ids_tm"].int()), mode


def test_pool_gather_fwd16_rejects():
    B, T, D, Lq, Dd = 2, 3, 8, 2, 8
    c = pool_case("exact", B, T, D, False, ["none"] * B, seed=2)
    tk = tok_case(B, Lq, Dd, seed=3)
    tri, E, R, seq, Wt = c["tri"].to(DEV), c["E"].to(DEV), c["R"].to(DEV), tk["seq"].to(DEV), tk["Wt"].to(DEV)
    g, ic = pool_buffers(c)
    ga, gb = torch.zeros(B, 3 * D, device=DEV, dtype=torch.float16), torch.zeros(B, 3 * D, device=DEV, dtype=torch.bfloat16)
    xa, xb = torch.zeros(Lq * B, Dd, device=DEV, dtype=torch.float16), torch.zeros(Lq * B, Dd, device=DEV, dtype=torch.bfloat16)
    tm = torch.full((Lq * B,), -9, device=DEV, dtype=torch.int32)

    def go(gb_, xa_, xb_, dd):
        return call("ark_pool_gather_fwd16", L.ptr(tri), L.ptr(E), L.ptr(R), L.ptr(g), L.ptr(ic), L.ptr(ga), L.i32(F16), L.ptr(gb_),
                    L.i32(BF16), L.i32(B), L.i32(T), L.i32(D), L.i64(-1), L.ptr(seq), L.i64(Lq + 1), L.ptr(Wt), L.ptr(xa_),
                    L.ptr(xb_), L.i32(Lq), L.i32(dd), L.ptr(tm), L.ptr(None))
    assert go(gb, None, xb, Dd) < 0          # x16b without x16a
    assert go(gb, xa, None, Dd) < 0          # g16b set while x16b is not
    assert go(gb, xa, xb, 6) < 0             # D_dec % 4
    assert (g == 7.0).all() and (tm == -9).all() and not xa.any() and not xb.any()
    assert go(gb, xa, xb, Dd) == 0           # the same arguments, accepted


# ---------------------------------------------------------------------------------------------------------------------
# 3. token gathers
TOK_SHAPES = [(1, 1, 4), (3, 7, 12), (16, 10, 512),
              (128, 33, 1024)]     # 1 081 344 float4 > 4096 blocks x 256 threads: the grid-stride loop takes a second trip


@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("B,Lq,D", TOK_SHAPES)
def test_tok_gather(B, Lq, D, with_pos):
    """ark_tok_gather: x[(t, b)] = W_tok[seq[b, t]] (+ W_pos[t]) in fp32, bit for bit; ark_tok_time_major; the tick"""
    tk = tok_case(B, Lq, D, seed=11 + B)
    seq, Wt, Wp = tk["seq"].to(DEV), tk["Wt"].to(DEV), tk["Wp"].to(DEV)
    hyper, before = new_hyper()
    x = torch.full((Lq * B, D), 7.0, device=DEV)
    for n in (1, 2):
        L.check(call("ark_tok_gather", L.ptr(seq), L.i64(Lq + 1), L.ptr(Wt), L.ptr(Wp if with_pos else None), L.ptr(x), L.i32(B),
                     L.i32(Lq), L.i32(D), L.ptr(hyper)), "ark_tok_gather")
        assert_ticks(hyper, before, n)
    assert same_bits(x.cpu(), tk["xp"] if with_pos else tk["x"])
    x2 = torch.full((Lq * B, D), 7.0, device=DEV)
    L.check(call("ark_tok_gather", L.ptr(seq), L.i64(Lq + 1), L.ptr(Wt), L.ptr(Wp if with_pos else None), L.ptr(x2), L.i32(B),
                 L.i32(Lq), L.i32(D), L.ptr(None)), "ark_tok_gather")
    assert_ticks(hyper, before, 2)
    assert same_bits(x2.cpu(), x.cpu())
    tm = torch.full((Lq * B,), -9, device=DEV, dtype=torch.int32)
    L.check(call("ark_tok_time_major", L.ptr(seq), L.i64(Lq + 1), L.ptr(tm), L.i32(B), L.i32(Lq), L.ptr(hyper)), "ark_tok_time_major")
    assert_ticks(hyper, before, 3)
    assert torch.equal(tm.cpu(), tk["ids_tm"].int())
    L.check(call("ark_tok_time_major", L.ptr(seq), L.i64(Lq + 1), L.ptr(tm), L.i32(B), L.i32(Lq), L.ptr(None)), "ark_tok_time_major")
    assert_ticks(hyper, before, 3)


@pytest.mark.parametrize("pa,pb,with_b", [(F16, BF16, True), (F16, F16, True), (BF16, BF16, True), (F16, BF16, False)])
@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("B,Lq,D", TOK_SHAPES)
def test_tok_gather16(B, Lq, D, with_pos, pa, pb, with_b):
    """ark_tok_gather16: the 16-bit casts (F16 saturating) of the fp32 row (+ position row)"""
    tk = tok_case(B, Lq, D, seed=11 + B)
    seq, Wt, Wp = tk["seq"].to(DEV), tk["Wt"].to(DEV), tk["Wp"].to(DEV)
    hyper, before = new_hyper()
    xa = torch.full((Lq * B, D), 3.0, device=DEV, dtype=dt16(pa))
    xb = torch.full((Lq * B, D), 3.0, device=DEV, dtype=dt16(pb))
    L.check(call("ark_tok_gather16", L.i32(pa), L.i32(pb), L.ptr(seq), L.i64(Lq + 1), L.ptr(Wt), L.ptr(Wp if with_pos else None),
                 L.ptr(xa), L.ptr(xb if with_b else None), L.i32(B), L.i32(Lq), L.i32(D), L.ptr(hyper)), "ark_tok_gather16")
    assert_ticks(hyper, before, 1)
    ref = tk["xp"] if with_pos else tk["x"]
    if not with_pos:
        assert (ref.abs() > 65504).any()                # the saturation is in play
    assert same_bits(xa.cpu(), cast16(ref, pa))
    if with_b:
        assert same_bits(xb.cpu(), cast16(ref, pb))
    else:
        assert (xb == 3.0).all()
    assert torch.isfinite(xa.float()).all()
    L.check(call("ark_tok_gather16", L.i32(pa), L.i32(pb), L.ptr(seq), L.i64(Lq + 1), L.ptr(Wt), L.ptr(Wp if with_pos else None),
                 L.ptr(xa), L.ptr(xb if with_b else None), L.i32(B), L.i32(Lq), L.i32(D), L.ptr(None)), "ark_tok_gather16")
    assert_ticks(hyper, before, 1)


@pytest.mark.parametrize("B,D", [(1, 4), (3, 12), (16, 512)])
def test_tok_gather_decode_form(B, D):
    """one position of a running sequence: ld_seq = 1, L = 1, w_pos pointing at row t of the position table"""
    t = 3
    tk = tok_case(B, 1, D, seed=17 + B, ld_extra=0)
    seq, Wt, Wp = tk["seq"].to(DEV), tk["Wt"].to(DEV), tk["Wp"].to(DEV)
    assert seq.shape == (B, 1) and tk["Wp"].shape[0] > t
    wp_t = ctypes.c_void_p(Wp.data_ptr() + t * D * 4)
    ref = tk["Wt"][tk["seq"][:, 0]] + tk["Wp"][t]
    x = torch.full((B, D), 7.0, device=DEV)
    L.check(call("ark_tok_gather", L.ptr(seq), L.i64(1), L.ptr(Wt), wp_t, L.ptr(x), L.i32(B), L.i32(1), L.i32(D), L.ptr(None)),
            "ark_tok_gather")
    assert same_bits(x.cpu(), ref)
    xa = torch.zeros(B, D, device=DEV, dtype=torch.float16)
    xb = torch.zeros(B, D, device=DEV, dtype=torch.bfloat16)
    L.check(call("ark_tok_gather16", L.i32(F16), L.i32(BF16), L.ptr(seq), L.i64(1), L.ptr(Wt), wp_t, L.ptr(xa), L.ptr(xb), L.i32(B),
                 L.i32(1), L.i32(D), L.ptr(None)), "ark_tok_gather16")
    assert same_bits(xa.cpu(), cast16(ref, F16)) and same_bits(xb.cpu(), cast16(ref, BF16))
    tm = torch.full((B,), -9, device=DEV, dtype=torch.int32)
    L.check(call("ark_tok_time_major", L.ptr(seq), L.i64(1), L.ptr(tm), L.i32(B), L.i32(1), L.ptr(None)), "ark_tok_time_major")
    assert torch.equal(tm.cpu(), tk["seq"][:, 0].int())


def test_tok_gather_rejects():
    tk = tok_case(2, 2, 8, seed=5)
    seq, Wt = tk["seq"].to(DEV), tk["Wt"].to(DEV)
    x = torch.full((4, 8), 7.0, device=DEV)
    xa, xb = torch.zeros(4, 8, device=DEV, dtype=torch.bfloat16), torch.zeros(4, 8, device=DEV, dtype=torch.float16)
    assert call("ark_tok_gather16", L.i32(BF16), L.i32(F16), L.ptr(seq), L.i64(3), L.ptr(Wt), L.ptr(None), L.ptr(xa), L.ptr(xb),
                L.i32(2), L.i32(2), L.i32(8), L.ptr(None)) < 0
    assert call("ark_tok_gather16", L.i32(F16), L.i32(BF16), L.ptr(seq), L.i64(3), L.ptr(Wt), L.ptr(None), L.ptr(xa), L.ptr(xb),
                L.i32(2), L.i32(2), L.i32(6), L.ptr(None)) < 0
    assert call("ark_tok_gather", L.ptr(seq), L.i64(3), L.ptr(Wt), L.ptr(None), L.ptr(x), L.i32(2), L.i32(2), L.i32(6), L.ptr(None)) < 0
    assert (x == 7.0).all() and not xa.any() and not xb.any()


# ---------------------------------------------------------------------------------------------------------------------
# 4. dW_tok[seq[b, t]] += dx[(t, b)]
def tok_scatter_case(kind, B, Lq, D, V, seed, id_hi=None):
    """ids below id_hi (default V) except id_hi // 2 and id_hi - 1, which no item refers to; column 0 one shared token;
    column Lq (never read: t < Lq) points at an unused row"""
    g = gen(seed)
    hi = id_hi or V
    seq = torch.randint(0, hi - 2, (B, Lq + 1), generator=g)
    seq += (seq >= hi // 2).long()
    seq[:, 0] = 3
    seq[:, Lq] = hi - 1
    unused = [r for r in range(V) if r == hi // 2 or r >= hi - 1]
    if kind == "exact":
        dx = dyadic(g, Lq * B, D)
        dx[1::4] = 0.0                                   # all-zero source rows
        dW0 = torch.full((V, D), FILL)
    else:
        dx, dW0 = torch.randn(Lq * B, D, generator=g), torch.randn(V, D, generator=g)
    ids = seq[:, :Lq].t().reshape(-1)
    ref, bound = scatter_ref(kind, dW0, ids, dx.double(), scaled=False)
    return dict(seq=seq, dx=dx, dW0=dW0, ref=ref, bound=bound, unused=unused, kind=kind)


def run_tok_scatter(c, B, Lq, D, V):
    seq, dx, dW = c["seq"].to(DEV), c["dx"].to(DEV), c["dW0"].to(DEV).clone()
    L.check(call("ark_tok_scatter", L.ptr(seq), L.i64(Lq + 1), L.ptr(dx), L.ptr(dW), L.i32(B), L.i32(Lq), L.i32(D), L.i32(V)),
            "ark_tok_scatter")
    out = dW.cpu()
    assert_close(c["kind"], out, c["ref"], c["bound"], "dW_tok")
    assert same_bits(out[c["unused"]], c["dW0"][c["unused"]])
    return out


TOK_SCATTER = [(4, 5, 64, 55), (16, 10, 100, 130),       # LDS tables; the second 64-column slice partly live
               (64, 40, 64, 55),                          # 54 item chunks, the last one short
               (128, 33, 1536, 55),                       # 24 slices: the 2048 / slices chunk cap
               (16, 10, 100, 192), (16, 10, 100, 193),    # last LDS size, first global size
               (8, 6, 72, 300), (4, 5, 200, 300),         # global atomics
               (128, 70, 8, 300)]                         # 8960 items > 4 x 2048 waves: the item loop takes a second trip


@pytest.mark.parametrize("kind", ["exact", "bounded"])
@pytest.mark.parametrize("B,Lq,D,V", TOK_SCATTER)
def test_tok_scatter(B, Lq, D, V, kind):
    c = tok_scatter_case(kind, B, Lq, D, V, seed=31 + B + V)
    run_tok_scatter(c, B, Lq, D, V)


def test_tok_scatter_lds_and_global_agree():
    """the same items into a table of 192 rows (privatised in LDS) and of 193 rows (global atomics): equal sums"""
    B, Lq, D = 16, 10, 100
    a = tok_scatter_case("exact", B, Lq, D, 192, seed=77, id_hi=192)
    b = tok_scatter_case("exact", B, Lq, D, 193, seed=77, id_hi=192)
    assert torch.equal(a["seq"], b["seq"]) and torch.equal(a["dx"], b["dx"])
    oa, ob = run_tok_scatter(a, B, Lq, D, 192), run_tok_scatter(b, B, Lq, D, 193)
    assert torch.equal(oa, ob[:192]) and (ob[192] == FILL).all()


# ---------------------------------------------------------------------------------------------------------------------
# 5 / 6. gradients of the triple embeddings
def triple_grad_case(kind, B, T, D, pad, n_ent, n_rel, id_ent, id_rel, seed, pooled):
    """pooled: ark_enc_pool_bwd (source row b, scaled by inv_cnt[b], triples whose relation is pad_rid masked);
    otherwise ark_triple_scatter (source row (t, b), no scale, no mask).  Entity ids < id_ent - 2, relation ids < id_rel - 2;
    id - 2 is never referred to, id - 1 is the pad id (when pad) or unused as well"""
    g = gen(seed)
    pad_eid, pad_rid = (id_ent - 1, id_rel - 1) if pad else (-1, -1)
    tri = torch.stack([torch.randint(0, id_ent - 2, (B, T), generator=g), torch.randint(0, id_rel - 2, (B, T), generator=g),
                       torch.randint(0, id_ent - 2, (B, T), generator=g)], -1)
    if pad:
        tri[..., 0][torch.rand(B, T, generator=g) < 0.2] = pad_eid
        tri[..., 2][torch.rand(B, T, generator=g) < 0.2] = pad_eid
        tri[..., 1][torch.rand(B, T, generator=g) < 0.25] = pad_rid
        tri[0, 0] = torch.tensor([pad_eid, 1, 2])       # a live triple with a pad head: relation and tail still count
        tri[0, 1] = torch.tensor([2, 1, pad_eid])
        tri[0, 2] = torch.tensor([3, pad_rid, 4])       # a padding triple with real entities
        tri[1, T // 2:, 1] = pad_rid                    # a padded tail
    h, r, tl = tri[..., 0], tri[..., 1], tri[..., 2]
    live = (r != pad_rid) if (pad and pooled) else torch.ones(B, T, dtype=torch.bool)
    if pooled:
        dg = dyadic(g, B, 3 * D) if kind == "exact" else torch.randn(B, 3 * D, generator=g)
        if kind == "exact":
            dg[1 % B] = 0.0
            ic = torch.tensor([1.0, 0.5, 0.25, 0.125])[torch.randint(0, 4, (B,), generator=g)]
        else:
            ic = 1.0 / live.sum(1).clamp(min=1).float()
        src = dg
        rows = (ic.double()[:, None] * dg.double())[:, None, :].expand(B, T, 3 * D)       # item (b, t)
    else:
        src = dyadic(g, T * B, 3 * D) if kind == "exact" else torch.randn(T * B, 3 * D, generator=g)
        if kind == "exact":
            src[2::5] = 0.0
        ic = None
        rows = src.double().view(T, B, 3 * D).transpose(0, 1)                              # item (b, t) <- row (t, b)
    rows = rows.reshape(B * T, 3 * D)
    skip = torch.full((B, T), -1)
    ids_e = torch.cat([torch.where(live & (h != pad_eid), h, skip).reshape(-1), torch.where(live & (tl != pad_eid), tl, skip).reshape(-1)])
    ids_r = torch.where(live & (r != pad_rid), r, skip).reshape(-1)
    if kind == "exact":
        dE0, dR0 = torch.full((n_ent, D), FILL), torch.full((n_rel, D), FILL)
    else:
        dE0, dR0 = torch.randn(n_ent, D, generator=g), torch.randn(n_rel, D, generator=g)
    refE, boundE = scatter_ref(kind, dE0, ids_e, torch.cat([rows[:, :D], rows[:, 2 * D:]]), scaled=pooled)
    refR, boundR = scatter_ref(kind, dR0, ids_r, rows[:, D:2 * D], scaled=pooled)
    keepE = [i for i in range(n_ent) if i >= id_ent - 2]
    keepR = [i for i in range(n_rel) if i >= id_rel - 2]
    return dict(tri=tri, src=src, ic=ic, dE0=dE0, dR0=dR0, refE=refE, refR=refR, boundE=boundE, boundR=boundR, keepE=keepE,
                keepR=keepR, pad_eid=pad_eid, pad_rid=pad_rid, kind=kind)


def check_triple_grads(c, dE, dR, what):
    dE, dR = dE.cpu(), dR.cpu()
    assert_close(c["kind"], dE, c["refE"], c["boundE"], ("dE", what))
    assert_close(c["kind"], dR, c["refR"], c["boundR"], ("dR", what))
    assert same_bits(dE[c["keepE"]], c["dE0"][c["keepE"]]), ("pad / unused entity rows", what)
    assert same_bits(dR[c["keepR"]], c["dR0"][c["keepR"]]), ("pad / unused relation rows", what)
    return dE, dR


# (n_ent, n_rel): one fused launch / fused at the 192-row limit / three launches, all LDS / entity table through global atomics
REGIMES = [(40, 9), (150, 42), (150, 43), (300, 12)]


@pytest.mark.parametrize("kind", ["exact", "bounded"])
@pytest.mark.parametrize("pad", [True, False])
@pytest.mark.parametrize("B,T,D", [(5, 7, 64), (6, 19, 100)])
def test_enc_pool_bwd(B, T, D, pad, kind):
    """ark_enc_pool_bwd in its three regimes.  exact: the same triples (ids of the smallest tables, the larger tables padded
    with unused rows) must give equal dE / dR everywhere; bounded: ids over each regime's whole tables"""
    first = None
    for n_ent, n_rel in REGIMES:
        ie, ir = (REGIMES[0] if kind == "exact" else (n_ent, n_rel))
        c = triple_grad_case(kind, B, T, D, pad, n_ent, n_rel, ie, ir, seed=300 + B + (0 if kind == "exact" else n_ent), pooled=True)
        tri, dg, ic = c["tri"].to(DEV), c["src"].to(DEV), c["ic"].to(DEV)
        dE, dR = c["dE0"].to(DEV).clone(), c["dR0"].to(DEV).clone()
        L.check(call("ark_enc_pool_bwd", L.ptr(tri), L.ptr(dg), L.ptr(ic), L.ptr(dE), L.ptr(dR), L.i32(B), L.i32(T), L.i32(D),
                     L.i32(n_ent), L.i32(n_rel), L.i64(c["pad_eid"]), L.i64(c["pad_rid"])), "ark_enc_pool_bwd")
        oE, oR = check_triple_grads(c, dE, dR, (n_ent, n_rel))
        if kind == "exact":
            if first is None:
                first = (c["tri"], oE, oR)
            else:
                assert torch.equal(c["tri"], first[0])
                assert torch.equal(oE[:REGIMES[0][0]], first[1]) and torch.equal(oR[:REGIMES[0][1]], first[2]), (n_ent, n_rel)


TRIPLE_SHAPES = [(3, 5, 16), (2, 7, 100)]       # T * B no multiple of the 4 rows of a workgroup; D > 64, no multiple of 64


@pytest.mark.parametrize("kind", ["exact", "bounded"])
@pytest.mark.parametrize("pad", [True, False])
@pytest.mark.parametrize("B,T,D", TRIPLE_SHAPES)
def test_triple_scatter(B, T, D, pad, kind):
    c = triple_grad_case(kind, B, T, D, pad, 40, 9, 40, 9, seed=400 + B, pooled=False)
    tri, dx = c["tri"].to(DEV), c["src"].to(DEV)
    dE, dR = c["dE0"].to(DEV).clone(), c["dR0"].to(DEV).clone()
    L.check(call("ark_triple_scatter", L.ptr(tri), L.ptr(dx), L.ptr(dE), L.ptr(dR), L.i32(B), L.i32(T), L.i32(D),
                 L.i64(c["pad_eid"]), L.i64(c["pad_rid"])), "ark_triple_scatter")
    check_triple_grads(c, dE, dR, "triple_scatter")


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("pad", [True, False])
@pytest.mark.parametrize("B,T,D", TRIPLE_SHAPES)
def test_triple_gather(B, T, D, pad, with_mask):
    """x[(t, b)] = [E[h] | R[r] | E[t]] of triple t of graph b, kmask[b, t] = (r != pad_rid)"""
    g = gen(500 + B)
    n_ent, n_rel = 23, 7
    pad_rid = n_rel - 1 if pad else -1
    tri = torch.stack([torch.randint(0, n_ent, (B, T), generator=g), torch.randint(0, n_rel, (B, T), generator=g),
                       torch.randint(0, n_ent, (B, T), generator=g)], -1)
    tri[0, T - 1, 1] = n_rel - 1
    E, R = torch.randn(n_ent, D, generator=g), torch.randn(n_rel, D, generator=g)
    ref = torch.cat([E[tri[..., 0]], R[tri[..., 1]], E[tri[..., 2]]], -1).transpose(0, 1).reshape(T * B, 3 * D)
    km_ref = (tri[..., 1] != pad_rid).to(torch.uint8)
    assert pad_rid < 0 or (km_ref == 0).any()
    tri_d, E_d, R_d = tri.to(DEV), E.to(DEV), R.to(DEV)
    x = torch.full((T * B, 3 * D), 7.0, device=DEV)
    km = torch.full((B, T), 9, device=DEV, dtype=torch.uint8)
    L.check(call("ark_triple_gather", L.ptr(tri_d), L.ptr(E_d), L.ptr(R_d), L.ptr(x), L.ptr(km if with_mask else None), L.i32(B),
                 L.i32(T), L.i32(D), L.i64(pad_rid)), "ark_triple_gather")
    assert same_bits(x.cpu(), ref)
    assert torch.equal(km.cpu(), km_ref if with_mask else torch.full((B, T), 9, dtype=torch.uint8))


# ---------------------------------------------------------------------------------------------------------------------
# 7. masked mean over time-major rows and its backward
def seq_pool_case(kind, B, T, W, masked, seed):
    g = gen(seed)
    x = dyadic(g, T * B, W) if kind == "exact" else torch.randn(T * B, W, generator=g)
    if kind == "exact":
        x[0] = 0.0
    if masked:
        km = torch.zeros(B, T, dtype=torch.uint8)
        for b in range(B):
            if b != 1 % B:                               # graph 1 % B stays fully masked
                km[b, torch.randperm(T, generator=g)[:pow2_below(max(T - b, 1))]] = 1
    else:
        km = torch.ones(B, T, dtype=torch.uint8)
    cnt = km.sum(1)
    w = 1.0 / cnt.clamp(min=1).float()
    xl = x.view(T, B, W) * km.t()[..., None]                                 # [T, B, W]
    s, sabs = xl.double().sum(0), xl.double().abs().sum(0)
    ref = s * w.double()[:, None]
    c = dict(x=x, km=km, w=w, cnt=cnt, kind=kind, masked=masked)
    if kind == "exact":
        for order in (range(T), range(T - 1, -1, -1)):
            acc = torch.zeros(B, W)
            for t in order:
                acc = acc + xl[t]
            assert torch.equal(acc.double(), s), "inputs are not exact in fp32"
        c["g"], c["bound"] = ref.float(), None
    else:
        c["g"], c["bound"] = ref, (cnt.double() + 1 + 2)[:, None] * U * sabs * w.double()[:, None]
    dg = dyadic(g, B, W) if kind == "exact" else torch.randn(B, W, generator=g)
    c["dg"] = dg
    c["dx"] = ((dg * w[:, None])[None] * km.t()[..., None].float()).expand(T, B, W).reshape(T * B, W)   # fp32 products
    return c


@pytest.mark.parametrize("kind", ["exact", "bounded"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,T,W", [(3, 1, 5), (2, 6, 64), (3, 11, 200),
                                   (4, 33, 4100)])      # 541 200 elements > 2048 x 256: the backward loop wraps
def test_seq_pool(B, T, W, masked, kind):
    c = seq_pool_case(kind, B, T, W, masked, seed=600 + T)
    x, km, dg = c["x"].to(DEV), c["km"].to(DEV), c["dg"].to(DEV)
    g, ic = torch.full((B, W), 7.0, device=DEV), torch.full((B,), -1.0, device=DEV)
    L.check(call("ark_seq_pool_fwd", L.ptr(x), L.ptr(km if masked else None), L.ptr(g), L.ptr(ic), L.i32(B), L.i32(T), L.i32(W)),
            "ark_seq_pool_fwd")
    assert_close(kind, g, c["g"], c["bound"], "g")
    assert torch.equal(ic.cpu(), c["w"])
    dx = torch.full((T * B, W), 7.0, device=DEV)
    L.check(call("ark_seq_pool_bwd", L.ptr(dg), L.ptr(km if masked else None), L.ptr(ic), L.ptr(dx), L.i32(B), L.i32(T), L.i32(W)),
            "ark_seq_pool_bwd")
    assert torch.equal(dx.cpu(), c["dx"])
    if masked:
        b = 1 % B
        assert c["cnt"][b] == 0 and ic[b].item() == 1.0 and not g[b].cpu().any() and not dx.view(T, B, W)[:, b].cpu().any()


# ---------------------------------------------------------------------------------------------------------------------
# 8. cross-attention over a memory of identical rows
XATTN = [(2, 3, 8, 2), (3, 70, 192, 3), (2, 6, 520, 2)]     # L > 64: a second lane trip; dh = 260, D no multiple of 64


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("B,Lq,D,H", XATTN)
def test_xattn_bcast(B, Lq, D, H, p):
    g = gen(700 + Lq)
    v, dctx = torch.randn(B, D, generator=g), torch.randn(Lq * B, D, generator=g)
    seed = 0x1234ABCD5678
    hyper, before = new_hyper()
    v_d, dctx_d = v.to(DEV), dctx.to(DEV)
    ctx, cs = torch.full((Lq * B, D), 7.0, device=DEV), torch.full((Lq * B, H), 7.0, device=DEV)
    L.check(call("ark_xattn_bcast_fwd", L.ptr(v_d), L.ptr(ctx), L.ptr(cs), L.i32(B), L.i32(Lq), L.i32(D), L.i32(H), L.f32(p),
                 L.u64(seed), L.ptr(hyper if p > 0 else None)), "ark_xattn_bcast_fwd")
    assert_ticks(hyper, before, 0)
    cs_c, ctx_c = cs.cpu(), ctx.cpu()
    head = torch.arange(D) // (D // H)
    if p == 0.0:
        assert (cs_c == 1.0).all()
        assert same_bits(ctx_c, v.repeat(Lq, 1))
    else:
        n = B * H * Lq * Lq
        assert n % 4 == 0
        mask = torch.empty(n, device=DEV)
        L.check(call("ark_dropout_mask", L.ptr(mask), L.i64(n), L.f32(p), L.u64(seed), L.ptr(hyper)), "ark_dropout_mask")
        m = mask.cpu().double().view(B, H, Lq, Lq)
        assert (m == 0).any() and (m != 0).any()
        cs_ref = m.mean(-1).permute(2, 0, 1).reshape(Lq * B, H)              # [(t, b), h]
        assert ((cs_c.double() - cs_ref).abs() <= Lq * 2.0 ** -23 * cs_ref.abs()).all()
        prod = cs_c.double()[:, head] * v.double().repeat(Lq, 1)
        assert ((ctx_c.double() - prod).abs() <= U * prod.abs()).all()      # one fp32 rounding of the product
    dv = torch.full((B, D), 7.0, device=DEV)
    L.check(call("ark_xattn_bcast_bwd", L.ptr(dctx_d), L.ptr(cs), L.ptr(dv), L.i32(B), L.i32(Lq), L.i32(D), L.i32(H)),
            "ark_xattn_bcast_bwd")
    terms = (cs_c.double()[:, head] * dctx.double()).view(Lq, B, D)
    assert_close("bounded", dv, terms.sum(0), (Lq + 1 + 2) * U * terms.abs().sum(0), "dv")


def test_xattn_bcast_rejects():
    v = torch.randn(2, 8, device=DEV)
    ctx, cs = torch.full((6, 8), 7.0, device=DEV), torch.full((6, 3), 7.0, device=DEV)
    hyper, _ = new_hyper()

    def go(H, p, hy):
        return call("ark_xattn_bcast_fwd", L.ptr(v), L.ptr(ctx), L.ptr(cs), L.i32(2), L.i32(3), L.i32(8), L.i32(H), L.f32(p),
                    L.u64(1), L.ptr(hy))
    assert go(3, 0.0, hyper) < 0             # D % H
    assert go(2, 1.0, hyper) < 0             # p = 1
    assert go(2, 0.25, None) < 0             # dropout without the draw counter
    assert call("ark_xattn_bcast_bwd", L.ptr(ctx), L.ptr(cs), L.ptr(v), L.i32(2), L.i32(3), L.i32(8), L.i32(3)) < 0
    assert (ctx == 7.0).all() and (cs == 7.0).all()
