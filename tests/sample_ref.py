"""fp64 statement of the fused sampler's contract (ark_sample_rows, ark_amd/csrc/sample.hip) for one row of logits, and a
numpy restatement of its counter hash.  Nothing else: no shapes, no tolerances, no GPU.

    w_i = exp((l_i - max l) / T)            T applies when it is neither 0 nor 1; -inf -> 0;  Z = sum w
    order = stable descending order of w     (equal weights: lower index first)
    top-k (0 < k < V): the first k positions of the order, Z_k their mass
    nucleus (0 < top_p < 1): the prefix up to and including the first position whose cumulative mass exceeds top_p * Z_k,
                             S its mass
    draw: the first kept position whose cumulative mass exceeds u * S, clamped to the last kept position
"""
import numpy as np

M32 = 0xFFFFFFFF


class Row:
    """w [V], order [V], cum [n_k] (cumulative masses of the top-k kept positions, sorted order), Z, n_k, Z_k, n_p, S"""

    def __init__(self, logits, temperature=1.0, top_p=0.0, top_k=0):
        l = np.asarray(logits, dtype=np.float64)
        V = l.shape[0]
        arg = l - l.max()
        if temperature and temperature != 1.0:
            arg = arg / float(temperature)
        with np.errstate(invalid="ignore"):
            w = np.exp(arg)
        w[np.isneginf(l)] = 0.0
        self.w = w
        self.order = np.argsort(-w, kind="stable")
        self.Z = float(w.sum())
        self.n_k = int(top_k) if 0 < top_k < V else V
        self.cum = np.cumsum(w[self.order][:self.n_k])
        self.Z_k = float(self.cum[-1])
        self.top_p = float(top_p) if 0.0 < top_p < 1.0 else None
        self.n_p = self.n_k
        if self.top_p is not None:
            over = np.nonzero(self.cum > self.top_p * self.Z_k)[0]
            if over.size:
                self.n_p = int(over[0]) + 1
        self.S = float(self.cum[self.n_p - 1])

    def position(self, u):
        """sorted position drawn by u in [0, 1)"""
        over = np.nonzero(self.cum[:self.n_p] > float(u) * self.S)[0]
        return int(over[0]) if over.size else self.n_p - 1

    def token(self, u):
        return int(self.order[self.position(u)])

    def kept(self):
        """token ids of the kept set, in sorted order"""
        return self.order[:self.n_p]

    def dense(self):
        """the distribution the token is drawn from, in vocabulary order"""
        p = np.zeros_like(self.w)
        k = self.kept()
        p[k] = self.w[k] / self.S
        return p

    def midpoint_u(self, j):
        """u at the midpoint of sorted position j's interval"""
        lo = self.cum[j - 1] if j > 0 else 0.0
        return 0.5 * (lo + self.cum[j]) / self.S

    # -- what a finite-precision sampler may return: every cumulative mass known only to within delta ----------------------
    def unambiguous(self, u, delta):
        """no cumulative mass within delta of top_p * Z_k, none within delta of u * S"""
        if self.top_p is not None and np.any(np.abs(self.cum - self.top_p * self.Z_k) <= delta):
            return False
        return not np.any(np.abs(self.cum[:self.n_p] - float(u) * self.S) <= delta)

    def admissible(self, u, delta):
        """tokens whose interval, widened by delta, contains the target under any cut whose own interval, widened by delta,
        contains top_p * Z_k"""
        lower = np.concatenate([[0.0], self.cum[:-1]])
        if self.top_p is None:
            cuts = [self.n_k]
        else:
            t = self.top_p * self.Z_k
            cuts = [int(j) + 1 for j in np.nonzero((self.cum + delta > t) & (lower - delta <= t))[0]] or [self.n_p]
        ok = set()
        for n in cuts:
            t = float(u) * float(self.cum[n - 1])
            hit = np.nonzero((self.cum[:n] + delta > t) & (lower[:n] - delta <= t))[0]
            ok.update(int(self.order[j]) for j in hit)
        return ok


def fmix32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def u_hash(seed, draw, rows):
    """u of rows 0 .. rows-1 for (seed, draw): fmix32 / step_hash of csrc/common.h; 24 bits, exact in float32"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    s0, s1 = seed & M32, seed >> 32
    hs = (int(fmix32((int(fmix32((int(draw) & M32) ^ s1)) + 0x85EBCA77) & M32)) + s0) & M32
    row = np.arange(rows, dtype=np.uint64)
    h = fmix32(fmix32((row * 0x9E3779B1 + hs) & M32) ^ np.uint64(s1))
    return ((h >> 8).astype(np.float64) * 2.0 ** -24).astype(np.float32)
