// Fused next-token sampler: temperature -> top-k -> nucleus -> draw (or argmax) for every row of logits[rows, V] in ONE
// launch, with no sort and no float atomics (reference distribution: kgvae/model/models.py:431-456 -- each cut is
// renormalised and the draw is made in SORTED space; here the divisions by the kept mass are folded into the targets).
//
// Order.  A row's weights w_i = exp((l_i - max l) / T) (fp32, max weight exactly 1, -inf -> 0) are read ONCE and kept on
// the CU, element i = j * TPR + t with thread t: in registers, and past 32 per thread in that thread's own LDS quads.  The contract order is descending weight, lower index first among equal
// weights; a position of that order is the pair (key, index), key = the weight's bit pattern (monotone for w >= 0).
//
// One primitive, select_mass(target, bound): the first sorted position whose cumulative mass exceeds `target`, clamped to
// the position `bound`.  It is a binary descent over the key: 30 passes, each ONE mass sum massGE(K) = sum of the weights
// with key >= K compared with the target; the mass above the final key is the last failing pass's sum, the ordinal among
// the final key's equal weights is floor((target - massGT) / w), and the index of that ordinal is a min-reduction (ordinal 0,
// the common case) or a count descent over the index (duplicated weights).  top-k is the same descent by count (exact),
// the nucleus cut is select_mass(top_p * Z_k), the draw is select_mass(u * S) bounded by the cut.
//
// Sums.  Every mass sum is formed from per-thread strided partials (<= NPT terms, added in index order), a 6-level xor
// butterfly over the wave and, in the block paths, a 4-level butterfly over the 16 wave partials that every thread
// reads from LDS in the same order: all threads hold the same bits (uniform control flow around the barriers), the tokens
// are reproducible run to run, and one sum's rounding error is at most (NPT + 10) * 2^-24 * Z.  No pass carries a residual
// into the next: each compares a fresh sum with the same target.  Error budget of a token (tests/test_sample_gpu.py):
// Z_k, the cut's descent, S, and the draw's descent are four sums, (64 + 10) * 4 = 296 at V <= 65 536, + 8 for the
// products and the tie arithmetic, + 32 for expf and its argument (ONE fp32 rounding of the fp64 quotient, |arg| <= 30):
// c = 336.
//
// Path switches (by V; `rows` never switches a path):
//   V <=    512 : one WAVE per row, 4 rows per 256-thread workgroup, 8 weights per lane, no LDS, no barrier
//   V <=   8192 : one 1024-thread workgroup per row,  8 weights per thread
//   V <=  32768 : one 1024-thread workgroup per row, 32 weights per thread
//   V <=  65536 : one 1024-thread workgroup per row, 64 weights per thread: 32 in registers, 32 in LDS (128 KB)
//   V >   65536 : ARK_ERR_SHAPE
#include "common.h"
#include "../../include/ark_amd.h"

namespace ark {

constexpr unsigned kKeyOne = 0x3F800000u;   // bits of 1.0f: the largest key of a row
constexpr int kSampBlock = 1024;

// ---- reductions: identical bits in every thread of the row's group (a wave, or the 16 waves of a block) ----------------
template <bool BLOCK, class T, class Op>
__device__ __forceinline__ T group_reduce(T v, Op op, T* part, int& flip) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  if constexpr (BLOCK) {
    T* slot = part + (flip << 4);   // two alternating sets of 16 slots: ONE barrier per reduction
    flip ^= 1;
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    v = slot[threadIdx.x & 15];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  }
  return v;
}

struct Pos { unsigned key; int idx; };   // a position of the sorted order
__device__ __forceinline__ bool pos_before(Pos a, Pos b) { return a.key > b.key || (a.key == b.key && a.idx < b.idx); }

template <int NPT, bool BLOCK>
struct RowSampler {
  static constexpr int TPR = BLOCK ? kSampBlock : 64;
  static constexpr int NR = NPT <= 32 ? NPT : 32;   // weights per thread in registers ...
  static constexpr int NL4 = (NPT - NR) / 4;        // ... and quads per thread in LDS (128 registers per thread at 1024 threads)
  float w[NR];
  f32x4* l4;   // quad g of thread t at l4[g * TPR + t]: 16 consecutive bytes per lane, read by no other thread
  int t, V, flip;
  float* pf;
  int* pi;

  __device__ __forceinline__ float rsum(float v) { return group_reduce<BLOCK>(v, [](float a, float b) { return a + b; }, pf, flip); }
  __device__ __forceinline__ float rmax(float v) { return group_reduce<BLOCK>(v, [](float a, float b) { return fmaxf(a, b); }, pf, flip); }
  __device__ __forceinline__ int isum(int v) { return group_reduce<BLOCK>(v, [](int a, int b) { return a + b; }, pi, flip); }
  __device__ __forceinline__ int imin(int v) { return group_reduce<BLOCK>(v, [](int a, int b) { return a < b ? a : b; }, pi, flip); }
  __device__ __forceinline__ int imax(int v) { return group_reduce<BLOCK>(v, [](int a, int b) { return a > b ? a : b; }, pi, flip); }

  // f(value, element index) over this thread's elements in index order; `update` stores f's result back
  template <class F>
  __device__ __forceinline__ void each(F f) {
#pragma unroll
    for (int j = 0; j < NR; ++j) f(w[j], j * TPR + t);
    if constexpr (NL4 > 0) {
#pragma unroll 2
      for (int g = 0; g < NL4; ++g) {   // (unrolled by 2 only: all 8 quads in flight at once would not fit beside w[])
        const f32x4 q = l4[g * TPR + t];
#pragma unroll
        for (int e = 0; e < 4; ++e) f(q[e], (NR + 4 * g + e) * TPR + t);
      }
    }
  }
  template <class F>
  __device__ __forceinline__ void update(F f) {
#pragma unroll
    for (int j = 0; j < NR; ++j) w[j] = f(w[j], j * TPR + t);
    if constexpr (NL4 > 0) {
#pragma unroll 2
      for (int g = 0; g < NL4; ++g) {   // (unrolled by 2 only: all 8 quads in flight at once would not fit beside w[])
        f32x4 q = l4[g * TPR + t];
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = f(q[e], (NR + 4 * g + e) * TPR + t);
        l4[g * TPR + t] = q;
      }
    }
  }

  // (keys are compared as integers: exact whatever the denormal mode; elements past V hold -1.0f, a negative integer)
  __device__ __forceinline__ float mass_ge(unsigned K) {
    float s = 0.f;
    each([&](float v, int) { s += (__float_as_int(v) >= (int)K) ? v : 0.f; });
    return rsum(s);
  }
  __device__ __forceinline__ int count_ge(unsigned K) {
    int c = 0;
    each([&](float v, int) { c += (__float_as_int(v) >= (int)K) ? 1 : 0; });
    return isum(c);
  }
  __device__ __forceinline__ int count_eq(unsigned K) {
    int c = 0;
    each([&](float v, int) { c += (__float_as_uint(v) == K) ? 1 : 0; });
    return isum(c);
  }
  // index of the m-th (0-based, index order) element whose weight has the bits K; 0x7fffffff if there is none
  __device__ __forceinline__ int tie_index(unsigned K, int m) {
    if (m == 0) {
      int best = 0x7fffffff;
      each([&](float v, int i) { if (__float_as_uint(v) == K && i < best) best = i; });
      return imin(best);
    }
    int lo = -1, hi = V - 1;   // count(idx <= lo) < m + 1 <= count(idx <= hi)
    while (hi - lo > 1) {
      const int mid = lo + ((hi - lo) >> 1);
      int c = 0;
      each([&](float v, int i) { c += (__float_as_uint(v) == K && i <= mid) ? 1 : 0; });
      if (isum(c) >= m + 1) hi = mid; else lo = mid;
    }
    return hi;
  }

  // first sorted position whose cumulative mass exceeds target, clamped to `bound` (bound.key > 0); cum = the mass up to
  // and including the returned position when it was not clamped, `cum_bound` otherwise
  __device__ __forceinline__ Pos select_mass(float target, Pos bound, float cum_bound, float& cum) {
    unsigned lo = bound.key, hi = kKeyOne + 1u;   // massGE(hi) <= target; keys below the bound's are clamped away anyway
    float m_hi = 0.f;
    while (hi - lo > 1u) {
      const unsigned mid = lo + ((hi - lo) >> 1);
      const float m = mass_ge(mid);
      if (m > target) lo = mid; else { hi = mid; m_hi = m; }
    }
    const float wk = __uint_as_float(lo);
    const float q = floorf(fmaxf(target - m_hi, 0.f) / wk);
    int m = q < 65536.f ? (int)q : 65536;
    if (m > 0) {
      const int n = count_eq(lo);
      if (m > n - 1) m = n - 1;
      if (m < 0) m = 0;
    }
    Pos p;
    p.key = lo;
    p.idx = tie_index(lo, m);
    cum = m_hi + (float)(m + 1) * wk;
    if (p.idx == 0x7fffffff || pos_before(bound, p)) { p = bound; cum = cum_bound; }
    return p;
  }

  __device__ __forceinline__ int run(const float* __restrict__ x, int sample, float T, float top_p, int top_k, float u) {
    float mx = -INFINITY;
    update([&](float, int i) {   // the logits first, the weights after
      const float l = i < V ? x[i] : -INFINITY;
      mx = fmaxf(mx, l);
      return l;
    });
    mx = rmax(mx);
    if (!sample || !(mx > -INFINITY)) {   // argmax, first index on ties (== ark_argmax_rows); a row without a finite entry
      int best = 0x7fffffff;
      each([&](float l, int i) { if (l == mx && l > -INFINITY && i < best) best = i; });
      best = imin(best);
      return (sample && best == 0x7fffffff) ? 0 : best;
    }
    const double inv_t = (T != 0.f && T != 1.f) ? 1.0 / (double)T : 1.0;
    float zp = 0.f;
    int kmin = 0x7fffffff;
    update([&](float l, int i) {
      if (i >= V) return -1.f;   // past the row's end: below every threshold, equal to no key
      const float a = (float)(((double)l - (double)mx) * inv_t);
      float v = l == mx ? 1.f : (l > -INFINITY ? fminf(expf(a), 1.f) : 0.f);
      if (!(v >= 0.f)) v = 0.f;   // NaN logits carry no mass
      zp += v;
      if (v > 0.f) kmin = min(kmin, __float_as_int(v));
      return v;
    });
    const float Z = rsum(zp);
    // last position of positive weight: the bound when no filter is active, and under a top-k that reaches into zero weights
    Pos bound;
    bound.key = (unsigned)imin(kmin);
    {
      int last = -1;
      each([&](float v, int i) { if (__float_as_uint(v) == bound.key) last = i; });
      bound.idx = imax(last);
    }
    float Zk = Z;
    if (top_k > 0 && top_k < V) {
      unsigned lo = 0u, hi = kKeyOne + 1u;   // countGE(lo) >= k > countGE(hi)
      int c_hi = 0;
      while (hi - lo > 1u) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        const int c = count_ge(mid);
        if (c >= top_k) lo = mid; else { hi = mid; c_hi = c; }
      }
      if (lo > 0u) {   // (key 0: the k-th weight is zero, every positive weight is kept)
        const int m = top_k - 1 - c_hi;
        Pos pk;
        pk.key = lo;
        pk.idx = tie_index(lo, m);
        if (pos_before(pk, bound)) {
          bound = pk;
          Zk = mass_ge(lo + 1u) + (float)(m + 1) * __uint_as_float(lo);
        }
      }
    }
    float S = Zk;
    if (top_p > 0.f && top_p < 1.f) bound = select_mass(top_p * Zk, bound, Zk, S);
    float cum;
    return select_mass(u * S, bound, S, cum).idx;
  }
};

__device__ __forceinline__ float sample_u(uint64_t seed, uint32_t draw, int row, const float* u_in, float* u_out, bool writer) {
  float u;
  if (u_in) {
    u = u_in[row];
    u = !(u > 0.f) ? 0.f : fminf(u, 1.f - 0x1p-24f);
  } else {
    const uint32_t s0 = (uint32_t)seed, s1 = (uint32_t)(seed >> 32);
    const uint32_t h = fmix32(fmix32((uint32_t)row * 0x9E3779B1u + step_hash(draw, s0, s1)) ^ s1);
    u = (float)(h >> 8) * 0x1p-24f;
  }
  if (u_out && writer) u_out[row] = u;
  return u;
}

template <int NPT, bool BLOCK>
__global__ __launch_bounds__(BLOCK ? kSampBlock : 256) void sample_rows_kernel(
    const float* __restrict__ x, long ld, int rows, int V, int sample, float T, float top_p, int top_k, uint64_t seed,
    uint32_t draw, const float* __restrict__ u_in, float* __restrict__ u_out, long forced, int64_t* __restrict__ out,
    long out_stride, int64_t* __restrict__ out2) {
  constexpr int kQuads = NPT > 32 ? (NPT - 32) / 4 * kSampBlock : 1;
  __shared__ f32x4 quads[kQuads];
  __shared__ float part_f[32];
  __shared__ int part_i[32];
  const int row = BLOCK ? (int)blockIdx.x : (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (row >= rows) return;   // (wave path only: a whole wave leaves, and that path has no barrier)
  const int t = BLOCK ? (int)threadIdx.x : (int)(threadIdx.x & 63);
  long tok;
  if (forced >= 0) {
    tok = forced;
  } else {
    const float u = sample ? sample_u(seed, draw, row, u_in, u_out, t == 0) : 0.f;
    RowSampler<NPT, BLOCK> rs;
    rs.t = t; rs.V = V; rs.flip = 0; rs.pf = part_f; rs.pi = part_i; rs.l4 = quads;
    tok = rs.run(x + (long)row * ld, sample, T, top_p, top_k, u);
  }
  if (t == 0) {
    out[(long)row * out_stride] = tok;
    if (out2) out2[row] = tok;
  }
}

}  // namespace ark

extern "C" int ark_sample_rows(const float* logits, int64_t ld, int rows, int V, int sample, float temperature, float top_p,
                               int top_k, uint64_t seed, uint32_t draw, const float* u_in, float* u_out, int64_t forced_tok,
                               int64_t* out, int64_t out_stride, int64_t* out2, void* stream) {
  using namespace ark;
  if (!logits || !out || rows <= 0 || V <= 0 || ld < V || out_stride < 1 || forced_tok >= V) return ARK_ERR_ARG;
  if (!(temperature >= 0.f) || top_p != top_p) return ARK_ERR_ARG;
  if (V > 65536) return ARK_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
#define ARK_SAMPLE_LAUNCH(NPT, BLOCK, GRID, THREADS)                                                                       \
  hipLaunchKernelGGL((sample_rows_kernel<NPT, BLOCK>), dim3(GRID), dim3(THREADS), 0, st, logits, (long)ld, rows, V, sample, \
                     temperature, top_p, top_k, seed, draw, u_in, u_out, (long)forced_tok, out, (long)out_stride, out2)
  if (V <= 512) ARK_SAMPLE_LAUNCH(8, false, (rows + 3) / 4, 256);
  else if (V <= 8192) ARK_SAMPLE_LAUNCH(8, true, rows, kSampBlock);
  else if (V <= 32768) ARK_SAMPLE_LAUNCH(32, true, rows, kSampBlock);
  else ARK_SAMPLE_LAUNCH(64, true, rows, kSampBlock);
#undef ARK_SAMPLE_LAUNCH
  ARK_LAUNCH_CHECK();
  return 0;
}
