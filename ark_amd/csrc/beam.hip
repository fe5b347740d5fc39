// Per-latent beam search: ONE beam step for every latent of a batch in one launch (ark_beam_step_rows), and the state
// reorder that follows it (ark_beam_gather_rows).  The reference's beam (kgvae/model/models.py:282-300) is shared by the
// whole batch and ranks candidates by the batch-MEAN log-probability; run on a batch of ONE latent it is that latent's own
// beam search, and that is what every latent b gets here: B independent B = 1 searches, no host round trip per token.
//
// Step.  logits[beam * B, ld]: row j * B + b is beam j of latent b.  For latent b and each beam j < active:
//   logp = (l - max l) - log(sum exp(l - max l));  the beam's `beam` best entries in descending value, lower index first
//   among equal values (== ark_argmax_rows);  candidate c = j * beam + k has score scores[j, b] + logp_k.
// The `beam` best candidates in descending score, lower c first among equal scores (the reference's stable descending
// sort), fill the slots i = 0 .. beam - 1: token -> tok_out[i, b] and nxt[i * B + b], parent j -> parent_out[i, b], score
// -> scores[i, b] (in place: a latent's scores are read before its first barrier and written after its last).  All kept
// tokens == eos: done[b] = 1, len[b] = t + 2.  A latent with done[b] set is left alone: nothing of it is read or written.
//
// Order without a sort.  An entry is the 64-bit key (monotone image of the value's bits) << 32 | ~index: larger key = earlier
// in the contract order, no two entries of a row share a key (-0 counts as +0).  Each thread streams its strided
// elements ONCE keeping its own 8 largest keys in registers (a compare against the 8th, rarely an insertion); the row's
// k-th entry is then the max-reduction of the threads' heads, popped by its owner, `beam` times.  The raw logits are
// compared, so the per-beam cut is EXACT.  The row maximum is the first entry.  A second pass over the row (L2) sums
// exp(l - max).  Nothing logits-sized is written.
//
// Sums.  Per-thread strided partials (<= 64 terms at V <= 65 536, added in index order), a 6-level xor butterfly over the wave and, in
// the block path, a 4-level butterfly over the 16 wave partials that every thread reads from LDS in the same order: all
// threads hold the same bits, no float atomics, the same inputs give the same outputs on every run.
// Error budget of one candidate score, in units of u = 2^-24 (tests/test_beam_rows_gpu.py):  the sum Z carries 64 + 10 =
// 74 roundings at V <= 65 536, + 2 for expf (1 ulp), + 12 for the one rounding of expf's argument (u * E_p|l - max| <=
// u * ln V <= 11.1 u of Z): log Z is off by 88 u + 2 u |log Z| (logf, 1 ulp); (l - max), the subtraction of log Z and the
// addition of the beam's score are one rounding each: 88 + 2 |log Z| + |l - max| + |logp| + |score| <= 88 + 4 (|s_j| + |logp|)
// <= 92 * scale with scale = max(1, max over the latent's candidates of |s_j| + |logp|).  Two candidates are ranked
// apart when their scores differ by more than twice that: C = 184, delta = C * 2^-24 * scale.
//
// Path switches (by V; B, beam and active never switch a path):
//   V <=   512 : one WAVE per latent, 4 latents per 256-thread workgroup, <= 8 elements per lane, no LDS, no barrier
//   V <= 65536 : one 1024-thread workgroup per latent, <= 64 elements per thread, one barrier per reduction
//   V >  65536, beam outside 1 .. 8, V < beam : ARK_ERR_SHAPE, nothing is launched
#include "common.h"
#include "../../include/ark_amd.h"

namespace ark {

constexpr int kBeamBlock = 1024;
constexpr int kBeamMax = 8;

template <bool BLOCK, class T, class Op>
__device__ __forceinline__ T beam_reduce(T v, Op op, T* part, int& flip) {
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

__device__ __forceinline__ unsigned long long beam_key(float v, int idx) {
  v += 0.0f;   // -0 -> +0: equal values, one key order
  const unsigned u = __float_as_uint(v);
  const unsigned ord = u ^ (((int)u >> 31) | 0x80000000u);
  return ((unsigned long long)ord << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)idx);
}
__device__ __forceinline__ float beam_key_value(unsigned long long k) {
  const unsigned ord = (unsigned)(k >> 32);
  return __uint_as_float(ord ^ ((ord >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}
__device__ __forceinline__ int beam_key_index(unsigned long long k) { return (int)(0xFFFFFFFFu - (unsigned)k); }

template <bool BLOCK>
__global__ __launch_bounds__(BLOCK ? kBeamBlock : 256) void beam_step_kernel(
    const float* __restrict__ x, long ld, int B, int V, int beam, int active, int eos, int t, float* __restrict__ scores,
    int* __restrict__ done, int* __restrict__ len, int64_t* __restrict__ tok_out, int64_t* __restrict__ nxt,
    int* __restrict__ parent_out) {
  typedef unsigned long long u64;
  constexpr int TPR = BLOCK ? kBeamBlock : 64;
  __shared__ float part_f[32];
  __shared__ u64 part_k[32];
  const int b = BLOCK ? (int)blockIdx.x : (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (b >= B) return;         // (wave path only: a whole wave leaves, and that path has no barrier)
  if (done[b]) return;        // uniform over the latent's group
  const int tid = BLOCK ? (int)threadIdx.x : (int)(threadIdx.x & 63);
  const int lane = (int)(threadIdx.x & 63);
  const int n_cand = active * beam;            // <= 64: candidate c lives in lane c
  const int my_j = lane / beam, my_k = lane - my_j * beam;
  const float my_s = lane < n_cand ? scores[(long)my_j * B + b] : 0.f;
  float my_val = 0.f, my_cand = 0.f;
  int my_tok = 0, flip = 0;

  for (int j = 0; j < active; ++j) {
    const float* __restrict__ row = x + ((long)j * B + b) * ld;
    u64 top[kBeamMax];
#pragma unroll
    for (int i = 0; i < kBeamMax; ++i) top[i] = 0ull;
    for (int i = tid; i < V; i += TPR) {
      const u64 k = beam_key(row[i], i);
      if (k > top[kBeamMax - 1]) {
        top[kBeamMax - 1] = k;
#pragma unroll
        for (int s = kBeamMax - 1; s > 0; --s) {
          const u64 hi = top[s] > top[s - 1] ? top[s] : top[s - 1];
          const u64 lo = top[s] > top[s - 1] ? top[s - 1] : top[s];
          top[s - 1] = hi;
          top[s] = lo;
        }
      }
    }
    float mx = 0.f;
#pragma unroll
    for (int r = 0; r < kBeamMax; ++r) {
      if (r < beam) {   // uniform
        const u64 best = beam_reduce<BLOCK>(top[0], [](u64 a, u64 c) { return a > c ? a : c; }, part_k, flip);
        if (top[0] == best) {   // its owner pops it (keys of real entries are unique)
#pragma unroll
          for (int s = 0; s < kBeamMax - 1; ++s) top[s] = top[s + 1];
          top[kBeamMax - 1] = 0ull;
        }
        const float v = beam_key_value(best);
        if (r == 0) mx = v;
        if (my_j == j && my_k == r) {
          my_val = v;
          my_tok = beam_key_index(best);
        }
      }
    }
    float zp = 0.f;
    for (int i = tid; i < V; i += TPR) zp += expf(row[i] - mx);
    const float Z = beam_reduce<BLOCK>(zp, [](float a, float c) { return a + c; }, part_f, flip);
    if (my_j == j) my_cand = my_s + ((my_val - mx) - logf(Z));
  }

  if (BLOCK && threadIdx.x >= 64) return;   // (no barrier from here on)
  int rank = 0;
  for (int c = 0; c < n_cand; ++c) {
    const float o = __shfl(my_cand, c, 64);
    rank += (o > my_cand || (o == my_cand && c < lane)) ? 1 : 0;
  }
  const bool kept = lane < n_cand && rank < beam;
  if ((unsigned)my_tok >= (unsigned)V) my_tok = 0;   // (only a row without `beam` ordered entries gets here)
  if (kept) {
    const long o = (long)rank * B + b;
    tok_out[o] = my_tok;
    nxt[o] = my_tok;
    parent_out[o] = my_j;
    scores[o] = my_cand;
  }
  const unsigned long long ended = __ballot(kept && my_tok == eos);
  if (lane == 0 && __popcll(ended) == beam) {
    done[b] = 1;
    len[b] = t + 2;
  }
}

// x[o, i, b, :] = x[o, parent[i, b], b, :] in place: one thread owns column group c of all NB rows of (o, b) and reads them
// before it writes; a latent whose parents are the identity is not touched.  (NB is a template parameter: with a run-time
// beam the 8-row register file of the general case cost 210 registers per thread.)
template <class T, int NB>
__global__ __launch_bounds__(256) void beam_gather_kernel(T* __restrict__ x, const int* __restrict__ parent, long total, int B,
                                                           int W) {
  const long id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= total) return;
  const int c = (int)(id % W);
  const long ob = id / W;
  const int b = (int)(ob % B);
  const long o = ob / B;
  int p[NB];
  bool ident = true;
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int q = parent[(long)i * B + b];
    p[i] = (unsigned)q < (unsigned)NB ? q : i;
    ident = ident && p[i] == i;
  }
  if (ident) return;
  const long rs = (long)B * W;
  T* base = x + (o * NB * B + b) * (long)W + c;
  T v[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) v[i] = base[p[i] * rs];
#pragma unroll
  for (int i = 0; i < NB; ++i) base[i * rs] = v[i];
}

template <class T>
static int beam_gather_launch(T* x, const int* parent, long total, int beam, int B, int W, hipStream_t st) {
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  switch (beam) {
#define ARK_BEAM_GATHER(NB) \
  case NB: hipLaunchKernelGGL((beam_gather_kernel<T, NB>), grid, block, 0, st, x, parent, total, B, W); break;
    ARK_BEAM_GATHER(2) ARK_BEAM_GATHER(3) ARK_BEAM_GATHER(4) ARK_BEAM_GATHER(5) ARK_BEAM_GATHER(6) ARK_BEAM_GATHER(7)
    ARK_BEAM_GATHER(8)
#undef ARK_BEAM_GATHER
    default: return ARK_ERR_SHAPE;
  }
  ARK_LAUNCH_CHECK();
  return 0;
}

}  // namespace ark

extern "C" int ark_beam_step_rows(const float* logits, int64_t ld, int B, int V, int beam, int active, int eos, int t,
                                  float* scores, int* done, int* len, int64_t* tok_out, int64_t* nxt, int* parent_out,
                                  void* stream) {
  using namespace ark;
  if (!logits || !scores || !done || !len || !tok_out || !nxt || !parent_out || B <= 0 || V <= 0 || ld < V || t < 0)
    return ARK_ERR_ARG;
  if (beam < 1 || beam > kBeamMax || V > 65536 || V < beam) return ARK_ERR_SHAPE;
  if (active != 1 && active != beam) return ARK_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (V <= 512)
    hipLaunchKernelGGL((beam_step_kernel<false>), dim3((B + 3) / 4), dim3(256), 0, st, logits, (long)ld, B, V, beam, active, eos,
                       t, scores, done, len, tok_out, nxt, parent_out);
  else
    hipLaunchKernelGGL((beam_step_kernel<true>), dim3(B), dim3(kBeamBlock), 0, st, logits, (long)ld, B, V, beam, active, eos, t,
                       scores, done, len, tok_out, nxt, parent_out);
  ARK_LAUNCH_CHECK();
  return 0;
}

extern "C" int ark_beam_gather_rows(float* x, const int* parent, int64_t outer, int beam, int B, int64_t width, void* stream) {
  using namespace ark;
  if (!x || !parent || outer <= 0 || B <= 0 || width <= 0) return ARK_ERR_ARG;
  if (beam < 1 || beam > kBeamMax) return ARK_ERR_SHAPE;
  if (beam == 1) return 0;   // one beam: its parent is itself
  hipStream_t st = (hipStream_t)stream;
  const bool vec = width % 4 == 0 && ((uintptr_t)x & 15) == 0;
  const long W = vec ? width / 4 : width;
  if (W > 0x7FFFFFFFL || outer > 0x7FFFFFFFL) return ARK_ERR_SHAPE;
  const long total = (long)outer * B * W;
  if ((total + 255) / 256 > 0x7FFFFFFFL) return ARK_ERR_SHAPE;
  if (vec) return beam_gather_launch(reinterpret_cast<f32x4*>(x), parent, total, beam, B, (int)W, st);
  return beam_gather_launch(x, parent, total, beam, B, (int)W, st);
}
