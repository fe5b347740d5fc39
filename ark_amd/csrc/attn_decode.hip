// Single-query attention over a K/V cache: the self-attention of ONE new position of t-ARK / t-SAIL generation
// (TxfEngine.decode_step).  out[b, h] = softmax(q[b, h] . K[0..n_keys)[b, h]^T / sqrt(dh)) . V[0..n_keys)[b, h]: the last causal
// row of ark_attn_fwd (txf.hip), eval mode (no dropout), no probabilities array.  Exact fp32 on the vector units.
//
// The kernel is bandwidth bound (n_keys * 2 * dh floats per (b, h) against about as many FMAs), so the layout of the loads is
// the design:
//   * one 256-thread workgroup per (b, h); its four waves take interleaved blocks of keys;
//   * inside a wave a key row is read by a GROUP of G lanes (dh / 4 rounded up to a power of two, 2..64: the template
//     parameter), 16 bytes per lane, so one wave instruction covers 64 / G whole key rows, coalesced along the head dimension
//     (ark_attn_fwd maps one lane to one key: every lane walks a row of its own at a stride of 3 * D * B floats);
//   * partial dot products are summed inside the group with __shfl_xor; every lane of the group then holds the score;
//   * ONE pass: online softmax (running maximum, running sum) with the V row accumulated in the same pass under the same
//     lane -> column mapping, so every K and V byte is read once; kUnroll keys per group are in flight together and share one
//     rescale;
//   * the groups of a wave merge through __shfl_xor, the four waves through LDS, with the usual exp(m_i - m) rescale; a
//     partition that saw no key (n_keys smaller than the number of partitions) has m = -inf and weight 0, never NaN.
// Any n_keys >= 1: nothing is sized by the sequence length.  One head's keys are NOT split over several workgroups, so the
// chip is full only from B * H >= 256 on.
#include "common.h"
#include "../../include/ark_amd.h"

namespace ark {

constexpr int kDecUnroll = 4;   // keys per lane group in flight per loop trip (2 x 16 B loads each)

// exp(a - ref) with the convention that an empty partition (a = -inf) weighs 0 even when ref is -inf too
__device__ __forceinline__ float dec_ref(float m) { return m == -INFINITY ? 0.f : m; }

template <int G>
__global__ __launch_bounds__(256) void attn_decode_kernel(const float* __restrict__ q, const float* __restrict__ kv,
                                                          float* __restrict__ out, int B, int n_keys, int D, int H, int dh,
                                                          float scale) {
  constexpr int KPW = 64 / G;   // key rows per wave instruction
  __shared__ float s_acc[4][256];
  __shared__ float s_m[4], s_l[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int g = lane / G, gl = lane % G;
  const int col = gl * 4;
  const bool live = col < dh;   // (a group wider than dh / 4 has idle lanes: they load nothing and add 0 to the dot)
  const long row = 2L * D;
  const float* kbase = kv + (long)b * row + h * dh + col;
  f32x4 q4 = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    q4 = *reinterpret_cast<const f32x4*>(q + (long)b * D + h * dh + col);
    q4 *= scale;
  }
  float m = -INFINITY, l = 0.f;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  // key of (trip it, slot u, wave, group g) = ((it * kDecUnroll + u) * 4 + wave) * KPW + g; the trip count is wave-uniform
  for (int j0 = wave * KPW; j0 < n_keys; j0 += kDecUnroll * 4 * KPW) {
    f32x4 k4[kDecUnroll], v4[kDecUnroll];
    float s[kDecUnroll];
#pragma unroll
    for (int u = 0; u < kDecUnroll; ++u) {
      const int j = j0 + u * 4 * KPW + g;
      k4[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      v4[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (live && j < n_keys) {
        const float* kr = kbase + (long)j * B * row;
        k4[u] = *reinterpret_cast<const f32x4*>(kr);
        v4[u] = *reinterpret_cast<const f32x4*>(kr + D);
      }
    }
    float mx = m;
#pragma unroll
    for (int u = 0; u < kDecUnroll; ++u) {
      float a = q4[0] * k4[u][0] + q4[1] * k4[u][1] + q4[2] * k4[u][2] + q4[3] * k4[u][3];
#pragma unroll
      for (int o = G / 2; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
      s[u] = (j0 + u * 4 * KPW + g < n_keys) ? a : -INFINITY;
      mx = fmaxf(mx, s[u]);
    }
    const float ref = dec_ref(mx);
    const float c = expf(m - ref);
    l *= c;
    acc *= c;
#pragma unroll
    for (int u = 0; u < kDecUnroll; ++u) {
      const float pj = expf(s[u] - ref);
      l += pj;
      acc += pj * v4[u];
    }
    m = mx;
  }
  // the groups of this wave: butterfly over the group index
#pragma unroll
  for (int o = G; o < 64; o <<= 1) {
    const float mo = __shfl_xor(m, o, 64), lo = __shfl_xor(l, o, 64);
    f32x4 ao;
#pragma unroll
    for (int e = 0; e < 4; ++e) ao[e] = __shfl_xor(acc[e], o, 64);
    const float mx = fmaxf(m, mo), ref = dec_ref(mx);
    const float ca = expf(m - ref), cb = expf(mo - ref);
    l = l * ca + lo * cb;
    acc = acc * ca + ao * cb;
    m = mx;
  }
  if (g == 0 && live) *reinterpret_cast<f32x4*>(&s_acc[wave][col]) = acc;
  if (lane == 0) { s_m[wave] = m; s_l[wave] = l; }
  __syncthreads();
  // the four waves: thread d owns output column d of this head (wave 0 always holds key 0, so mx is finite)
  const int d = threadIdx.x;
  if (d < dh) {
    const float mx = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float c = expf(s_m[w] - mx);
      num += c * s_acc[w][d];
      den += c * s_l[w];
    }
    out[(long)b * D + h * dh + d] = num / den;
  }
}

}  // namespace ark

extern "C" int ark_attn_decode_fwd(const float* q, const float* kv, float* out, int B, int n_keys, int D, int n_heads, void* stream) {
  using namespace ark;
  if (!q || !kv || !out || B <= 0 || n_keys < 1 || D <= 0 || n_heads <= 0) return ARK_ERR_ARG;
  if (D % n_heads != 0) return ARK_ERR_SHAPE;
  const int dh = D / n_heads;
  if (dh % 4 != 0 || dh > 256) return ARK_ERR_SHAPE;
  if ((long)B * n_heads > 0x7FFFFFFFL) return ARK_ERR_SHAPE;
  if (((uintptr_t)q | (uintptr_t)kv | (uintptr_t)out) & 15) return ARK_ERR_ALIGN;
  const float scale = 1.0f / sqrtf((float)dh);
  const dim3 grid((unsigned)(B * n_heads)), block(256);
  const hipStream_t st = (hipStream_t)stream;
#define ARK_DEC_LAUNCH(G) hipLaunchKernelGGL(attn_decode_kernel<G>, grid, block, 0, st, q, kv, out, B, n_keys, D, n_heads, dh, scale)
  const int lanes = dh / 4;
  if (lanes <= 2) ARK_DEC_LAUNCH(2);
  else if (lanes <= 4) ARK_DEC_LAUNCH(4);
  else if (lanes <= 8) ARK_DEC_LAUNCH(8);
  else if (lanes <= 16) ARK_DEC_LAUNCH(16);
  else if (lanes <= 32) ARK_DEC_LAUNCH(32);
  else ARK_DEC_LAUNCH(64);
#undef ARK_DEC_LAUNCH
  ARK_LAUNCH_CHECK();
  return 0;
}
