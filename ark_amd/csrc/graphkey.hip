// Canonical graphs on the device: token rows -> sorted packed triples + a 128-bit order-independent key (ark_graph_canon), and
// set statistics of pairs of canonical graphs (ark_graph_pair_stats).  What kgvae.model.utils does per row in the
// interpreter -- seq_to_triples, then str(sorted(graph)) into a Python set -- for every row of a batch in one launch.
//
// Parse (== seq_to_triples).  Row b has len = row_len, or min(max(lens[b], 0), row_len) when lens is given.  Position 0 is
// skipped; slot s covers positions 1 + 3s .. 3 + 3s and is COMPLETE when 3 + 3s < len.  The list ends in front of the first
// slot that is not complete or whose FIRST token is eos; an eos at the second or third position of a slot is an ordinary
// token.  n = number of slots in the list (<= cap = (row_len - 1) / 3).
//
// Pack.  p = tok0 << 42 | tok1 << 21 | tok2 of the RAW tokens (unsigned 64-bit arithmetic).  With every token below 2^21 the
// fields do not overlap and p < 2^63; h = tok0 - ENT_BASE, r = tok1 - REL_BASE, t = tok2 - ENT_BASE are monotone, so ascending
// p is the order of sorted(graph) on (h, r, t).  The filler is ~0 (-1 as int64): as an unsigned value it is above every p,
// the all-ones triple (2^63 - 1) included, so the list sorts in front of it.
//
// Key.  mix = the splitmix64 finaliser.  For seed in (kSeed0, kSeed1):  h = seed;  for p in the sorted list, in order:
// h = mix(h ^ p);  then h = mix(h ^ n).  key[b] = (h of kSeed0, h of kSeed1), stored as int64 bit patterns.  It depends on
// (n, sorted list) only: duplicates are kept, so a graph with a doubled triple has another key, as its string has.
//
// Sort.  A bitonic network over NS = the power of two >= cap, elements past n being the filler.
//   cap <=   64 : one WAVE per row, 4 rows per 256-thread workgroup; lane s owns slot s, the 21 compare-exchange steps are
//                 __shfl_xor over the 64 lanes; no LDS, no barrier.  The fold reads element i with a uniform __shfl.
//   cap <= 1024 : one 256-thread workgroup per row; the list lives in 8 KB of LDS (+ 16 B of reduction slots), one barrier per
//                 step, NS / 2 compare-exchange pairs per step over the threads.  Pair t of a step with distance j touches
//                 elements i = ((t & ~(j - 1)) << 1 | t & (j - 1)) and i + j: for j >= 32 a wave's 8-byte reads are consecutive
//                 (conflict-free); for j < 32 runs of j consecutive elements alternate with gaps of j, which at j = 1 is a
//                 stride of 16 bytes, a 2-way bank conflict on the last step of each merge.  Thread 0 folds the key from LDS.
//   cap >  1024 : ARK_ERR_SHAPE, nothing is launched.
// The path depends on cap alone.  No atomics, nothing crosses a workgroup, every loop is bounded by cap (<= 1024).
#include "common.h"
#include "../../include/ark_amd.h"

namespace ark {

typedef unsigned long long gk_u64;

constexpr gk_u64 kGraphSeed0 = 0x9E3779B97F4A7C15ull;   // == ARK_GRAPH_KEY_SEED0 / 1 (include/ark_amd.h)
constexpr gk_u64 kGraphSeed1 = 0xC2B2AE3D27D4EB4Full;
constexpr gk_u64 kGraphFill = ~0ull;
constexpr int kGraphCapWave = 64;
constexpr int kGraphCapBlock = 1024;
static_assert(kGraphSeed0 == ARK_GRAPH_KEY_SEED0 && kGraphSeed1 == ARK_GRAPH_KEY_SEED1, "key seeds");

__device__ __forceinline__ gk_u64 graph_mix(gk_u64 x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

__device__ __forceinline__ int graph_row_len(const int64_t* __restrict__ lens, int b, int row_len) {
  if (!lens) return row_len;
  const int64_t l = lens[b];
  return l < 0 ? 0 : (l < (int64_t)row_len ? (int)l : row_len);
}

// slot s of a row: true when the list ends in front of it; otherwise p = its packed triple
__device__ __forceinline__ bool graph_slot(const int64_t* __restrict__ row, int s, int cap, int len, int64_t eos, gk_u64& p) {
  p = kGraphFill;
  if (s >= cap || 3 + 3 * s >= len) return true;
  const int64_t a = row[1 + 3 * s];
  if (a == eos) return true;
  p = ((gk_u64)a << 42) | ((gk_u64)row[2 + 3 * s] << 21) | (gk_u64)row[3 + 3 * s];
  return false;
}

__global__ __launch_bounds__(256) void graph_canon_wave_kernel(const int64_t* __restrict__ toks, long ld, int B, int cap,
                                                               int row_len, const int64_t* __restrict__ lens, int64_t eos,
                                                               int64_t* __restrict__ canon, int* __restrict__ n_out,
                                                               int* __restrict__ nset_out, int64_t* __restrict__ key) {
  const int b = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (b >= B) return;   // a whole wave leaves; this path has no barrier
  const int lane = (int)(threadIdx.x & 63);
  const int len = graph_row_len(lens, b, row_len);
  gk_u64 v;
  const bool stop = graph_slot(toks + (long)b * ld, lane, cap, len, eos, v);
  const gk_u64 stops = __ballot(stop);
  const int n = stops ? (int)__ffsll((long long)stops) - 1 : 64;
  if (lane >= n) v = kGraphFill;
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const gk_u64 o = __shfl_xor(v, j, 64);
      const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
      v = (keep_min == (o < v)) ? o : v;
    }
  }
  const gk_u64 prev = __shfl_up(v, 1, 64);
  const int nset = __popcll(__ballot(lane < n && (lane == 0 || v != prev)));
  gk_u64 h0 = kGraphSeed0, h1 = kGraphSeed1;
  for (int i = 0; i < n; ++i) {   // n is uniform over the wave
    const gk_u64 p = __shfl(v, i, 64);
    h0 = graph_mix(h0 ^ p);
    h1 = graph_mix(h1 ^ p);
  }
  h0 = graph_mix(h0 ^ (gk_u64)n);
  h1 = graph_mix(h1 ^ (gk_u64)n);
  if (lane < cap) canon[(long)b * cap + lane] = (int64_t)v;
  if (lane == 0) {
    n_out[b] = n;
    nset_out[b] = nset;
    key[2 * (long)b] = (int64_t)h0;
    key[2 * (long)b + 1] = (int64_t)h1;
  }
}

// (sum or min over the 256 threads of a workgroup, the same value in every thread; `part` = 4 ints of LDS)
template <class Op>
__device__ __forceinline__ int graph_block_reduce(int v, Op op, int* part) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  __syncthreads();   // (the previous reduction's reads of `part` are over)
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return op(op(part[0], part[1]), op(part[2], part[3]));
}

__global__ __launch_bounds__(256) void graph_canon_block_kernel(const int64_t* __restrict__ toks, long ld, int cap, int ns,
                                                                int row_len, const int64_t* __restrict__ lens, int64_t eos,
                                                                int64_t* __restrict__ canon, int* __restrict__ n_out,
                                                                int* __restrict__ nset_out, int64_t* __restrict__ key) {
  __shared__ gk_u64 a[kGraphCapBlock];
  __shared__ int part[4];
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int64_t* __restrict__ row = toks + (long)b * ld;
  const int len = graph_row_len(lens, b, row_len);
  int first = cap;   // the first slot of this thread's that ends the list
  for (int s = tid; s < ns; s += 256) {
    gk_u64 p;
    const bool stop = graph_slot(row, s, cap, len, eos, p);
    a[s] = p;
    if (stop && s < first) first = s;
  }
  const int n = graph_block_reduce(first, [](int x, int y) { return x < y ? x : y; }, part);
  for (int s = tid; s < ns; s += 256)
    if (s >= n) a[s] = kGraphFill;
  for (int k = 2; k <= ns; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int t = tid; t < (ns >> 1); t += 256) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const gk_u64 x = a[i], y = a[i + j];
        if ((x > y) == ((i & k) == 0)) {
          a[i] = y;
          a[i + j] = x;
        }
      }
    }
  }
  __syncthreads();
  int cnt = 0;
  for (int i = tid; i < n; i += 256) cnt += (i == 0 || a[i] != a[i - 1]) ? 1 : 0;
  const int nset = graph_block_reduce(cnt, [](int x, int y) { return x + y; }, part);
  for (int i = tid; i < cap; i += 256) canon[(long)b * cap + i] = (int64_t)a[i];
  if (tid == 0) {
    gk_u64 h0 = kGraphSeed0, h1 = kGraphSeed1;
    for (int i = 0; i < n; ++i) {
      const gk_u64 p = a[i];
      h0 = graph_mix(h0 ^ p);
      h1 = graph_mix(h1 ^ p);
    }
    n_out[b] = n;
    nset_out[b] = nset;
    key[2 * (long)b] = (int64_t)graph_mix(h0 ^ (gk_u64)n);
    key[2 * (long)b + 1] = (int64_t)graph_mix(h1 ^ (gk_u64)n);
  }
}

// One wave per pair (A = row ia[q], B = row ib[q] of canon): every lane takes the FIRST occurrences among its strided elements
// of A and looks each up in B by binary search (both lists ascending as unsigned values); B's first occurrences are counted the
// same way.  A pair with an index outside 0 .. rows - 1 gets -1 in all three outputs.
__global__ __launch_bounds__(256) void graph_pair_stats_kernel(const int64_t* __restrict__ canon, const int* __restrict__ n,
                                                               int rows, int cap, const int* __restrict__ ia,
                                                               const int* __restrict__ ib, int P, int* __restrict__ inter,
                                                               int* __restrict__ da, int* __restrict__ db) {
  const int q = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (q >= P) return;
  const int lane = (int)(threadIdx.x & 63);
  const int ra = ia[q], rb = ib[q];
  if ((unsigned)ra >= (unsigned)rows || (unsigned)rb >= (unsigned)rows) {
    if (lane == 0) inter[q] = da[q] = db[q] = -1;
    return;
  }
  const gk_u64* __restrict__ A = reinterpret_cast<const gk_u64*>(canon) + (long)ra * cap;
  const gk_u64* __restrict__ Bv = reinterpret_cast<const gk_u64*>(canon) + (long)rb * cap;
  const int na = min(max(n[ra], 0), cap), nb = min(max(n[rb], 0), cap);
  int c_a = 0, c_b = 0, c_i = 0;
  for (int i = lane; i < na; i += 64) {
    const gk_u64 x = A[i];
    if (i > 0 && A[i - 1] == x) continue;
    ++c_a;
    int lo = 0, hi = nb;   // first position of B with B[pos] >= x
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (Bv[mid] < x) lo = mid + 1; else hi = mid;
    }
    c_i += (lo < nb && Bv[lo] == x) ? 1 : 0;
  }
  for (int i = lane; i < nb; i += 64) c_b += (i == 0 || Bv[i - 1] != Bv[i]) ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    c_a += __shfl_xor(c_a, o, 64);
    c_b += __shfl_xor(c_b, o, 64);
    c_i += __shfl_xor(c_i, o, 64);
  }
  if (lane == 0) {
    inter[q] = c_i;
    da[q] = c_a;
    db[q] = c_b;
  }
}

}  // namespace ark

extern "C" int ark_graph_canon(const int64_t* toks, int64_t ld, int B, int row_len, const int64_t* lens, int64_t eos,
                               int64_t* canon, int* n, int* nset, int64_t* key, void* stream) {
  using namespace ark;
  if (!toks || !n || !nset || !key || B <= 0 || row_len < 1 || ld < row_len) return ARK_ERR_ARG;
  const int cap = (row_len - 1) / 3;
  if (cap > kGraphCapBlock) return ARK_ERR_SHAPE;
  if (cap > 0 && !canon) return ARK_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (cap <= kGraphCapWave) {
    hipLaunchKernelGGL(graph_canon_wave_kernel, dim3((B + 3) / 4), dim3(256), 0, st, toks, (long)ld, B, cap, row_len, lens, eos,
                       canon, n, nset, key);
  } else {
    int ns = 128;
    while (ns < cap) ns <<= 1;
    hipLaunchKernelGGL(graph_canon_block_kernel, dim3(B), dim3(256), 0, st, toks, (long)ld, cap, ns, row_len, lens, eos, canon, n,
                       nset, key);
  }
  ARK_LAUNCH_CHECK();
  return 0;
}

extern "C" int ark_graph_pair_stats(const int64_t* canon, const int* n, int rows, int cap, const int* ia, const int* ib, int P,
                                    int* inter, int* da, int* db, void* stream) {
  using namespace ark;
  if (!n || !ia || !ib || !inter || !da || !db || rows <= 0 || P <= 0 || cap < 0) return ARK_ERR_ARG;
  if (cap > kGraphCapBlock) return ARK_ERR_SHAPE;
  if (cap > 0 && !canon) return ARK_ERR_ARG;
  hipLaunchKernelGGL(graph_pair_stats_kernel, dim3((P + 3) / 4), dim3(256), 0, (hipStream_t)stream, canon, n, rows, cap, ia, ib,
                     P, inter, da, db);
  ARK_LAUNCH_CHECK();
  return 0;
}
