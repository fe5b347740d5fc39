// Canonical graphs on the device: token rows -> sorted packed triples + a 128-bit order-independent key (ark_graph_canon),
// set statistics of pairs of canonical graphs (ark_graph_pair_stats), and for every graph of one batch the graph of another
// with the largest Jaccard index (ark_graph_nearest, described in front of its kernels).  What kgvae.model.utils does per row in the
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

// ---------------------------------------------------------------------------------- nearest reference (ark_graph_nearest)
// For every query row the reference row with the largest Jaccard index of the two sets of distinct triples.  J is kept as the
// fraction num / den: (1, 1) when both sets are empty, else (inter, dq + dr - inter), den >= 1; two fractions are compared by
// num_a * den_b against num_b * den_a (num <= 1024, den <= 2048: the products stay below 2^21), equal fractions by the lower
// reference index.  That order is TOTAL, so the winner of a set of references does not depend on how the set is cut into
// strips, waves or lanes, nor on the order its parts are merged in.
//   both caps <= 8 : lane per pair.  A workgroup owns 64 queries, lane l of each of its 4 waves holding query l's distinct
//                    triples in 8 registers (repeats and empty slots = the filler ~0).  The strip of references passes in
//                    chunks of 64 rows staged in 4 KB of LDS (repeats and empty slots = ~0 - 1, so that an empty slot never
//                    equals an empty slot); wave w takes rows w, w + 4, ... of the chunk, reads each element once as an LDS
//                    broadcast and compares it with the 8 registers: 64 compares per pair, no branch, no bank conflict.
//   both caps <= 64: lane per pair again, the queries' and the chunk's distinct lists in LDS and a linear merge per pair
//                    (graph_nearest_merge_kernel, described there).
//   otherwise      : wave per reference row.  A workgroup stages TQ queries' lists (TQ = 8, or 4 above capq 512: <= 32 KB of
//                    LDS) and wave w takes rows r0 + w, r0 + w + 4, ... of the strip: lane l holds the row's elements l,
//                    l + 64, ..., looks every FIRST occurrence up in each of the TQ lists by binary search, and the hits are
//                    counted with a ballot, so the TQ counts are wave-uniform and no shuffle reduction is needed.
// Either way a reference row is fetched once per tile of queries, each wave keeps the best reference of its rows per query,
// the 4 waves are merged through LDS, and with more than one strip the per-strip winners go to the caller's scratch and
// graph_nearest_combine_kernel merges them.  No atomics.  Every index is bounded by the clipped n (<= cap <= 1024).
constexpr int kNearSmallCap = 8;
constexpr int kNearChunk = 64;
constexpr int kNearMaxStrips = 1024;
constexpr gk_u64 kNearFillRef = ~0ull - 1;

__device__ __forceinline__ int near_clip(int n, int cap) { return min(max(n, 0), cap); }

// is reference ci with (cinter, cdr) in front of reference bi with (binter, bdr) for a query of dq distinct triples?  An index
// of -1 is "none".
__device__ __forceinline__ bool near_better(int dq, int ci, int cinter, int cdr, int bi, int binter, int bdr) {
  if (ci < 0) return false;
  if (bi < 0) return true;
  const int cu = dq + cdr - cinter, bu = dq + bdr - binter;
  const int cn = cu == 0 ? 1 : cinter, cd = cu == 0 ? 1 : cu;
  const int bn = bu == 0 ? 1 : binter, bd = bu == 0 ? 1 : bu;
  const int l = cn * bd, r = bn * cd;
  return l > r || (l == r && ci < bi);
}

__global__ __launch_bounds__(256) void graph_nearest_lane_kernel(const int64_t* __restrict__ qcanon, const int* __restrict__ qn,
                                                                 int NQ, int capq, const int64_t* __restrict__ rcanon,
                                                                 const int* __restrict__ rn, int NR, int capr, int exclude_self,
                                                                 int per, int* __restrict__ pidx, int* __restrict__ pinter,
                                                                 int* __restrict__ pdr, int* __restrict__ dq_out) {
  __shared__ gk_u64 ref[kNearChunk * kNearSmallCap];
  __shared__ int ref_d[kNearChunk];
  __shared__ int best_s[3][3][64];
  const int tid = (int)threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q = (int)blockIdx.x * 64 + lane;
  const int r0 = (int)min((long)NR, (long)blockIdx.y * per), r1 = (int)min((long)NR, (long)r0 + per);
  const gk_u64* __restrict__ Q = reinterpret_cast<const gk_u64*>(qcanon);
  const gk_u64* __restrict__ R = reinterpret_cast<const gk_u64*>(rcanon);
  gk_u64 qv[kNearSmallCap];
  int dq = 0;
  {
    const int nq = q < NQ ? near_clip(qn[q], capq) : 0;
    gk_u64 prev = 0;
#pragma unroll
    for (int i = 0; i < kNearSmallCap; ++i) {
      gk_u64 x = kGraphFill;
      if (i < nq) {
        const gk_u64 raw = Q[(long)q * capq + i];
        if (i == 0 || raw != prev) {
          x = raw;
          ++dq;
        }
        prev = raw;
      }
      qv[i] = x;
    }
  }
  int bi = -1, binter = -1, bdr = -1;
  for (int c0 = r0; c0 < r1; c0 += kNearChunk) {   // (uniform over the workgroup)
    const int cn = min(kNearChunk, r1 - c0);
    __syncthreads();   // the previous chunk has been read
    for (int s = tid; s < kNearChunk * kNearSmallCap; s += 256) {   // two rounds, all threads in both
      const int j = s >> 3, e = s & 7;
      gk_u64 x = kNearFillRef;
      bool first = false;
      if (j < cn) {
        const int r = c0 + j;
        if (e < near_clip(rn[r], capr)) {
          const gk_u64* __restrict__ row = R + (long)r * capr;
          const gk_u64 raw = row[e];
          first = e == 0 || row[e - 1] != raw;
          if (first) x = raw;
        }
      }
      ref[s] = x;
      const gk_u64 m = __ballot(first);
      if (e == 0) ref_d[j] = __popcll((m >> lane) & 0xFFull);   // (a row's 8 slots are 8 neighbouring lanes)
    }
    __syncthreads();
    for (int j = w; j < cn; j += 4) {
      int inter = 0;
#pragma unroll
      for (int e = 0; e < kNearSmallCap; ++e) {
        const gk_u64 x = ref[j * kNearSmallCap + e];
        bool hit = false;
#pragma unroll
        for (int i = 0; i < kNearSmallCap; ++i) hit |= qv[i] == x;
        inter += hit ? 1 : 0;
      }
      const int r = c0 + j, dr = ref_d[j];
      const int ci = (q < NQ && !(exclude_self && r == q)) ? r : -1;
      if (near_better(dq, ci, inter, dr, bi, binter, bdr)) {
        bi = ci;
        binter = inter;
        bdr = dr;
      }
    }
  }
  if (w > 0) {
    best_s[w - 1][0][lane] = bi;
    best_s[w - 1][1][lane] = binter;
    best_s[w - 1][2][lane] = bdr;
  }
  __syncthreads();
  if (w == 0 && q < NQ) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int ci = best_s[k][0][lane], cinter = best_s[k][1][lane], cdr = best_s[k][2][lane];
      if (near_better(dq, ci, cinter, cdr, bi, binter, bdr)) {
        bi = ci;
        binter = cinter;
        bdr = cdr;
      }
    }
    const long o = (long)blockIdx.y * NQ + q;
    pidx[o] = bi;
    pinter[o] = binter;
    pdr[o] = bdr;
    if (blockIdx.y == 0) dq_out[q] = dq;
  }
}

extern __shared__ gk_u64 near_lds[];

// one row of a canonical batch -> its DISTINCT elements, in order, at dst[0], dst[stride], ...; returns their number.  One
// wave, cap <= 64 (one element per lane); the position of a first occurrence is the number of first occurrences below it.
__device__ __forceinline__ int near_compact_row(const gk_u64* __restrict__ row, int n, int lane, gk_u64* dst, int stride) {
  gk_u64 x = 0;
  bool first = false;
  if (lane < n) {
    x = row[lane];
    first = lane == 0 || row[lane - 1] != x;
  }
  const gk_u64 m = __ballot(first);
  if (first) dst[__popcll(m & ((1ull << lane) - 1)) * stride] = x;
  return __popcll(m);
}

// Lane per pair for lists of up to 64 triples (wd-movies): as graph_nearest_lane_kernel, but the 64 queries' distinct lists
// live in LDS, element i of query l at [i][l] (a lane's 8-byte read lands on banks 2l, 2l + 1 whatever its i: no conflict
// within a half-wave), the chunk is kMergeChunk reference rows of distinct elements, and a pair is one linear merge of two
// ascending lists: at most dq + dr steps of two LDS reads.  Dynamic LDS: (64 capq + kMergeChunk capr) * 8 bytes.
constexpr int kNearMergeCap = 64;
constexpr int kNearMergeChunk = 32;

__global__ __launch_bounds__(256) void graph_nearest_merge_kernel(const int64_t* __restrict__ qcanon, const int* __restrict__ qn,
                                                                  int NQ, int capq, const int64_t* __restrict__ rcanon,
                                                                  const int* __restrict__ rn, int NR, int capr, int exclude_self,
                                                                  int per, int* __restrict__ pidx, int* __restrict__ pinter,
                                                                  int* __restrict__ pdr, int* __restrict__ dq_out) {
  __shared__ int dq_s[64];
  __shared__ int ref_d[kNearMergeChunk];
  __shared__ int best_s[3][3][64];
  gk_u64* qlist = near_lds;                       // [capq][64]
  gk_u64* rlist = near_lds + (long)capq * 64;     // [kNearMergeChunk][capr]
  const int tid = (int)threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q0 = (int)blockIdx.x * 64, q = q0 + lane;
  const int r0 = (int)min((long)NR, (long)blockIdx.y * per), r1 = (int)min((long)NR, (long)r0 + per);
  const gk_u64* __restrict__ Q = reinterpret_cast<const gk_u64*>(qcanon);
  const gk_u64* __restrict__ R = reinterpret_cast<const gk_u64*>(rcanon);
  for (int qi = w; qi < 64; qi += 4) {   // (uniform over the wave)
    int d = 0;
    if (q0 + qi < NQ) d = near_compact_row(Q + (long)(q0 + qi) * capq, near_clip(qn[q0 + qi], capq), lane, qlist + qi, 64);
    if (lane == 0) dq_s[qi] = d;
  }
  __syncthreads();
  const int dq = dq_s[lane];
  int bi = -1, binter = -1, bdr = -1;
  for (int c0 = r0; c0 < r1; c0 += kNearMergeChunk) {   // (uniform over the workgroup)
    const int cn = min(kNearMergeChunk, r1 - c0);
    __syncthreads();   // the previous chunk has been read
    for (int j = w; j < cn; j += 4) {
      const int r = c0 + j;
      const int d = near_compact_row(R + (long)r * capr, near_clip(rn[r], capr), lane, rlist + j * capr, 1);
      if (lane == 0) ref_d[j] = d;
    }
    __syncthreads();
    for (int j = w; j < cn; j += 4) {
      const int dr = ref_d[j];
      const gk_u64* row = rlist + j * capr;
      int i = 0, k = 0, inter = 0;
      while (i < dq && k < dr) {
        const gk_u64 a = qlist[i * 64 + lane], b = row[k];
        inter += a == b ? 1 : 0;
        i += a <= b ? 1 : 0;
        k += b <= a ? 1 : 0;
      }
      const int r = c0 + j;
      const int ci = (q < NQ && !(exclude_self && r == q)) ? r : -1;
      if (near_better(dq, ci, inter, dr, bi, binter, bdr)) {
        bi = ci;
        binter = inter;
        bdr = dr;
      }
    }
  }
  if (w > 0) {
    best_s[w - 1][0][lane] = bi;
    best_s[w - 1][1][lane] = binter;
    best_s[w - 1][2][lane] = bdr;
  }
  __syncthreads();
  if (w == 0 && q < NQ) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int ci = best_s[k][0][lane], cinter = best_s[k][1][lane], cdr = best_s[k][2][lane];
      if (near_better(dq, ci, cinter, cdr, bi, binter, bdr)) {
        bi = ci;
        binter = cinter;
        bdr = cdr;
      }
    }
    const long o = (long)blockIdx.y * NQ + q;
    pidx[o] = bi;
    pinter[o] = binter;
    pdr[o] = bdr;
    if (blockIdx.y == 0) dq_out[q] = dq;
  }
}

template <int TQ>
__global__ __launch_bounds__(256) void graph_nearest_wave_kernel(const int64_t* __restrict__ qcanon, const int* __restrict__ qn,
                                                                 int NQ, int capq, const int64_t* __restrict__ rcanon,
                                                                 const int* __restrict__ rn, int NR, int capr, int exclude_self,
                                                                 int per, int* __restrict__ pidx, int* __restrict__ pinter,
                                                                 int* __restrict__ pdr, int* __restrict__ dq_out) {
  gk_u64* lists = near_lds;                                       // [TQ][capq]
  int* nq_s = reinterpret_cast<int*>(near_lds + (long)TQ * capq);   // [TQ]
  int* dq_s = nq_s + TQ;                                          // [TQ]
  int* best_s = dq_s + TQ;                                        // [4][TQ][3]
  const int tid = (int)threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q0 = (int)blockIdx.x * TQ;
  const int r0 = (int)min((long)NR, (long)blockIdx.y * per), r1 = (int)min((long)NR, (long)r0 + per);
  const gk_u64* __restrict__ Q = reinterpret_cast<const gk_u64*>(qcanon);
  const gk_u64* __restrict__ R = reinterpret_cast<const gk_u64*>(rcanon);
  for (int qi = w; qi < TQ; qi += 4) {
    const int q = q0 + qi;
    int n = 0, d = 0;
    if (q < NQ) {   // (uniform over the wave)
      n = near_clip(qn[q], capq);
      const gk_u64* __restrict__ row = Q + (long)q * capq;
      for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool first = false;
        if (i < n) {
          const gk_u64 x = row[i];
          lists[qi * capq + i] = x;
          first = i == 0 || row[i - 1] != x;
        }
        d += __popcll(__ballot(first));
      }
    }
    if (lane == 0) {
      nq_s[qi] = n;
      dq_s[qi] = d;
    }
  }
  __syncthreads();
  int nq[TQ], dq[TQ], bi[TQ], binter[TQ], bdr[TQ];
#pragma unroll
  for (int qi = 0; qi < TQ; ++qi) {
    nq[qi] = nq_s[qi];
    dq[qi] = dq_s[qi];
    bi[qi] = binter[qi] = bdr[qi] = -1;
  }
  for (int r = r0 + w; r < r1; r += 4) {   // (uniform over the wave)
    const int nr = near_clip(rn[r], capr);
    const gk_u64* __restrict__ row = R + (long)r * capr;
    int c[TQ];
#pragma unroll
    for (int qi = 0; qi < TQ; ++qi) c[qi] = 0;
    int dr = 0;
    for (int base = 0; base < nr; base += 64) {
      const int i = base + lane;
      gk_u64 x = 0;
      bool first = false;
      if (i < nr) {
        x = row[i];
        first = i == 0 || row[i - 1] != x;
      }
      dr += __popcll(__ballot(first));
#pragma unroll
      for (int qi = 0; qi < TQ; ++qi) {
        const gk_u64* L = lists + qi * capq;
        int lo = 0, hi = first ? nq[qi] : 0;   // first position of L with L[pos] >= x
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (L[mid] < x) lo = mid + 1; else hi = mid;
        }
        const bool hit = first && lo < nq[qi] && L[lo] == x;
        c[qi] += __popcll(__ballot(hit));
      }
    }
#pragma unroll
    for (int qi = 0; qi < TQ; ++qi) {
      const int q = q0 + qi;
      const int ci = (q < NQ && !(exclude_self && r == q)) ? r : -1;
      if (near_better(dq[qi], ci, c[qi], dr, bi[qi], binter[qi], bdr[qi])) {
        bi[qi] = ci;
        binter[qi] = c[qi];
        bdr[qi] = dr;
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int qi = 0; qi < TQ; ++qi) {
      int* b = best_s + (w * TQ + qi) * 3;
      b[0] = bi[qi];
      b[1] = binter[qi];
      b[2] = bdr[qi];
    }
  }
  __syncthreads();
  if (tid < TQ && q0 + tid < NQ) {
    const int d = dq_s[tid];
    int ti = -1, tinter = -1, tdr = -1;
    for (int k = 0; k < 4; ++k) {
      const int* b = best_s + (k * TQ + tid) * 3;
      if (near_better(d, b[0], b[1], b[2], ti, tinter, tdr)) {
        ti = b[0];
        tinter = b[1];
        tdr = b[2];
      }
    }
    const long o = (long)blockIdx.y * NQ + q0 + tid;
    pidx[o] = ti;
    pinter[o] = tinter;
    pdr[o] = tdr;
    if (blockIdx.y == 0) dq_out[q0 + tid] = d;
  }
}

// the winners of the strips of one query, merged (p*[strips][NQ])
__global__ __launch_bounds__(256) void graph_nearest_combine_kernel(const int* __restrict__ pidx, const int* __restrict__ pinter,
                                                                    const int* __restrict__ pdr, int NQ, int strips,
                                                                    const int* __restrict__ dq, int* __restrict__ idx,
                                                                    int* __restrict__ inter, int* __restrict__ dr) {
  const int q = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (q >= NQ) return;
  const int d = dq[q];
  int bi = -1, binter = -1, bdr = -1;
  for (int s = 0; s < strips; ++s) {
    const long o = (long)s * NQ + q;
    const int ci = pidx[o], cinter = pinter[o], cdr = pdr[o];
    if (near_better(d, ci, cinter, cdr, bi, binter, bdr)) {
      bi = ci;
      binter = cinter;
      bdr = cdr;
    }
  }
  idx[q] = bi;
  inter[q] = binter;
  dr[q] = bdr;
}

static bool near_small(int capq, int capr) { return capq <= kNearSmallCap && capr <= kNearSmallCap; }
static bool near_merge(int capq, int capr) { return !near_small(capq, capr) && capq <= kNearMergeCap && capr <= kNearMergeCap; }
static int near_tile(int capq, int capr) { return capq <= kNearMergeCap && capr <= kNearMergeCap ? 64 : (capq > 512 ? 4 : 8); }

// strips of the reference axis: the caller's number, or enough to put ~2048 workgroups on the chip while a strip still holds
// a chunk's worth of rows; never more than there are rows
static int near_strips(int NQ, int NR, int capq, int capr, int strips) {
  const int most = max(1, min(NR, kNearMaxStrips));
  if (strips > 0) return min(strips, most);
  const int tq = near_tile(capq, capr);
  const long tiles = ((long)NQ + tq - 1) / tq;
  const int rows = near_small(capq, capr) ? kNearChunk : (near_merge(capq, capr) ? kNearMergeChunk : 16);
  return (int)max(1l, min((2048 + tiles - 1) / tiles, (long)min(most, max(1, NR / rows))));
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

extern "C" long ark_graph_nearest_scratch_bytes(int NQ, int NR, int capq, int capr, int strips) {
  using namespace ark;
  if (NQ <= 0 || NR < 0 || capq < 0 || capr < 0) return 0;
  const int s = near_strips(NQ, NR, capq, capr, strips);
  return s > 1 ? 3l * s * NQ * (long)sizeof(int) : 0;
}

extern "C" int ark_graph_nearest(const int64_t* qcanon, const int* qn, int NQ, int capq, const int64_t* rcanon, const int* rn,
                                 int NR, int capr, int exclude_self, int strips, int* idx, int* inter, int* dq, int* dr,
                                 void* scratch, int64_t scratch_bytes, void* stream) {
  using namespace ark;
  if (!qn || !idx || !inter || !dq || !dr || NQ <= 0 || NR < 0 || capq < 0 || capr < 0) return ARK_ERR_ARG;
  if (capq > kGraphCapBlock || capr > kGraphCapBlock) return ARK_ERR_SHAPE;
  if ((capq > 0 && !qcanon) || (NR > 0 && (!rn || (capr > 0 && !rcanon)))) return ARK_ERR_ARG;
  const int ns = near_strips(NQ, NR, capq, capr, strips);
  const long need = ns > 1 ? 3l * ns * NQ * (long)sizeof(int) : 0;
  if (need > 0 && (!scratch || scratch_bytes < need)) return ARK_ERR_ARG;
  const int per = (NR + ns - 1) / ns;
  int *pidx = idx, *pinter = inter, *pdr = dr;
  if (ns > 1) {
    pidx = static_cast<int*>(scratch);
    pinter = pidx + (long)ns * NQ;
    pdr = pinter + (long)ns * NQ;
  }
  hipStream_t st = (hipStream_t)stream;
  const int tq = near_tile(capq, capr);
  const dim3 grid((NQ + tq - 1) / tq, ns);
  if (near_small(capq, capr)) {
    hipLaunchKernelGGL(graph_nearest_lane_kernel, grid, dim3(256), 0, st, qcanon, qn, NQ, capq, rcanon, rn, NR, capr, exclude_self,
                       per, pidx, pinter, pdr, dq);
  } else if (near_merge(capq, capr)) {
    const size_t lds = ((size_t)64 * capq + (size_t)kNearMergeChunk * capr) * sizeof(gk_u64);
    hipLaunchKernelGGL(graph_nearest_merge_kernel, grid, dim3(256), lds, st, qcanon, qn, NQ, capq, rcanon, rn, NR, capr,
                       exclude_self, per, pidx, pinter, pdr, dq);
  } else {
    const size_t lds = (size_t)tq * capq * sizeof(gk_u64) + (size_t)tq * 14 * sizeof(int);
    if (tq == 8)
      hipLaunchKernelGGL(graph_nearest_wave_kernel<8>, grid, dim3(256), lds, st, qcanon, qn, NQ, capq, rcanon, rn, NR, capr,
                         exclude_self, per, pidx, pinter, pdr, dq);
    else
      hipLaunchKernelGGL(graph_nearest_wave_kernel<4>, grid, dim3(256), lds, st, qcanon, qn, NQ, capq, rcanon, rn, NR, capr,
                         exclude_self, per, pidx, pinter, pdr, dq);
  }
  ARK_LAUNCH_CHECK();
  if (ns > 1) {
    hipLaunchKernelGGL(graph_nearest_combine_kernel, dim3((NQ + 255) / 256), dim3(256), 0, st, pidx, pinter, pdr, NQ, ns, dq, idx,
                       inter, dr);
    ARK_LAUNCH_CHECK();
  }
  return 0;
}
