// knn_pattern.hip -- the FSAI pattern's k-nearest-neighbour search (Nfft4GPDistanceEuclidKnn, kernels.c:121-278):
// pattern row i >= lfil holds the lfil-1 nearest points among 0..i-1 by (squared distance, index), then i.
//
//   k_knn          the radix select: one workgroup per row, an MSB-first radix select on the bits of the
//                  squared distances (non-negative doubles order like their bit patterns), then a rank sort
//                  of the survivors by (distance, index).  Settles every row of any data.
//   k_knn_bounded  the fp64 bounded scan: 16 rows per workgroup, sample / count / collect (d <= 64)
//   k_knn_screen   the 32-row screen: fp32 keys on v_mfma_f32_32x32x2_f32, exact fp64 ranking (d <= 64)
//   k_knn_tile     the tile screen: 256 rows per workgroup, bf16-split keys (d <= 32, lfil <= 25)
//   knn_pattern()  the cascade over them, and Nfft4GPAmdDebugKnn, the hook the tests and tools/knn_probe.py
//                  call it through.
// Every kernel takes all rows lfil..n-1 or an ascending list of rows (a row shard's own rows, or the rows an
// earlier stage could not settle), and every stage but the radix select appends the rows it cannot settle to a
// fail list.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "internal.h"

using namespace nfft4gp_amd;

namespace {

constexpr int kKnnThreads = 256;
constexpr int kKnnGather = 256;    // survivors of the radix select sorted directly

__device__ __forceinline__ double sqdist(const double* __restrict__ X, int ldim, int d, const double* xi, int j)
{
   double s = 0.0;
   for (int c = 0; c < d; c++) {
      const double t = X[(size_t)c * ldim + j] - xi[c];
      s = fma(t, t, s);
   }
   return s;
}

// The rank of each of the cnt candidates (key[e], idx[e]) held in LDS by (key, index), candidate e on thread t of
// nt; emit(rank, e) for the candidates of rank below `first`.  KeyT: the bits of a non-negative double, or the
// double itself.
template <typename KeyT, typename F>
__device__ __forceinline__ void knn_rank(const KeyT* key, const int* idx, int cnt, int first, int t, int nt, F&& emit)
{
   for (int e = t; e < cnt; e += nt) {
      const KeyT ke = key[e];
      const int ie = idx[e];
      int rank = 0;
      for (int o = 0; o < cnt; o++) {
         const KeyT ko = key[o];
         rank += (ko < ke || (ko == ke && idx[o] < ie)) ? 1 : 0;
      }
      if (rank < first) emit(rank, e);
   }
}

// ... and the first K of them, in that order, are the pattern row at ja_row
template <typename KeyT>
__device__ __forceinline__ void knn_rank_row(const KeyT* key, const int* idx, int cnt, int K, int t, int nt,
                                             int* __restrict__ ja_row)
{
   knn_rank(key, idx, cnt, K, t, nt, [&](int rank, int e) { ja_row[rank] = idx[e]; });
}

// The first bin of the 256-bin LDS histogram h whose cumulative count reaches K, or -1 when h holds fewer than
// K keys.  One wave; every lane returns it.
__device__ __forceinline__ int knn_kth_bin(const unsigned int* h, int K)
{
   const int lane = threadIdx.x & 63;
   unsigned int loc = 0;
   for (int b = 0; b < 4; b++) loc += h[lane * 4 + b];
   unsigned int incl = loc;
   for (int off = 1; off < 64; off <<= 1) {
      const unsigned int o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
   }
   const unsigned long long hit = __ballot(incl >= (unsigned)K);
   if (!hit) return -1;
   const int first = __ffsll((long long)hit) - 1;
   int b = lane * 4;
   if (lane == first) {
      unsigned int cum = incl - loc;
      for (; b < lane * 4 + 3; b++) {
         if (cum + h[b] >= (unsigned)K) break;
         cum += h[b];
      }
   }
   return __shfl(b, first, 64);
}

// pattern rows i in [lfil, n): ja[ia[i] .. ia[i] + lfil - 2] = the lfil-1 nearest of 0..i-1 by
// (squared distance, index), ja[ia[i] + lfil - 1] = i.  Grid-stride over rows, or over the rows of
// `rows` (nrows of them) when given: the rows k_knn_bounded could not settle.
__global__ __launch_bounds__(kKnnThreads) void k_knn(const double* __restrict__ X, int ldim, int n, int d, int lfil,
                                                     const int* __restrict__ ia, int* __restrict__ ja,
                                                     const int* __restrict__ rows, int nrows)
{
   __shared__ unsigned int hist[256];
   __shared__ double s_xi[kMaxDims];
   __shared__ unsigned long long s_key[kKnnGather + kFsaiMaxK];
   __shared__ int s_idx[kKnnGather + kFsaiMaxK];
   __shared__ int s_nsel, s_ngat;
   __shared__ unsigned long long s_prefix;
   __shared__ int s_bits, s_need, s_eq;
   const int tid = threadIdx.x;
   const int K = lfil - 1;
   const int nloop = rows ? nrows : n - lfil;
   for (int it = blockIdx.x; it < nloop; it += gridDim.x) {
      const int i = rows ? rows[it] : lfil + it;
      for (int c = tid; c < d; c += kKnnThreads) s_xi[c] = X[(size_t)c * ldim + i];
      if (tid == 0) {
         s_prefix = 0ull;
         s_bits = 0;
         s_need = K;
         s_eq = i;
      }
      __syncthreads();
      // MSB-first radix select: narrow the prefix of the K-th smallest key byte by byte until the
      // candidates that share it fit the gather buffer
      while (s_bits < 64 && s_eq > kKnnGather) {
         const int bits = s_bits;
         const unsigned long long prefix = s_prefix;
         for (int b = tid; b < 256; b += kKnnThreads) hist[b] = 0u;
         __syncthreads();
         for (int j = tid; j < i; j += kKnnThreads) {
            const unsigned long long u = (unsigned long long)__double_as_longlong(sqdist(X, ldim, d, s_xi, j));
            if (bits == 0 || (u >> (64 - bits)) == prefix) atomicAdd(&hist[(u >> (56 - bits)) & 255ull], 1u);
         }
         __syncthreads();
         if (tid == 0) {
            unsigned int cum = 0;
            int b = 0;
            for (; b < 255; b++) {
               if (cum + hist[b] >= (unsigned)s_need) break;
               cum += hist[b];
            }
            s_need -= (int)cum;
            s_eq = (int)hist[b];
            s_prefix = (prefix << 8) | (unsigned long long)b;
            s_bits = bits + 8;
         }
         __syncthreads();
      }
      // collect: keys below the prefix are in; keys equal to it compete for the remaining s_need slots
      if (tid == 0) {
         s_nsel = 0;
         s_ngat = 0;
      }
      __syncthreads();
      {
         const int bits = s_bits;
         const unsigned long long prefix = s_prefix;
         for (int j = tid; j < i; j += kKnnThreads) {
            const unsigned long long u = (unsigned long long)__double_as_longlong(sqdist(X, ldim, d, s_xi, j));
            const unsigned long long top = bits == 0 ? 0ull : (u >> (64 - bits));
            if (bits > 0 && top < prefix) {
               const int p = atomicAdd(&s_nsel, 1);
               s_key[kKnnGather + p] = u;
               s_idx[kKnnGather + p] = j;
            } else if (bits == 0 || top == prefix) {
               const int p = atomicAdd(&s_ngat, 1);
               if (p < kKnnGather) {
                  s_key[p] = u;
                  s_idx[p] = j;
               }
            }
         }
      }
      __syncthreads();
      // rank the gathered candidates by (key, index); the first s_need join the selection
      const int ng = min(s_ngat, kKnnGather);
      const int nsel0 = s_nsel;
      __syncthreads();
      knn_rank(s_key, s_idx, ng, K - nsel0, tid, kKnnThreads, [&](int rank, int e) {
         s_key[kKnnGather + nsel0 + rank] = s_key[e];
         s_idx[kKnnGather + nsel0 + rank] = s_idx[e];
      });
      __syncthreads();
      // final order of the K neighbours: by (key, index), then the point itself
      const int row = ia[i];
      knn_rank_row(s_key + kKnnGather, s_idx + kKnnGather, K, K, tid, kKnnThreads, ja + row);
      if (tid == 0) ja[row + K] = i;
      __syncthreads();
   }
}

// The same pattern rows, kKnnRows consecutive rows per workgroup sharing every load of a point (the
// scan is bound by the on-chip bandwidth of re-reading the earlier points, so the rows per workgroup
// set the speed), in two passes over the earlier points instead of k_knn's three to four:
//   sample  the squared distances to points 0..S-1 (S = min(i0, 4096)) histogrammed by exponent (256
//           bins over 2^-224 .. 2^31, clamped) give the bin of the sample's (lfil-1)-th smallest, so
//           every true neighbour has a key below tau = the bin's upper end;
//   count   keys below tau, binned by (exponent - (E-16), 4 top mantissa bits) with tau = 2^E -- 256
//           monotone bins over [2^(E-16), tau), smaller keys in bin 0 -- locate the bin b* of the
//           (lfil-1)-th key;
//   collect keys in bins below b* are in, keys in b* (at most kKnnGather2) are ranked by (key, index).
// Only keys below tau touch the LDS histograms (a few percent of them).  A row whose bin b* holds more
// than kKnnGather2 keys (duplicates, pathological data) is appended to `fail` for k_knn.  d <= 64.
constexpr int kKnnRows = 16;
constexpr int kKnnPoints = 2;  // points per thread in the distance scans (knn_scan)
constexpr int kKnnSample = 4096;
constexpr int kKnnGather2 = 128;
constexpr int kKnnMaxDims2 = 64;
constexpr int kExpBase = 1023 - 224;
__device__ __forceinline__ int knn_bin(unsigned long long u, int base)
{
   const int e = (int)(u >> 52);
   return (e < base) ? 0 : (((e - base) << 4) | (int)((u >> 48) & 15ull));
}

// The squared distances of points j in [0, jend) to the workgroup's R query rows (q in LDS), P points
// per thread so that every LDS read of a query coordinate serves P distances, and the next feature's
// loads issued before the current feature's arithmetic.  Each distance is the same sum as sqdist's:
// t = x_j - q, s = fma(t, t, s) over the features in order.  f(j, acc) sees the R keys of point j.
template <int P, int R, typename F>
__device__ __forceinline__ void knn_scan(const double* __restrict__ X, int ldim, int d, const double (*q)[R],
                                         int jend, F&& f)
{
   constexpr int T = kKnnThreads;
   for (int jb = threadIdx.x; jb < jend; jb += T * P) {
      double acc[P][R];
#pragma unroll
      for (int p = 0; p < P; p++)
#pragma unroll
         for (int r = 0; r < R; r++) acc[p][r] = 0.0;
      double xn[P];
#pragma unroll
      for (int p = 0; p < P; p++) xn[p] = jb + p * T < jend ? X[jb + p * T] : 0.0;
      for (int c = 0; c < d; c++) {
         double xc[P];
#pragma unroll
         for (int p = 0; p < P; p++) xc[p] = xn[p];
         if (c + 1 < d) {
#pragma unroll
            for (int p = 0; p < P; p++)
               xn[p] = jb + p * T < jend ? X[(size_t)(c + 1) * ldim + jb + p * T] : 0.0;
         }
#pragma unroll
         for (int r = 0; r < R; r++) {
            const double qv = q[c][r];
#pragma unroll
            for (int p = 0; p < P; p++) {
               const double t = xc[p] - qv;
               acc[p][r] = fma(t, t, acc[p][r]);
            }
         }
      }
#pragma unroll
      for (int p = 0; p < P; p++)
         if (jb + p * T < jend) f(jb + p * T, acc[p]);
   }
}

template <int P>
__global__ __launch_bounds__(kKnnThreads) void k_knn_bounded(const double* __restrict__ X, int ldim, int n, int d,
                                                             int lfil, const int* __restrict__ ia,
                                                             int* __restrict__ ja, int* __restrict__ fail,
                                                             int* __restrict__ nfail, const int* __restrict__ rows,
                                                             int nrows)
{
   constexpr int R = kKnnRows;
   __shared__ double q[kKnnMaxDims2][R];
   __shared__ unsigned int h0[R][256];
   __shared__ unsigned int h1[R][256];
   __shared__ unsigned long long s_key[R][kKnnGather2 + kFsaiMaxK];
   __shared__ int s_idx[R][kKnnGather2 + kFsaiMaxK];
   __shared__ unsigned long long s_tau[R];
   __shared__ int s_base[R], s_bstar[R], s_ok[R];
   __shared__ int s_nsel[R], s_ngat[R], s_row[R];
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
   const int K = lfil - 1;
   // rows: ascending row indices (nrows of them) instead of lfil..n-1
   const int nall = rows ? nrows : n - lfil;
   const int ngroups = (nall + R - 1) / R;
   for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
      const int nr = min(R, nall - g * R);
      const int i0 = rows ? rows[g * R] : lfil + g * R;
      if (tid < R) s_row[tid] = tid < nr ? (rows ? rows[g * R + tid] : i0 + tid) : n;
      __syncthreads();
      for (int e = tid; e < R * d; e += kKnnThreads) {
         const int r = e / d, c = e % d;
         q[c][r] = (r < nr) ? X[(size_t)c * ldim + s_row[r]] : 0.0;
      }
      for (int e = tid; e < R * 256; e += kKnnThreads) {
         h0[e / 256][e % 256] = 0u;
         h1[e / 256][e % 256] = 0u;
      }
      if (tid < R) {
         s_nsel[tid] = 0;
         s_ngat[tid] = 0;
      }
      __syncthreads();
      // sample: exponent histogram of keys to points 0..S-1 (S <= i0 <= every row's i)
      const int S = min(i0, kKnnSample);
      knn_scan<P, R>(X, ldim, d, q, S, [&](int, const double* acc) {
#pragma unroll
         for (int r = 0; r < R; r++)
            if (r < nr) {
               const int e = (int)((unsigned long long)__double_as_longlong(acc[r]) >> 52);
               atomicAdd(&h0[r][min(255, max(0, e - kExpBase))], 1u);
            }
      });
      __syncthreads();
      // one wave per row: the first bin where the cumulative count reaches K (the sample holds at least K keys)
      for (int r = wave; r < nr; r += kKnnThreads / 64) {
         const int b = knn_kth_bin(h0[r], K);
         if (lane == 0) {
            const int E = b + kExpBase + 1;  // keys of bin b have exponents < E (bin 255: any)
            s_tau[r] = (b == 255) ? ~0ull : ((unsigned long long)E << 52);
            s_base[r] = ((b == 255) ? 2047 : E) - 16;
         }
      }
      __syncthreads();
      // count: keys below tau by (exponent, 4 mantissa bits)
      const int jmax = s_row[nr - 1];
      knn_scan<P, R>(X, ldim, d, q, jmax, [&](int j, const double* acc) {
#pragma unroll
         for (int r = 0; r < R; r++) {
            const unsigned long long u = (unsigned long long)__double_as_longlong(acc[r]);
            if (r < nr && j < s_row[r] && u < s_tau[r]) atomicAdd(&h1[r][knn_bin(u, s_base[r])], 1u);
         }
      });
      __syncthreads();
      for (int r = wave; r < nr; r += kKnnThreads / 64) {
         const int b = knn_kth_bin(h1[r], K);  // the sample's K keys are below tau and counted again: never -1
         if (lane == 0) {
            s_bstar[r] = b;
            s_ok[r] = (h1[r][b] <= (unsigned)kKnnGather2) ? 1 : 0;
         }
      }
      __syncthreads();
      // collect
      knn_scan<P, R>(X, ldim, d, q, jmax, [&](int j, const double* acc) {
#pragma unroll
         for (int r = 0; r < R; r++) {
            const unsigned long long u = (unsigned long long)__double_as_longlong(acc[r]);
            if (r < nr && s_ok[r] && j < s_row[r] && u < s_tau[r]) {
               const int b = knn_bin(u, s_base[r]);
               if (b < s_bstar[r]) {
                  const int p = atomicAdd(&s_nsel[r], 1);
                  s_key[r][kKnnGather2 + p] = u;
                  s_idx[r][kKnnGather2 + p] = j;
               } else if (b == s_bstar[r]) {
                  const int p = atomicAdd(&s_ngat[r], 1);
                  s_key[r][p] = u;
                  s_idx[r][p] = j;
               }
            }
         }
      });
      __syncthreads();
      // rank the bin-b* keys by (key, index); the first K - below join (one wave per row)
      for (int r = wave; r < nr; r += kKnnThreads / 64) {
         if (!s_ok[r]) continue;
         const int ng = s_ngat[r], nsel0 = s_nsel[r];
         knn_rank(s_key[r], s_idx[r], ng, K - nsel0, lane, 64, [&](int rank, int e) {
            s_key[r][kKnnGather2 + nsel0 + rank] = s_key[r][e];
            s_idx[r][kKnnGather2 + nsel0 + rank] = s_idx[r][e];
         });
      }
      __syncthreads();
      for (int r = wave; r < nr; r += kKnnThreads / 64) {
         const int i = s_row[r];
         if (!s_ok[r]) {
            if (lane == 0) fail[atomicAdd(nfail, 1)] = i;
            continue;
         }
         const int row = ia[i];
         knn_rank_row(s_key[r] + kKnnGather2, s_idx[r] + kKnnGather2, K, K, lane, 64, ja + row);
         if (lane == 0) ja[row + K] = i;
      }
      __syncthreads();
   }
}

// The same pattern rows from fp32 screening keys: the scans of k_knn_bounded run on an fp32 copy of the
// points with the key of point j to row r kept as acc = -(|x_j|^2 + |q_r|^2) / 2 + x_j.q_r, so key~ =
// max(0, -2 acc) and "key~ < T" is the single compare acc > -T/2 against a workgroup-uniform value (one
// packed fp32 FMA per two (point, row) pairs per feature, half the bytes per point, 32 rows per workgroup;
// the fp64 scan spends a subtract and an FMA per pair per feature).  Only the few candidates left are
// ranked by the exact fp64 key sqdist() computes:
//   sample  two passes over points 0..S-1 (S = min(i0, 4096)): exponent histogram, then 16 bins per
//           octave below it; U = the upper end of the bin of the sample's (lfil-1)-th smallest key~, so
//           lfil-1 earlier points have key~ < U;
//   collect one pass over the earlier points (knn_stream_mfma): every point with key~ <= the row's limit,
//           which starts at U + 2 m, where m bounds |key~ - key| (below), and tightens as candidates arrive;
//   exact   one wave per row: key = sqdist's sum, rank the candidates by (key, index), the first lfil-1
//           are the row.
// |key~ - key| <= m: rounding the coordinates to fp32 moves sqrt(key) by at most u (|x_j| + |q|) (u =
// 2^-24); the fp32 norms, the start value and the d-term sum add at most (6 d + 6) u M^2, with M^2 =
// max_j |x_j|^2, so |key~ - key| <= (6 d + 15) u M^2; m = (8 d + 64) u M^2.  The lfil-1 points with key~ <
// U have key < U + m, so every true neighbour (key <= the (lfil-1)-th smallest) has key~ < U + 2 m in any
// scan and is collected; ranking the collected set by the exact key is therefore the exact selection, ties
// by index included.  A row with more than kScrCap candidates (duplicates, coordinates far from the origin
// against their spread) goes to `fail`; the host leaves every row to k_knn when M^2 is not finite.
constexpr int kScrRows = 32;  // one 32-row MFMA tile per workgroup
constexpr int kScrThreads = 512;
constexpr int kScrCap = 160;
constexpr int kScrSample = 4096;

// Xf = fp32 copy of X (column-major, leading dimension n, zero features d..dp-1), nx = fl32 squared norms,
// *m2 = bits of max nx
__global__ __launch_bounds__(256) void k_knn_prep(const double* __restrict__ X, int ldim, int n, int d, int dp,
                                                  float* __restrict__ Xf, float* __restrict__ nx,
                                                  unsigned int* __restrict__ m2)
{
   unsigned int mx = 0u;
   for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
      float a = 0.f;
      for (int c = 0; c < d; c++) {
         const float v = (float)X[(size_t)c * ldim + j];
         Xf[(size_t)c * n + j] = v;
         a = fmaf(v, v, a);
      }
      for (int c = d; c < dp; c++) Xf[(size_t)c * n + j] = 0.f;
      nx[j] = a;
      mx = max(mx, __float_as_uint(a));  // non-negative floats order like their bits (NaN above inf)
   }
   for (int off = 32; off > 0; off >>= 1) mx = max(mx, (unsigned int)__shfl_xor((int)mx, off, 64));
   if ((threadIdx.x & 63) == 0) atomicMax(m2, mx);
}

__device__ __forceinline__ int knn_bin32(unsigned int u, int base)
{
   const int e = (int)(u >> 23);
   return (e < base) ? 0 : (((e - base) << 4) | (int)((u >> 19) & 15u));
}

struct ScrShared {
   float q[kKnnMaxDims2][kScrRows];  // the rows' fp32 coordinates
   float nqh[kScrRows];              // -|q_r|^2 / 2
   union {
      unsigned int h[kScrRows][256];
      double key[kScrRows][kScrCap];
      float ck[kScrRows][kScrCap];  // the one-pass collect's candidate accumulators
   } u;
   int idx[kScrRows][kScrCap];
   float thr[kScrRows];  // -T_r / 2 of the current scan (rows beyond nr: +inf, never pass)
   int base[kScrRows], cnt[kScrRows];
   int row[kScrRows];    // the rows' indices (a row counts only points before it)
};

typedef float f32x16 __attribute__((ext_vector_type(16)));

// Value v of a 32 x 32 MFMA accumulator in lane l holds point l & 31 against this row of the tile (h = l >> 5)
__device__ __forceinline__ constexpr int mfma_row(int v, int h) { return (v & 3) + 8 * (v >> 2) + 4 * h; }

// One scan of the sample, points [0, j1), every one of them before all the rows, against the workgroup's 32 rows
// on v_mfma_f32_32x32x2_f32: each wave takes tiles of 32 points; the rows' coordinates are the A operand, held in
// registers for the whole scan (lane l: row l & 31, features 2s + (l >> 5)), the points' the B operand (one
// coalesced fp32 load per step), and the 32 x 32 accumulator starts at -(|x_j|^2 + |q_r|^2) / 2 (lane l: point
// l & 31, rows mfma_row(v, l >> 5) of its 16 values).  MODE 0: exponent histogram of every key~; MODE 1: the keys
// below the row's threshold binned 16 per octave from S.base.  STEPS = ceil(d / 2) bound.
template <int MODE, int STEPS>
__device__ __forceinline__ void knn_scan_mfma(ScrShared& S, const float* __restrict__ Xf,
                                              const float* __restrict__ nx, int n, int j1)
{
   constexpr int W = kScrThreads / 64, step = W * 32;
   const int lane = threadIdx.x & 63, h = lane >> 5, col = lane & 31, wave = threadIdx.x >> 6;
   float a[STEPS];
#pragma unroll
   for (int st = 0; st < STEPS; st++) a[st] = S.q[2 * st + h][col];  // zero beyond d
   float nqh[16], thr[16];
#pragma unroll
   for (int v = 0; v < 16; v++) {
      nqh[v] = S.nqh[mfma_row(v, h)];
      thr[v] = S.thr[mfma_row(v, h)];
   }
   // the loads run two tiles ahead of the MFMAs (software pipelining over the memory latency)
   float b0[STEPS], b1[STEPS], a00 = 0.f, a01 = 0.f;
   auto load = [&](int jb, float (&b)[STEPS], float& a0) {
      const int jl = min(jb + col, j1 - 1);  // a valid point for the lanes past the end (their keys are dropped)
      a0 = nx[jl];
#pragma unroll
      for (int st = 0; st < STEPS; st++) b[st] = Xf[(size_t)(2 * st + h) * n + jl];  // Xf zero-padded to 2 STEPS
   };
   if (wave * 32 < j1) load(wave * 32, b0, a00);
   if (wave * 32 + step < j1) load(wave * 32 + step, b1, a01);
   for (int jb = wave * 32; jb < j1; jb += step) {
      const bool ok = jb + col < j1;
      f32x16 c;
      float bc[STEPS];
#pragma unroll
      for (int v = 0; v < 16; v++) c[v] = fmaf(a00, -0.5f, nqh[v]);
#pragma unroll
      for (int st = 0; st < STEPS; st++) {
         bc[st] = b0[st];
         b0[st] = b1[st];
      }
      a00 = a01;
      if (jb + 2 * step < j1) load(jb + 2 * step, b1, a01);
#pragma unroll
      for (int st = 0; st < STEPS; st++) c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[st], bc[st], c, 0, 0, 0);
      if (!ok) continue;
      if (MODE == 0) {
#pragma unroll
         for (int v = 0; v < 16; v++) {
            if (c[v] < thr[v]) continue;  // rows beyond nr (thr +inf)
            atomicAdd(&S.u.h[mfma_row(v, h)][__float_as_uint(fmaxf(0.f, -2.f * c[v])) >> 23], 1u);
         }
         continue;
      }
      bool any = false;
#pragma unroll
      for (int v = 0; v < 16; v++) any |= c[v] > thr[v];
      if (!any) continue;
#pragma unroll
      for (int v = 0; v < 16; v++) {
         if (!(c[v] > thr[v])) continue;
         const int r = mfma_row(v, h);
         const float key = fmaxf(0.f, -2.f * c[v]);
         atomicAdd(&S.u.h[r][knn_bin32(__float_as_uint(key), S.base[r])], 1u);
      }
   }
}

// The one-pass collect: every point j in [j0, j1) with key~ <= the row's limit L (acc >= S.thr = -L/2)
// appends (j, acc) to the row's candidates, and at round boundaries the workgroup stops and each row holding
// more than `trigger` candidates tightens L to V + 2m, V = the (lfil-1)-th smallest key~ it holds, and drops
// the candidates above it.  Invariant: the candidates are every scanned point with key~ <= L, and L >= the
// true (lfil-1)-th smallest key + m (the lfil-1 candidates with key~ <= V have key <= V + m), so every true
// neighbour is still a candidate when the scan ends.  The boundaries fall every 16 rounds of 256 points up to
// 16384 points, then every quarter of the points seen, so the appends between two boundaries stay near
// (lfil - 1) / 4; a row that overflows kScrCap anyway goes to the fallback (cnt > kScrCap).  CHECK: only
// points before the row (j < S.row[r]) count.  The tile feed (loads two tiles ahead, accumulator start, MFMA
// chain) repeats knn_scan_mfma's on purpose: one shared feed taking the scans' bodies as callables compiled
// k_knn_screen<16> to 136 bytes of scratch per lane against 56 (profiles/knn_refactor_usage.txt).
template <bool CHECK, int STEPS>
__device__ __forceinline__ void knn_stream_mfma(ScrShared& S, const float* __restrict__ Xf,
                                                const float* __restrict__ nx, int n, int j0, int j1, int nr, int K,
                                                float margin2)
{
      constexpr int W = kScrThreads / 64, CAP = kScrCap;
   const int lane = threadIdx.x & 63, h = lane >> 5, col = lane & 31, wave = threadIdx.x >> 6;
   const int trigger = min(CAP - 48, max(64, 2 * K));
   float a[STEPS];
#pragma unroll
   for (int st = 0; st < STEPS; st++) a[st] = S.q[2 * st + h][col];
   float nqh[16], thr[16];
   int rlim[16];
#pragma unroll
   for (int v = 0; v < 16; v++) {
      const int r = mfma_row(v, h);
      nqh[v] = S.nqh[r];
      thr[v] = S.thr[r];
      rlim[v] = CHECK ? S.row[r] : 0;
   }
   float b0[STEPS], b1[STEPS], a00 = 0.f, a01 = 0.f;
   auto load = [&](int jb, float (&b)[STEPS], float& a0) {
      const int jl = min(jb + col, j1 - 1);
      a0 = nx[jl];
#pragma unroll
      for (int st = 0; st < STEPS; st++) b[st] = Xf[(size_t)(2 * st + h) * n + jl];
   };
   constexpr int step = W * 32;
   const int nrounds = (j1 - j0 + step - 1) / step;  // workgroup-uniform: every wave meets every boundary
   if (j0 + wave * 32 < j1) load(j0 + wave * 32, b0, a00);
   if (j0 + wave * 32 + step < j1) load(j0 + wave * 32 + step, b1, a01);
   int next = 16;  // the round after which the next boundary falls
   for (int k = 0; k < nrounds; k++) {
      const int jb = j0 + wave * 32 + k * step;
      if (jb < j1) {
         const int j = jb + col;
         const bool ok = j < j1;
         f32x16 c;
         float bc[STEPS];
#pragma unroll
         for (int v = 0; v < 16; v++) c[v] = fmaf(a00, -0.5f, nqh[v]);
#pragma unroll
         for (int st = 0; st < STEPS; st++) {
            bc[st] = b0[st];
            b0[st] = b1[st];
         }
         a00 = a01;
         if (jb + 2 * step < j1) load(jb + 2 * step, b1, a01);
#pragma unroll
         for (int st = 0; st < STEPS; st++) c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[st], bc[st], c, 0, 0, 0);
         bool any = false;
#pragma unroll
         for (int v = 0; v < 16; v++) any |= c[v] >= thr[v];
         if (ok && any) {
#pragma unroll
            for (int v = 0; v < 16; v++) {
               const int r = mfma_row(v, h);
               if (!(c[v] >= thr[v]) || (CHECK && j >= rlim[v])) continue;
               const int slot = atomicAdd(&S.cnt[r], 1);
               if (slot < CAP) {
                  S.idx[r][slot] = j;
                  S.u.ck[r][slot] = c[v];
               }
            }
         }
      }
      if (k + 1 != next || k + 1 == nrounds) continue;
      next = (k + 1 < 64) ? k + 17 : k + 1 + (k + 1) / 4;
      __syncthreads();
      for (int r = wave; r < nr; r += W) {
         const int cnt = S.cnt[r];
         if (cnt <= trigger || cnt > CAP) continue;
         // V = the K-th smallest key~ held: the largest key~ of rank < K (rank = the number strictly below)
         float vmax = 0.f;
         for (int e = lane; e < cnt; e += 64) {
            const float ke = fmaxf(0.f, -2.f * S.u.ck[r][e]);
            int rank = 0;
            for (int o = 0; o < cnt; o++) rank += (fmaxf(0.f, -2.f * S.u.ck[r][o]) < ke) ? 1 : 0;
            if (rank < K) vmax = fmaxf(vmax, ke);
         }
         for (int off = 32; off > 0; off >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, off, 64));
         const float tnew = -0.5f * ((vmax + margin2) * 1.000001f);
         if (!(tnew > S.thr[r])) continue;  // wave-uniform
         // keep acc >= tnew, in order (the writes of a 64-chunk land at or below its reads)
         int kept = 0;
         for (int e0 = 0; e0 < cnt; e0 += 64) {
            const int e = e0 + lane;
            const float ce = e < cnt ? S.u.ck[r][e] : 0.f;
            const int je = e < cnt ? S.idx[r][e] : 0;
            const bool keep = e < cnt && ce >= tnew;
            const unsigned long long m = __ballot(keep);
            const int pos = kept + __popcll(m & ((1ull << lane) - 1ull));
            if (keep) {
               S.u.ck[r][pos] = ce;
               S.idx[r][pos] = je;
            }
            kept += __popcll(m);
         }
         if (lane == 0) {
            S.cnt[r] = kept;
            S.thr[r] = tnew;
         }
      }
      __syncthreads();
#pragma unroll
      for (int v = 0; v < 16; v++) thr[v] = S.thr[mfma_row(v, h)];
   }
}

// The 32-row screen in one launch: the sample, then the one-pass collect above from the sample's limit
// U + 2m, exact keys, rank.  Compiled for 2 waves per SIMD: the stream's registers (two tiles of loads in
// flight beside the accumulator) do not fit more, and a third wave's spills cost more than it hides.
template <int STEPS>
__global__ __launch_bounds__(kScrThreads, 2) void k_knn_screen(const double* __restrict__ X, int ldim,
                                                               const float* __restrict__ Xf,
                                                               const float* __restrict__ nx, int n, int d, int lfil,
                                                               float margin2, const int* __restrict__ ia,
                                                               int* __restrict__ ja, int* __restrict__ fail,
                                                               int* __restrict__ nfail, const int* __restrict__ rows,
                                                               int nrows_list)
{
   constexpr int R = kScrRows, CAP = kScrCap, W = kScrThreads / 64;
   __shared__ ScrShared S;
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
   const int K = lfil - 1;
   // rows (ascending, all >= lfil; nrows_list of them) instead of lfil .. n-1: a row shard's own rows
   const int nall = rows ? nrows_list : n - lfil;
   const int ngroups = (nall + R - 1) / R;
   const float inf = __int_as_float(0x7f800000);
   // a row whose histogram holds fewer than K keys (the scans' roundings may differ) goes to the fallback
   auto give_up = [&](int r) {  // lane 0 of the row's wave
      S.thr[r] = inf;
      S.cnt[r] = CAP + 1;
   };
   // upper end of bin b of the 16-per-octave bins from base (bin 0 also holds every exponent below base)
   auto bin_top = [](int base, int b) {
      const int e = base + (b >> 4);
      return (e < 0) ? 0.f : __uint_as_float(((unsigned)e << 23) + ((unsigned)((b & 15) + 1) << 19));
   };
   auto clear_h = [&]() {
      for (int e = tid; e < R * 256; e += kScrThreads) S.u.h[e / 256][e % 256] = 0u;
   };
   for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
      const int lp0 = g * R;  // list position of the group's first row
      const int nr = min(R, nall - lp0);
      const int i0 = rows ? rows[lp0] : lfil + lp0;
      const int ilast = rows ? rows[lp0 + nr - 1] : i0 + nr - 1;
      auto row_of = [&](int r) { return rows ? rows[lp0 + r] : i0 + r; };
      for (int e = tid; e < R * 2 * STEPS; e += kScrThreads) {
         const int r = e % R, c = e / R;
         S.q[c][r] = (r < nr) ? Xf[(size_t)c * n + row_of(r)] : 0.f;
      }
      clear_h();
      if (tid < R) {
         S.row[tid] = tid < nr ? row_of(tid) : 0;
         S.nqh[tid] = (tid < nr) ? -0.5f * nx[row_of(tid)] : 0.f;
         S.cnt[tid] = 0;
         S.thr[tid] = (tid < nr) ? -inf : inf;
      }
      __syncthreads();
      const int Sn = min(i0, kScrSample);
      knn_scan_mfma<0, STEPS>(S, Xf, nx, n, Sn);
      __syncthreads();
      for (int r = wave; r < nr; r += W) {
         const int b = knn_kth_bin(S.u.h[r], K);  // exponent bin: keys there are below 2^(b - 126)
         if (lane == 0 && b < 0) give_up(r);
         if (lane == 0 && b >= 0) {
            S.thr[r] = (b == 255) ? -inf : -0.5f * __uint_as_float((unsigned)(b + 1) << 23);
            S.base[r] = ((b == 255) ? 255 : b + 1) - 16;
         }
      }
      __syncthreads();
      clear_h();
      __syncthreads();
      knn_scan_mfma<1, STEPS>(S, Xf, nx, n, Sn);
      __syncthreads();
      for (int r = wave; r < nr; r += W) {
         const int b = knn_kth_bin(S.u.h[r], K);
         if (lane == 0 && b < 0 && S.thr[r] != inf) give_up(r);
         if (lane == 0 && b >= 0) {
            // the sample's limit U + 2m (thr = -U / 2 here; inf: gave up, -inf: U = inf)
            const float U = (S.thr[r] == -inf) ? inf : bin_top(S.base[r], b);
            S.thr[r] = (U == inf) ? -inf : -0.5f * ((U + margin2) * 1.000001f);
         }
      }
      __syncthreads();
      // the earlier points: [0, i0) before all rows, [i0, ilast) before some
      knn_stream_mfma<false, STEPS>(S, Xf, nx, n, 0, i0, nr, K, margin2);
      knn_stream_mfma<true, STEPS>(S, Xf, nx, n, i0, ilast, nr, K, margin2);
      __syncthreads();
      // exact keys of the candidates (the histogram space is free now)
      for (int r = wave; r < nr; r += W) {
         const int i = S.row[r], cnt = S.cnt[r];
         if (cnt > CAP || cnt < K) continue;
         for (int e = lane; e < cnt; e += 64) {
            const int j = S.idx[r][e];
            double a = 0.0;
            for (int c = 0; c < d; c++) {
               const double t = X[(size_t)c * ldim + j] - X[(size_t)c * ldim + i];
               a = fma(t, t, a);
            }
            S.u.key[r][e] = a;
         }
      }
      __syncthreads();
      for (int r = wave; r < nr; r += W) {
         const int i = S.row[r], cnt = S.cnt[r];
         if (cnt > CAP || cnt < K) {
            if (lane == 0) fail[atomicAdd(nfail, 1)] = i;
            continue;
         }
         const int row = ia[i];
         knn_rank_row(S.u.key[r], S.idx[r], cnt, K, lane, 64, ja + row);
         if (lane == 0) ja[row + K] = i;
      }
      __syncthreads();
   }
}

// ---- the one-launch tiled screen (variant 4, the default for d <= 32 and lfil <= 25) ----
// 256 rows per workgroup, 32 per wave; the earlier points stream once through LDS in stages of 64, each
// stage read by all eight waves, so the HBM / L2 traffic per (point, row) pair is an eighth of the
// 32-row screens'.  key~ comes from v_mfma_f32_32x32x16_bf16 on a three-term bf16 split of the
// coordinates: x = xh + xl + ex with xh = bf16(x), xl = bf16(x - xh), |ex| <= 2^-18 |x|, and
// x.q ~ xh.qh + xh.ql + xl.qh (bf16 products are exact in fp32).  Error of key~ = |x|^2 + |q|^2 - 2 x.q
// (fp32 norms of the fp32-rounded coordinates, as the 32-row screens):
//   split       2 * 3.02 * 2^-18 |x||q|                     <= 387 * 2^-24 M^2
//   MFMA sums   2 * 3d additions of partial sums <= 2.02 M^2 <= 12.2 d * 2^-24 M^2 (one fp32 rounding each)
//   norms       2 (d + 2) * 2^-24 M^2, start value 4 * 2^-24 M^2
// so |key~ - key| <= (14.2 d + 395) 2^-24 M^2 and m = (16 d + 448) 2^-24 M^2 (M^2 = max |x_j|^2 >= 2^-60, so
// bf16 subnormal flushes stay far below it).  Each row keeps its candidates (index, acc) in LDS, at most
// kTileCap: it starts accepting every earlier point; whenever a row holds more than kTileCap - 32 after a
// 32-point tile, its wave tightens the row's limit to V + 2m (V = the (lfil-1)-th smallest key~ held) and
// drops the candidates above it (the invariant of knn_stream_mfma), so a tile can never overflow a row that
// the limit has settled; rows that overflow anyway (many equal keys) go to the fallback.  The rows are the
// wave's own, so the selections need no barrier; the exact fp64 keys and the (key, index) ranking run on
// one candidate per lane.
constexpr int kTileRows = 256;
constexpr int kTileCap = 64;
constexpr int kTileStep = 64;  // Xb's padding: n rounded up to 64 points
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct TileShared {
   int idx[kTileRows][kTileCap];
   float ck[kTileRows][kTileCap];
   float thr[kTileRows];
   int cnt[kTileRows];
   int row[kTileRows];
};

__device__ __forceinline__ unsigned int bf16_rn(float f)  // bits of the nearest bf16 (finite f)
{
   const unsigned int u = __float_as_uint(f);
   return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// Xb: per 32-point block, [chunk KCH][hi, lo][half][point 32] x 16 B (features 16 ch + 8 half + 0..7),
// zero past d and past n; nx = fp32 squared norms (+inf past n, so padded points never pass); *m2 = bits
// of max nx over the n points.  npad = n rounded up to kTileStep.
template <int KCH>
__global__ __launch_bounds__(256) void k_knn_prep_bf(const double* __restrict__ X, int ldim, int n, int npad, int d,
                                                     uint4* __restrict__ Xb, float* __restrict__ nx,
                                                     unsigned int* __restrict__ m2)
{
   constexpr int BLK = KCH * 2 * 2 * 32;
   unsigned int mx = 0u;
   for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < npad; j += gridDim.x * blockDim.x) {
      float a = 0.f;
      uint4* blk = Xb + (size_t)(j >> 5) * BLK + (j & 31);
#pragma unroll
      for (int ch = 0; ch < KCH; ch++) {
#pragma unroll
         for (int half = 0; half < 2; half++) {
            unsigned int hw[4] = {0u, 0u, 0u, 0u}, lw[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int e = 0; e < 8; e++) {
               const int c = 16 * ch + 8 * half + e;
               const double x = (j < n && c < d) ? X[(size_t)c * ldim + j] : 0.0;
               const float f = (float)x;
               a = fmaf(f, f, a);
               const unsigned int hb = bf16_rn(f);
               const unsigned int lb = bf16_rn((float)(x - (double)__uint_as_float(hb << 16)));
               hw[e >> 1] |= hb << (16 * (e & 1));
               lw[e >> 1] |= lb << (16 * (e & 1));
            }
            blk[((ch * 2 + 0) * 2 + half) * 32] = make_uint4(hw[0], hw[1], hw[2], hw[3]);
            blk[((ch * 2 + 1) * 2 + half) * 32] = make_uint4(lw[0], lw[1], lw[2], lw[3]);
         }
      }
      nx[j] = j < n ? a : __int_as_float(0x7f800000);
      if (j < n) mx = max(mx, __float_as_uint(a));
   }
   for (int off = 32; off > 0; off >>= 1) mx = max(mx, (unsigned int)__shfl_xor((int)mx, off, 64));
   if ((threadIdx.x & 63) == 0) atomicMax(m2, mx);
}

// Every wave loads its B fragments from global memory itself (the eight waves read the same lines close
// together: L1 / L2 hits), two tiles ahead in registers -- no LDS stages and no barriers in the scan (an
// LDS-staged scan with a barrier per 64 points, loads four stages ahead, measured 0.221 s against 0.174 s at
// n = 1e6, d = 32, and was removed)
template <int KCH>
__global__ __launch_bounds__(512, 2) void k_knn_tile(const double* __restrict__ X, int ldim,
                                                     const uint4* __restrict__ Xb, const float* __restrict__ nx,
                                                     int n, int d, int lfil, float margin2,
                                                     const int* __restrict__ ia, int* __restrict__ ja,
                                                     int* __restrict__ fail, int* __restrict__ nfail,
                                                     const int* __restrict__ rows, int nrows_list)
{
   constexpr int R = kTileRows, CAP = kTileCap, BLK = KCH * 2 * 2 * 32;
   __shared__ TileShared S;
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
   const int K = lfil - 1;
   const int nall = rows ? nrows_list : n - lfil;
   const int ngroups = (nall + R - 1) / R;
   const float inf = __int_as_float(0x7f800000);
   for (int gi = blockIdx.x; gi < ngroups; gi += gridDim.x) {
      const int g = ngroups - 1 - gi;  // the longest scans first
      const int lp0 = g * R, nr = min(R, nall - lp0);
      auto row_of = [&](int r) { return rows ? rows[lp0 + r] : lfil + lp0 + r; };
      const int ilast = row_of(nr - 1);  // the rows see points [0, ilast) at most
      if (tid < R) {
         S.row[tid] = tid < nr ? row_of(tid) : 0;
         S.cnt[tid] = 0;
         S.thr[tid] = tid < nr ? -__FLT_MAX__ : inf;
      }
      // the wave's 32 rows as the A operand (lane: row 32 wave + col, features 8 h + 0..7 of each chunk)
      const int iA = (32 * wave + col < nr) ? row_of(32 * wave + col) : row_of(0);
      bf16x8 ah[KCH], al[KCH];
      {
         const uint4* blk = Xb + (size_t)(iA >> 5) * BLK + (iA & 31);
#pragma unroll
         for (int ch = 0; ch < KCH; ch++) {
            const uint4 hv = blk[((ch * 2 + 0) * 2 + h) * 32], lv = blk[((ch * 2 + 1) * 2 + h) * 32];
            ah[ch] = __builtin_bit_cast(bf16x8, hv);
            al[ch] = __builtin_bit_cast(bf16x8, lv);
         }
      }
      float nqh[16], thr[16];
      int rlim[16];
#pragma unroll
      for (int v = 0; v < 16; v++) {
         const int r = 32 * wave + mfma_row(v, h);
         nqh[v] = r < nr ? -0.5f * nx[row_of(r)] : 0.f;
         rlim[v] = r < nr ? row_of(r) : 0;
      }
      const int rowmin = row_of(0);
      const unsigned long long below = (1ull << lane) - 1ull;
      int cntv = 0;  // lane l < 32: candidates of the wave's row l
      __syncthreads();
#pragma unroll
      for (int v = 0; v < 16; v++) thr[v] = S.thr[32 * wave + mfma_row(v, h)];
      // test a tile's keys against the rows' limits (points j0 + col), append, tighten
      auto test_tile = [&](const f32x16& c, int j0) {
         const int j = j0 + col;
         // per group of 4 rows of the lane (v = 4 g .. 4 g + 3) the largest margin; NaN keys drop out
         float mg[4];
#pragma unroll
         for (int g = 0; g < 4; g++)
            mg[g] = fmaxf(fmaxf(c[4 * g] - thr[4 * g], c[4 * g + 1] - thr[4 * g + 1]),
                          fmaxf(c[4 * g + 2] - thr[4 * g + 2], c[4 * g + 3] - thr[4 * g + 3]));
         const float mx = fmaxf(fmaxf(mg[0], mg[1]), fmaxf(mg[2], mg[3]));
         if (!__ballot(mx >= 0.f)) return;
         // append: the wave owns its rows, so each (v, lane half) pair's slots come from one ballot
         // (lanes 0-31: row rl = (v & 3) + 8 (v >> 2), lanes 32-63: rl + 4) and the counts live in cntv
         // a point at or after a row never counts for it (rlim: the lane's 16 rows' indices; jj = -1 while
         // every point of the tile precedes every row)
         const int jj = (j0 + 31 < rowmin) ? -1 : j;
#pragma unroll
         for (int g = 0; g < 4; g++) {
            if (!__ballot(mg[g] >= 0.f)) continue;  // no lane passes in this group of 4 rows
#pragma unroll
            for (int vv = 0; vv < 4; vv++) {
               const int v = 4 * g + vv;
               const int rl = mfma_row(v, 0);
               const bool pass = c[v] >= thr[v] && jj < rlim[v];
               const unsigned long long m = __ballot(pass);
               if (!m) continue;
               const unsigned int mlo = (unsigned int)m, mhi = (unsigned int)(m >> 32);
               const int blo = __builtin_amdgcn_readlane(cntv, rl), bhi = __builtin_amdgcn_readlane(cntv, rl + 4);
               if (pass) {
                  const int base = h ? bhi : blo;
                  const int pos = base + __popcll(m & below) - (h ? __popc(mlo) : 0);
                  if (pos < CAP) {
                     S.idx[32 * wave + rl + 4 * h][pos] = j;
                     S.ck[32 * wave + rl + 4 * h][pos] = c[v];
                  }
               }
               cntv += (lane == rl) ? __popc(mlo) : (lane == rl + 4) ? __popc(mhi) : 0;
            }
         }
         // the wave's rows that another tile could overflow: tighten them (wave-uniform loop)
         unsigned long long todo = __ballot(lane < 32 && cntv > CAP - 32);
         if (!todo) return;
         while (todo) {
            const int rl = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int r = 32 * wave + rl;
            const int cnt = __builtin_amdgcn_readlane(cntv, rl);
            if (cnt > CAP) {  // overflowed: the fallback takes the row
               if (lane == 0) S.thr[r] = inf;
               continue;
            }
            const float ce = lane < cnt ? S.ck[r][lane] : -inf;
            const int je = lane < cnt ? S.idx[r][lane] : 0;
            const float ke = lane < cnt ? fmaxf(0.f, -2.f * ce) : inf;
            int rank = 0;
            for (int o = 0; o < cnt; o++)
               rank += (__int_as_float(__builtin_amdgcn_readlane(__float_as_int(ke), o)) < ke) ? 1 : 0;
            float vk = (lane < cnt && rank < K) ? ke : 0.f;
            for (int off = 32; off > 0; off >>= 1) vk = fmaxf(vk, __shfl_xor(vk, off, 64));
            const float tnew = -0.5f * ((vk + margin2) * 1.000001f);
            if (!(tnew > S.thr[r])) continue;
            const bool keep = lane < cnt && ce >= tnew;
            const unsigned long long m = __ballot(keep);
            if (keep) {
               const int pos = __popcll(m & ((1ull << lane) - 1ull));
               S.ck[r][pos] = ce;
               S.idx[r][pos] = je;
            }
            if (lane == rl) cntv = __popcll(m);
            if (lane == 0) S.thr[r] = tnew;
         }
#pragma unroll
         for (int v = 0; v < 16; v++) thr[v] = S.thr[32 * wave + mfma_row(v, h)];
      };
      // software pipeline: a tile's tests run under the next tile's MFMAs (c1 carries the previous tile)
      f32x16 c0, c1;
      {
         const int ntl = (ilast + 31) / 32;  // 32-point tiles
         uint4 bh0[KCH], bl0[KCH], bh1[KCH], bl1[KCH];
         float nx0, nx1;
         auto fetchf = [&](int t, uint4 (&fh)[KCH], uint4 (&fl)[KCH], float& fn) {
            t = min(t, ntl - 1);
            const uint4* blk = Xb + (size_t)t * BLK + col;
#pragma unroll
            for (int ch = 0; ch < KCH; ch++) {
               fh[ch] = blk[((ch * 2 + 0) * 2 + h) * 32];
               fl[ch] = blk[((ch * 2 + 1) * 2 + h) * 32];
            }
            fn = nx[(size_t)t * 32 + col];
         };
         auto mfma_frag = [&](const uint4 (&fh)[KCH], const uint4 (&fl)[KCH], float fn) {
            f32x16 c;
#pragma unroll
            for (int v = 0; v < 16; v++) c[v] = fmaf(fn, -0.5f, nqh[v]);
#pragma unroll
            for (int ch = 0; ch < KCH; ch++) {
               const bf16x8 bh = __builtin_bit_cast(bf16x8, fh[ch]), bl = __builtin_bit_cast(bf16x8, fl[ch]);
               c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[ch], bl, c, 0, 0, 0);
               c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[ch], bh, c, 0, 0, 0);
               c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[ch], bh, c, 0, 0, 0);
            }
            return c;
         };
         fetchf(0, bh0, bl0, nx0);
         fetchf(1, bh1, bl1, nx1);
         for (int t0 = 0; t0 < ntl; t0 += 2) {
            c0 = mfma_frag(bh0, bl0, nx0);
            fetchf(t0 + 2, bh0, bl0, nx0);
            if (t0 > 0) test_tile(c1, t0 * 32 - 32);
            if (t0 + 1 < ntl) {
               c1 = mfma_frag(bh1, bl1, nx1);
               fetchf(t0 + 3, bh1, bl1, nx1);
            }
            test_tile(c0, t0 * 32);
         }
         if (ntl % 2 == 0) test_tile(c1, (ntl - 1) * 32);
      }
      if (lane < 32) S.cnt[32 * wave + lane] = cntv;
      // exact fp64 keys of the candidates (one per lane) and the (key, index) ranking; the wave's rows
      for (int rl = 0; rl < 32; rl++) {
         const int r = 32 * wave + rl;
         if (r >= nr) break;
         const int i = S.row[r], cnt = S.cnt[r];
         if (cnt > CAP || cnt < K) {
            if (lane == 0) fail[atomicAdd(nfail, 1)] = i;
            continue;
         }
         double ke = 0.0;
         int ie = 0x7fffffff;
         if (lane < cnt) {
            ie = S.idx[r][lane];
            for (int c = 0; c < d; c++) {
               const double t = X[(size_t)c * ldim + ie] - X[(size_t)c * ldim + i];
               ke = fma(t, t, ke);
            }
         }
         int rank = 0;
         for (int o = 0; o < cnt; o++) {
            const double ko = __shfl(ke, o, 64);
            const int io = __builtin_amdgcn_readlane(ie, o);
            rank += (ko < ke || (ko == ke && io < ie)) ? 1 : 0;
         }
         const int rp = ia[i];
         if (lane < cnt && rank < K) ja[rp + rank] = ie;
         if (lane == 0) ja[rp + K] = i;
      }
      __syncthreads();
   }
}

// ---- the cascade ----
// The host side: one function per stage.  A stage takes the job, the rows to settle and -- all but the radix
// select -- a fail list it appends the rows it could not settle to; it returns how many those are, -1 on an
// error, or kNotApplicable (nothing launched) when its preconditions on d, lfil and the data do not hold.
constexpr int kNotApplicable = -2;

struct KnnJob {
   const double* X;
   int n, ldim, d, lfil;
   const int* ia;
   int* ja;
   hipStream_t s;
};

struct RowList {  // device; rows == nullptr: all rows lfil .. n-1 (count of them)
   const int* rows;
   int count;
};

struct FailList {  // device: rows[0 .. *count); m2 = count + 1, the word a screen's prep leaves the max norm's bits in
   int* rows;
   int* count;
   unsigned int* m2() const { return (unsigned int*)(count + 1); }
};

// device buffers that live as long as the scope: freed on every exit, after the stream's work
struct DeviceScope {
   hipStream_t s;
   std::vector<void*> held;
   explicit DeviceScope(hipStream_t stream) : s(stream) {}
   DeviceScope(const DeviceScope&) = delete;
   DeviceScope& operator=(const DeviceScope&) = delete;
   ~DeviceScope()
   {
      (void)hipStreamSynchronize(s);
      for (void* p : held) (void)hipFree(p);
   }
   template <class T>
   T* alloc(size_t count)
   {
      void* p = nullptr;
      if (hipMalloc(&p, sizeof(T) * std::max<size_t>(1, count)) != hipSuccess) return nullptr;
      held.push_back(p);
      return (T*)p;
   }
};

int fail_reset(const FailList& fail, hipStream_t s)
{
   return hipMemsetAsync(fail.count, 0, 2 * sizeof(int), s) == hipSuccess ? 0 : -1;
}

// the number of rows the stage just launched left in the fail list, or -1
int fail_count(const FailList& fail, hipStream_t s)
{
   int nfail = -1;
   if (hipGetLastError() != hipSuccess ||
       hipMemcpyAsync(&nfail, fail.count, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
       hipStreamSynchronize(s) != hipSuccess)
      return -1;
   return nfail;
}

// A screen's prep: launch(m2 word) runs its prep kernel; M^2 = max_j |x_j|^2 comes back, and margin2 = 2 m for
// the screen's m = coeff * 2^-24 * M^2 (with the slack the kernels' own roundings of it need).  0, -1, or
// kNotApplicable when M^2 < min_m2 or either is not finite.
template <class Launch>
int knn_prep(const FailList& fail, hipStream_t s, double coeff, float min_m2, Launch&& launch, float* margin2)
{
   if (fail_reset(fail, s)) return -1;
   launch(fail.m2());
   float m2 = 0.f;
   if (hipGetLastError() != hipSuccess ||
       hipMemcpyAsync(&m2, fail.m2(), sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess ||
       hipStreamSynchronize(s) != hipSuccess)
      return -1;
   const double margin = coeff * std::ldexp(1.0, -24) * (double)m2;
   if (!std::isfinite(m2) || !(m2 >= min_m2) || !std::isfinite((float)(2.0 * margin))) return kNotApplicable;
   *margin2 = (float)(2.0 * margin) * 1.0001f;
   return 0;
}

// the radix select: settles every row of `in`
int knn_stage_select(const KnnJob& J, const RowList& in)
{
   hipLaunchKernelGGL(k_knn, dim3(std::min(in.count, 4096)), dim3(kKnnThreads), 0, J.s, J.X, J.ldim, J.n, J.d, J.lfil,
                      J.ia, J.ja, in.rows, in.count);
   return hipGetLastError() == hipSuccess ? 0 : -1;
}

// the fp64 bounded scan (d <= kKnnMaxDims2; the cascade sends larger d to the radix select)
int knn_stage_bounded(const KnnJob& J, const RowList& in, const FailList& fail)
{
   if (fail_reset(fail, J.s)) return -1;
   const int ngroups = (in.count + kKnnRows - 1) / kKnnRows;
   // 2 points per thread: 5.6 -> 4.0 s for the n = 1e6, d = 32, lfil = 20 setup; 4 drop to 1 wave per SIMD
   hipLaunchKernelGGL(k_knn_bounded<kKnnPoints>, dim3(std::min(ngroups, 8192)), dim3(kKnnThreads), 0, J.s, J.X, J.ldim,
                      J.n, J.d, J.lfil, J.ia, J.ja, fail.rows, fail.count, in.rows, in.count);
   return fail_count(fail, J.s);
}

// the 32-row screen: any d <= kKnnMaxDims2 and lfil, finite data
int knn_stage_screen(const KnnJob& J, const RowList& in, const FailList& fail)
{
   const int n = J.n, d = J.d;
   const int steps = d <= 4 ? 2 : d <= 8 ? 4 : d <= 16 ? 8 : d <= 32 ? 16 : 32;
   DeviceScope mem(J.s);
   float* Xf = mem.alloc<float>((size_t)n * 2 * steps);
   float* nx = mem.alloc<float>((size_t)n);
   if (!Xf || !nx) return -1;
   float margin2 = 0.f;
   const int rc = knn_prep(fail, J.s, 8.0 * d + 64.0, 0.f, [&](unsigned int* m2) {
      hipLaunchKernelGGL(k_knn_prep, dim3(std::min((n + 255) / 256, 4096)), dim3(256), 0, J.s, J.X, J.ldim, n, d,
                         2 * steps, Xf, nx, m2);
   }, &margin2);
   if (rc) return rc;
   const int ngroups = (in.count + kScrRows - 1) / kScrRows;
   auto screen = steps == 2    ? k_knn_screen<2>
                 : steps == 4  ? k_knn_screen<4>
                 : steps == 8  ? k_knn_screen<8>
                 : steps == 16 ? k_knn_screen<16>
                               : k_knn_screen<32>;
   hipLaunchKernelGGL(screen, dim3(std::min(ngroups, 4096)), dim3(kScrThreads), 0, J.s, J.X, J.ldim, (const float*)Xf,
                      (const float*)nx, n, d, J.lfil, margin2, J.ia, J.ja, fail.rows, fail.count, in.rows, in.count);
   return fail_count(fail, J.s);
}

// the tile screen: d <= 32, lfil <= 25, and M^2 >= 2^-60 so that the bf16 split's subnormal flushes stay below m
int knn_stage_tile(const KnnJob& J, const RowList& in, const FailList& fail)
{
   const int n = J.n, d = J.d;
   if (d > 32 || J.lfil > 25) return kNotApplicable;
   const int kch = d <= 16 ? 1 : 2;
   const int npad = (n + kTileStep - 1) / kTileStep * kTileStep;
   DeviceScope mem(J.s);
   uint4* Xb = mem.alloc<uint4>((size_t)npad * kch * 4);
   float* nx = mem.alloc<float>((size_t)npad);
   if (!Xb || !nx) return -1;
   float margin2 = 0.f;
   const int rc = knn_prep(fail, J.s, 16.0 * d + 448.0, std::ldexp(1.0f, -60), [&](unsigned int* m2) {
      auto prep = kch == 1 ? k_knn_prep_bf<1> : k_knn_prep_bf<2>;
      hipLaunchKernelGGL(prep, dim3(std::min((npad + 255) / 256, 4096)), dim3(256), 0, J.s, J.X, J.ldim, n, npad, d, Xb,
                         nx, m2);
   }, &margin2);
   if (rc) return rc;
   const int ngroups = (in.count + kTileRows - 1) / kTileRows;
   auto tile = kch == 1 ? k_knn_tile<1> : k_knn_tile<2>;
   hipLaunchKernelGGL(tile, dim3(std::min(ngroups, 65535)), dim3(kScrThreads), 0, J.s, J.X, J.ldim, (const uint4*)Xb,
                      (const float*)nx, n, d, J.lfil, margin2, J.ia, J.ja, fail.rows, fail.count, in.rows, in.count);
   return fail_count(fail, J.s);
}

// NFFT4GP_AMD_KNN names a variant (0, 2, 3 or 4); anything else, the retired 1 included, is the default
int knn_default_variant()
{
   const char* e = getenv("NFFT4GP_AMD_KNN");
   if (e && e[0] && !e[1] && (e[0] == '0' || e[0] == '2' || e[0] == '3')) return e[0] - '0';
   return 4;
}

}  // namespace

namespace nfft4gp_amd {

// The cascade.  The first stage is the variant's: 4 the tile screen, which hands over to the 32-row screen
// where it does not apply; 3 the 32-row screen; 0 the bounded scan; 2 the radix select.  The rows a screen
// leaves go to the bounded scan, in ascending order, when they are more than 64 (clustered data far from the
// origin against its spread), and the rest to the radix select, which also takes every row when no other stage
// applies (d > 64, non-finite data).
int knn_pattern(const double* dX, int n, int ldim, int d, int lfil, const int* dia, int* dja, hipStream_t s,
                int variant, const int* d_rows, int nrows_list)
{
   if (variant < 0) variant = knn_default_variant();
   if (variant != 0 && variant != 2 && variant != 3 && variant != 4) return -1;
   if (n <= lfil || (d_rows && nrows_list <= 0)) return 0;
   const KnnJob J{dX, n, ldim, d, lfil, dia, dja, s};
   const RowList all{d_rows, d_rows ? nrows_list : n - lfil};
   if (variant == 2 || d > kKnnMaxDims2) return knn_stage_select(J, all) ? -1 : all.count;
   DeviceScope mem(s);
   int* fbuf = mem.alloc<int>((size_t)all.count + 2);
   if (!fbuf) return -1;
   const FailList fail{fbuf, fbuf + all.count};
   int left = kNotApplicable;
   if (variant == 4) left = knn_stage_tile(J, all, fail);
   if (variant != 0 && left == kNotApplicable) left = knn_stage_screen(J, all, fail);
   if (variant == 0) left = knn_stage_bounded(J, all, fail);
   if (left == kNotApplicable) return knn_stage_select(J, all) ? -1 : all.count;
   if (left < 0) return -1;
   int rest = left;
   if (variant != 0 && left > 64) {
      std::vector<int> hrows(left);
      if (hipMemcpy(hrows.data(), fail.rows, sizeof(int) * left, hipMemcpyDeviceToHost) != hipSuccess) return -1;
      std::sort(hrows.begin(), hrows.end());
      int* drows = mem.alloc<int>(hrows.size());
      if (!drows || hipMemcpy(drows, hrows.data(), sizeof(int) * left, hipMemcpyHostToDevice) != hipSuccess) return -1;
      rest = knn_stage_bounded(J, RowList{drows, left}, fail);
      if (rest < 0) return -1;
   }
   if (rest > 0 && knn_stage_select(J, RowList{fail.rows, rest})) return -1;
   return left;
}

}  // namespace nfft4gp_amd

extern "C" {

// Test hook: the KNN pattern (lfil column indices per row) of the host points X (n x d, leading dimension
// ldim) with the given variant (knn_pattern; negative: the default): rows lfil..n-1, or the rows of `rows`
// (nrows of them, ascending, each >= lfil) in list order; *nfail = knn_pattern's return value.  -1, with ja_out
// untouched, on an error or an unknown variant.
int Nfft4GPAmdDebugKnn(const double* X, int n, int ldim, int d, int lfil, int variant, int* ja_out, int* nfail,
                       const int* rows, int nrows)
{
   if (n <= lfil || lfil < 1 || lfil > kFsaiMaxK || d <= 0 || d > kMaxDims || ldim < n) return -1;
   const int m = rows ? nrows : n - lfil;
   if (m <= 0) return -1;
   // row pointers of the m rows alone, packed in list order (the KNN kernels read ia of their rows only)
   std::vector<int> hia(n + 1, 0);
   for (int r = 0; r < m; r++) {
      const int i = rows ? rows[r] : lfil + r;
      if (i < lfil || i >= n || (rows && r > 0 && i <= rows[r - 1])) return -1;
      hia[i] = r * lfil;
   }
   hipStream_t s = current_stream();
   double* dX = nullptr;
   int *dia = nullptr, *dja = nullptr, *drows = nullptr;
   int rc = -1;
   if (upload(&dX, X, (size_t)ldim * d) == 0 && upload(&dia, hia.data(), hia.size()) == 0 &&
       upload(&dja, (const int*)nullptr, (size_t)m * lfil) == 0 && (!rows || upload(&drows, rows, (size_t)m) == 0)) {
      const int nf = knn_pattern(dX, n, ldim, d, lfil, dia, dja, s, variant, drows, rows ? m : 0);
      if (nf >= 0 && hipMemcpyAsync(ja_out, dja, sizeof(int) * (size_t)m * lfil, hipMemcpyDeviceToHost, s) == hipSuccess &&
          hipStreamSynchronize(s) == hipSuccess) {
         if (nfail) *nfail = nf;
         rc = 0;
      }
   }
   (void)hipStreamSynchronize(s);
   (void)hipFree(dX);
   (void)hipFree(dia);
   (void)hipFree(dja);
   (void)hipFree(drows);
   return rc;
}

}  // extern "C"
