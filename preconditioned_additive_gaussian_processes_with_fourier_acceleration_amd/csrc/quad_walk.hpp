// quad_walk.hpp -- phi^T S phi for the 128 points of a workgroup on v_mfma_f64_16x16x4_f64, S symmetric R_p x R_p.
// The body of k_model_std (model_variance.hip), shared with k_fgp_loo (feature_gp.hip),
// which walks three matrices one after another and also dots the points' features with NLIN coefficient vectors.
// k_model_paths (model_paths.hip) takes the points, the feature generation and the buffers from here for
// Phi B.  The features themselves are window_points.hpp's mv_features.
//
// One workgroup owns 128 points and walks S in column tiles of 144 (4 windows); per tile the product
// Phi S[:, tile] (128 x 144) is accumulated over k steps of 36 (one window).  The Phi operand is generated into LDS
// per step: one sincospi per (point, window) and 16 rotations, four threads per point each storing a quarter of the
// window's features.  8 waves of 16 points x 144 columns (9 MFMA blocks, operands swapped as in k_gemm_f64: a lane
// holds the columns lane / 16 + 4 reg of 16 consecutive points).  LDS is double-buffered as in k_gemm_f64: step c's
// MFMAs read buffer c & 1 while step c + 1's rows of S (global loads issued before them) are in flight and its
// features are generated into the other buffer; one barrier per step.  The epilogue regenerates the tile's own 4
// windows of features and dots them with the accumulators: Phi and Phi S never reach memory.  S is symmetric, so a
// tile walks only the windows up to its own and doubles the earlier ones' sum: 144 of 256 k steps at 32 windows.
// A point's sum runs over (tile, window, block, register) in a fixed order, then over its 4 lanes in lane order
// (quad_fold): its bits depend on neither its place in the batch nor the batch size.
#pragma once
#include "window_points.hpp"

namespace nfft4gp_amd {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kMsPts = 128, kMsCols = 4 * kMvPad, kMsThreads = 512;
constexpr int kMsLdA = kMsPts + 1, kMsLdB = kMsCols + 1;
constexpr int kMsBuf = kMvPad * (kMsLdA + kMsLdB);          // doubles per buffer: features, then rows of S
constexpr size_t kMsLds = sizeof(double) * 2 * kMsBuf;      // 157.8 KB: one workgroup per CU
constexpr int kMsRowGroups = 6;                             // S fetch: 72 column pairs x 6 row groups of 6 rows

// the windows and points of a walk
struct QuadPoints {
   const double* centre;
   const double* scale;
   const int* feature;
   int nw;
   const double* X;
   long long ldim;
   long long ip;  // the thread's point (tid & 127 of the workgroup's 128); live: it exists
   bool live;
};

// rows 33..35 of both feature buffers are zero for the whole kernel (a window's 3 padded slots); once, before a walk
__device__ inline void quad_zero_pad(double* m_smem)
{
   for (int b = 0; b < 2; b++)
      for (int e = threadIdx.x; e < (kMvPad - kMvFeat) * kMsLdA; e += kMsThreads)
         m_smem[b * kMsBuf + kMvFeat * kMsLdA + e] = 0.0;
}

// window c's 33 features of the 128 points into As[feature][point]; part: 0 cos 0..8, 1 cos 9..16, 2 sin 1..8,
// 3 sin 9..16.  With NLIN > 0 the thread also adds its quarter of the window to lin[q] += coef[q ldc + slot] feature
// (the coefficient's address is uniform over the wave: a scalar load)
template <int NLIN>
__device__ inline void quad_gen(const QuadPoints& Q, int c, double x, int p, int part, double* As,
                                const double* __restrict__ coef, int ldc, double* lin)
{
   (void)mv_features(x, Q.centre[c], Q.scale[c], [&](int j, double v) {
      const int k = j <= 16 ? j : j - 16;
      if (part == (j <= 16 ? 0 : 2) + (k <= 8 ? 0 : 1)) {
         As[j * kMsLdA + p] = v;
#pragma unroll
         for (int q = 0; q < NLIN; q++) lin[q] = fma(coef[(size_t)q * ldc + c * kMvPad + j], v, lin[q]);
      }
   });
}

// The lane's share of phi^T S phi for the point wm + lr of the workgroup (quad_fold adds the 4 lanes' shares).
// m_smem: kMsLds bytes, quad_zero_pad done.  with_lin (uniform over the workgroup; NLIN > 0): the epilogue's
// feature generation also accumulates the NLIN linear forms of the thread's point p = tid & 127 into lin.
template <int NLIN>
__device__ inline double quad_walk(const double* __restrict__ S, int Rp, const QuadPoints& Q, double* m_smem,
                                   bool with_lin, const double* __restrict__ coef, int ldc, double* lin)
{
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
   const int wm = wave * 16, lr = lane & 15, lg = lane >> 4;
   const int p = tid & (kMsPts - 1), part = tid >> 7;
   const int fcol = 2 * (tid % (kMsCols / 2)), frow = tid / (kMsCols / 2);  // frow >= 6: no part in the S fetch
   const int nw = Q.nw;
   auto xload = [&](int c) { return Q.live ? Q.X[(size_t)Q.feature[c] * (size_t)Q.ldim + Q.ip] : Q.centre[c]; };
   auto gen = [&](int c, double x, double* As) { quad_gen<0>(Q, c, x, p, part, As, nullptr, 0, nullptr); };
   double2 bv[kMvPad / kMsRowGroups];
   double psum = 0.0;
   const int ntile = Rp / kMsCols;
   for (int t = 0; t < ntile; t++) {
      auto fetch = [&](int c) {  // rows 36 c .. 36 c + 35 of S, the tile's 144 columns (R_p is a whole number of tiles)
         const double* Sc = S + (size_t)(c * kMvPad + frow) * Rp + t * kMsCols + fcol;
         if (frow < kMsRowGroups) {
#pragma unroll
            for (int u = 0; u < kMvPad / kMsRowGroups; u++)
               bv[u] = *reinterpret_cast<const double2*>(Sc + (size_t)u * kMsRowGroups * Rp);
         }
      };
      auto store = [&](double* Bs) {
         if (frow < kMsRowGroups) {
#pragma unroll
            for (int u = 0; u < kMvPad / kMsRowGroups; u++) {
               Bs[(frow + u * kMsRowGroups) * kMsLdB + fcol] = bv[u].x;
               Bs[(frow + u * kMsRowGroups) * kMsLdB + fcol + 1] = bv[u].y;
            }
         }
      };
      d4 acc[9];
#pragma unroll
      for (int j = 0; j < 9; j++) acc[j] = d4{0.0, 0.0, 0.0, 0.0};
      __syncthreads();  // the previous tile's epilogue has left both buffers
      fetch(0);
      gen(0, xload(0), m_smem);
      store(m_smem + kMvPad * kMsLdA);
      __syncthreads();
      int cur = 0;
      const int cend = min(nw, 4 * t + 4);  // S is symmetric: the windows after the tile's own are not walked
      for (int c = 0; c < cend; c++) {
         const bool more = c + 1 < cend;
         if (c == 4 * t) {  // the windows before the tile's own count twice (exact), its own once
#pragma unroll
            for (int j = 0; j < 9; j++) acc[j] *= 2.0;
         }
         double xn = 0.0;
         if (more) {
            fetch(c + 1);  // in flight during this step's MFMAs
            xn = xload(c + 1);
         }
         const double* As = m_smem + cur * kMsBuf;
         const double* Bs = As + kMvPad * kMsLdA;
#pragma unroll 3
         for (int k4 = 0; k4 < kMvPad / 4; k4++) {
            const int kk = 4 * k4 + lg;
            const double a = As[kk * kMsLdA + wm + lr];
            double b[9];
#pragma unroll
            for (int j = 0; j < 9; j++) b[j] = Bs[kk * kMsLdB + 16 * j + lr];
#pragma unroll
            for (int j = 0; j < 9; j++) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(b[j], a, acc[j], 0, 0, 0);
         }
         if (more) {  // the other buffer: nobody reads it during this step
            gen(c + 1, xn, m_smem + (cur ^ 1) * kMsBuf);
            store(m_smem + (cur ^ 1) * kMsBuf + kMvPad * kMsLdA);
         }
         __syncthreads();
         cur ^= 1;
      }
      // acc[j][rg] = (Phi S)[point wm + lr][column 144 t + 16 j + lg + 4 rg]; window wl of the tile holds the
      // columns [36 wl, 36 wl + 36): blocks j = 36 wl / 16 .. (36 wl + 35) / 16
#pragma unroll
      for (int wl = 0; wl < 4; wl++) {
         const int c = 4 * t + wl;
         if (c < nw) {  // uniform over the workgroup
            double* As = m_smem + (wl & 1) * kMsBuf;  // its readers of two windows ago are behind the last barrier
            if (NLIN > 0 && with_lin)
               quad_gen<NLIN>(Q, c, xload(c), p, part, As, coef, ldc, lin);
            else
               gen(c, xload(c), As);
            __syncthreads();
#pragma unroll
            for (int j = (kMvPad * wl) / 16; j <= (kMvPad * wl + kMvPad - 1) / 16; j++)
#pragma unroll
               for (int rg = 0; rg < 4; rg++) {
                  const int fj = 16 * j + lg + 4 * rg - kMvPad * wl;
                  const double phi = (fj >= 0 && fj < kMvPad) ? As[fj * kMsLdA + wm + lr] : 0.0;
                  psum = fma(acc[j][rg], phi, psum);
               }
         }
      }
   }
   return psum;
}

// s_q[point] = the sum of the point's 4 lanes' shares, in lane order (the caller's barrier follows)
__device__ inline void quad_fold(double psum, double* s_q)
{
   const int lane = threadIdx.x & 63, wm = (threadIdx.x >> 6) * 16, lr = lane & 15, lg = lane >> 4;
   const double v0 = __shfl(psum, lr), v1 = __shfl(psum, lr + 16), v2 = __shfl(psum, lr + 32),
                v3 = __shfl(psum, lr + 48);
   if (lg == 0) s_q[wm + lr] = ((v0 + v1) + v2) + v3;
}

}  // namespace nfft4gp_amd
