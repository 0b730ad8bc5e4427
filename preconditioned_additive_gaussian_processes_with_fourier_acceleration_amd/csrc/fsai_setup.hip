// fsai_setup.hip -- the FSAI preconditioner built on the GPU, with gradients, behind the reference's
// interface (SRC/preconds/fsai.h:46-207):
//
//   Nfft4GPAmdPrecondFsaiCreate / SetLfil / Reset / Free          fsai.c:3-104
//   Nfft4GPAmdPrecondFsaiSetupWithKernel (precond_kernel_setup)   fsai.c:302-312 -> :314-673
//       pattern  Nfft4GPDistanceEuclidKnn (kernels.c:121-278): row i < lfil is dense (0..i); row i >= lfil
//                holds the lfil-1 nearest points among 0..i-1, then i: knn_pattern() (knn_pattern.hip).
//       values   per row, the kernel submatrix K_a of its points, L_a = chol(K_a), A_ai = K_a^{-1} e_k /
//                sqrt(e_k' K_a^{-1} e_k); with gradients dA_g = K_a^{-1}(-dK_g A_ai) - 1/2 (.)_k dd A_ai
//                (fsai.c:530-563).  k_fsai_rows: one wave per row, K_a in LDS.
//   Nfft4GPAmdPrecondFsaiSolve  (func_solve)   x = L^T (L rhs)                 fsai.c:106-123
//   Nfft4GPAmdPrecondFsaiInvL / InvLT          L^{-1} rhs, L^{-T} rhs          fsai.c:675-728
//   Nfft4GPAmdPrecondFsaiDvp    (func_dvp)                                     fsai.c:125-216
//   Nfft4GPAmdPrecondFsaiTrace  (func_trace)   2 sum_i dL_g(i,i) / L(i,i)      fsai.c:218-276
//   Nfft4GPAmdPrecondFsaiLogdet (func_logdet)  2 sum_i log(1 / L(i,i))         fsai.c:278-301
//
// The triangular solves are CSR SpTRSVs over level sets computed once at setup (a row's level is one
// more than its dependencies'; ~250 levels for 2e4 KNN rows): ONE workgroup walks the levels with a
// barrier between them, so there is no grid-wide synchronisation and no spinning.  Each row sums in the
// reference's order with unfused multiply-add, so given the same factors the solves, products and Dvp
// are bitwise the reference's.
//
// Kernel: the plain (non-additive) Gaussian or Matern-1/2 kernel of all d columns of `data` with the
// parameters of `fkernel_params` (_params[0] = f, _params[1] = l, _noise_level = mu; kernels.c:680-1289,
// :2390-3033), as the reference's FSAI runs on Nfft4GPKernelGaussianKernel.  The reference's FSAI on its
// additive kernel would evaluate buffer rows instead of the pattern's points (kernels.c:3160 ignores
// the data argument); this library does not reproduce that.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "callbacks.hpp"
#include "csr.hpp"
#include "internal.h"
#include "kernel_eval.hpp"

using namespace nfft4gp_amd;

namespace {

constexpr int kTrsvThreads = 1024;

// In place on the wave's LDS vector b: b = L^{-1} b (trans = 0) or L^{-T} b (trans = 1), L lower in A.
template <int LD>
__device__ void wave_trsv(double (*A)[LD], int k, double* b, int trans)
{
   const int lane = threadIdx.x;
   if (!trans) {
      for (int m = 0; m < k; m++) {
         if (lane == 0) b[m] /= A[m][m];
         __syncthreads();
         if (lane > m && lane < k) b[lane] -= A[lane][m] * b[m];
         __syncthreads();
      }
   } else {
      for (int m = k - 1; m >= 0; m--) {
         if (lane == 0) b[m] /= A[m][m];
         __syncthreads();
         if (lane < m) b[lane] -= A[m][lane] * b[m];
         __syncthreads();
      }
   }
}

// one wave per row i: A_ai (and dA_ai for the three gradients) into aa / da (fsai.c:353-398, :493-563)
//
// W (kw x n column-major, optional): the Schur-complement kernel K(x_r, x_c) - W(:, r)' W(:, c) of the AFN
// setup (Nfft4GPKernelSchurCombineKernel, kernels.c:3599-3760, with W = L11^{-1} K12), staged through LDS
// kSchurChunk rows of W at a time so each row reads its lfil columns of W once.
// Gradients of the Schur kernel (MATLAB schurCombinedKernelMat.m): with B_g = L11^{-1} dK12_g (GB, g = f, l;
// zero for mu) and C_g = (L11^{-1} dK11_g L11^{-T}) W (GC, g = f, l, mu), both kw x n per g,
//   dS_g(r, c) = dK_g(r, c) - W_r' B_g,c - B_g,r' W_c + W_r' C_g,c,
// so (dS_g a)_r = (dK_g a)_r - W_r' (B_g a - C_g a) - B_g,r' (W a) with the kw-vectors W a = sum_c W_c a_c etc.
// KM: the LDS arrays' row capacity (>= lfil); KM = 32 takes 17 KB per workgroup (9 per CU) where 64
// takes 51 KB (3 per CU).
constexpr int kSchurChunk = 32;
// KM = 20 (the reference's default lfil) takes 8.8 KB, so 18 row-waves share a CU instead of 9 at KM = 32: the
// Schur rows are bound by the latency of their W-chunk loads, and twice the rows in flight hide twice as much
template <int KM>
__global__ __launch_bounds__(64) void k_fsai_rows(const double* __restrict__ X, long long ldim,
                                                  const int* __restrict__ ia, const int* __restrict__ ja,
                                                  KernelParams P, const double* __restrict__ W, int kw, int grad,
                                                  int nnz, double* __restrict__ aa, double* __restrict__ da,
                                                  const double* __restrict__ GB, const double* __restrict__ GC,
                                                  const int* __restrict__ wcol)
{
   __shared__ double A[KM][KM + 1];
   __shared__ double Ws[KM][kSchurChunk + 1];
   __shared__ double a[KM], u[KM];
   __shared__ int idx[KM], widx[KM];
   const int i = blockIdx.x;
   const int lane = threadIdx.x;
   const int j1 = ia[i];
   const int k = ia[i + 1] - j1;
   if (lane < k) {
      idx[lane] = ja[j1 + lane];
      // W's column of the entry: the point itself, or (a row shard's chunk of W) its position in the chunk
      widx[lane] = wcol ? wcol[j1 + lane] : idx[lane];
   }
   __syncthreads();
   // K_a (lower triangle is all the factorisation reads)
   for (int e = lane; e < k * k; e += 64) {
      const int r = e % k, c = e / k;
      if (c > r) continue;
      double K, dK[3];
      kern_pair(P, X, ldim, idx[r], idx[c], r == c, K, dK);
      A[r][c] = K;
   }
   __syncthreads();
   if (W) {
      // the next chunk's W entries are loaded into registers while this chunk's products run
      constexpr int kPerLane = (KM * kSchurChunk + 63) / 64;
      double wr[kPerLane];
      auto fetch_chunk = [&](int t0) {
         const int tc = min(kSchurChunk, kw - t0);
#pragma unroll
         for (int q = 0; q < kPerLane; q++) {
            const int e = lane + 64 * q;
            wr[q] = e < k * tc ? W[(size_t)widx[e / tc] * kw + t0 + e % tc] : 0.0;
         }
      };
      fetch_chunk(0);
      for (int t0 = 0; t0 < kw; t0 += kSchurChunk) {
         const int tc = min(kSchurChunk, kw - t0);
#pragma unroll
         for (int q = 0; q < kPerLane; q++) {
            const int e = lane + 64 * q;
            if (e < k * tc) Ws[e / tc][e % tc] = wr[q];
         }
         __syncthreads();
         if (t0 + kSchurChunk < kw) fetch_chunk(t0 + kSchurChunk);
         for (int e = lane; e < k * k; e += 64) {
            const int r = e % k, c = e / k;
            if (c > r) continue;
            double acc = 0.0;
            for (int tt = 0; tt < tc; tt++) acc = fma(Ws[r][tt], Ws[c][tt], acc);
            A[r][c] -= acc;
         }
         __syncthreads();
      }
   }
   // Cholesky, lower (dpotrf 'L')
   for (int j = 0; j < k; j++) {
      if (lane == 0) A[j][j] = sqrt(A[j][j]);
      __syncthreads();
      if (lane > j && lane < k) A[lane][j] /= A[j][j];
      __syncthreads();
      if (lane > j && lane < k) {
         const double arj = A[lane][j];
         for (int c = j + 1; c <= lane; c++) A[lane][c] -= arj * A[c][j];
      }
      __syncthreads();
   }
   // A_ai = K_a^{-1} e_k, scaled by 1/sqrt(its last entry)
   if (lane < k) a[lane] = (lane == k - 1) ? 1.0 : 0.0;
   __syncthreads();
   wave_trsv(A, k, a, 0);
   wave_trsv(A, k, a, 1);
   const double dd_scale = 1.0 / sqrt(a[k - 1]);
   __syncthreads();
   if (lane < k) {
      a[lane] *= dd_scale;
      aa[j1 + lane] = a[lane];
   }
   __syncthreads();
   if (!grad) return;
   for (int g = 0; g < 3; g++) {
      // u = -dK_g A_ai (dK_g recomputed from the coordinates: K_a's storage now holds its factor)
      if (lane < k) {
         double acc = 0.0;
         for (int c = 0; c < k; c++) {
            double K, dK[3];
            kern_pair(P, X, ldim, idx[lane], idx[c], lane == c, K, dK);
            acc = fma(dK[g], a[c], acc);
         }
         u[lane] = -acc;
      }
      __syncthreads();
      if (W && GC) {
         // the Schur terms, kSchurChunk entries of the kw-vectors at a time: Ws holds (W a, B_g a - C_g a)
         const double* Bg = g < 2 ? GB + (size_t)g * kw * ((size_t)gridDim.x) : nullptr;
         const double* Cg = GC + (size_t)g * kw * ((size_t)gridDim.x);
         double acc = 0.0;
         for (int t0 = 0; t0 < kw; t0 += kSchurChunk) {
            const int tc = min(kSchurChunk, kw - t0);
            if (lane < tc) {
               double wa = 0.0, ba = 0.0, ca = 0.0;
               for (int c = 0; c < k; c++) {
                  const size_t o = (size_t)widx[c] * kw + t0 + lane;
                  wa = fma(W[o], a[c], wa);
                  if (Bg) ba = fma(Bg[o], a[c], ba);
                  ca = fma(Cg[o], a[c], ca);
               }
               Ws[0][lane] = wa;
               Ws[1][lane] = ba - ca;
            }
            __syncthreads();
            if (lane < k) {
               const size_t o = (size_t)widx[lane] * kw + t0;
               for (int tt = 0; tt < tc; tt++) {
                  acc = fma(W[o + tt], Ws[1][tt], acc);
                  if (Bg) acc = fma(Bg[o + tt], Ws[0][tt], acc);
               }
            }
            __syncthreads();
         }
         if (lane < k) u[lane] += acc;  // u = -(dS_g a)
         __syncthreads();
      }
      wave_trsv(A, k, u, 0);
      wave_trsv(A, k, u, 1);
      const double t = -0.5 * u[k - 1] * dd_scale;
      __syncthreads();
      if (lane < k) da[(size_t)g * nnz + j1 + lane] = fma(t, a[lane], u[lane]);
      __syncthreads();
   }
}

// the row kernel with the smallest LDS rows for the pattern (NFFT4GP_AMD_FSAI_KM=32 forces the 32-row one, A/B)
typedef void (*FsaiRowsFn)(const double*, long long, const int*, const int*, KernelParams, const double*, int, int,
                           int, double*, double*, const double*, const double*, const int*);
static FsaiRowsFn fsai_rows_kernel(int lfil)
{
   static const int force = getenv("NFFT4GP_AMD_FSAI_KM") ? atoi(getenv("NFFT4GP_AMD_FSAI_KM")) : 0;
   if (lfil <= 20 && force != 32) return k_fsai_rows<20>;
   if (lfil <= 32) return k_fsai_rows<32>;
   return k_fsai_rows<kFsaiMaxK>;
}

// ---- level-scheduled CSR triangular solves: one workgroup, a barrier between levels ----------------
// x = L^{-1} rhs (fsai.c:675-699): x[i] = (rhs[i] - sum_{j < diag} L_ij x_j) / L_ii in the row's order
__global__ __launch_bounds__(kTrsvThreads) void k_trsv_lower(const int* __restrict__ lev_ptr, int nlev,
                                                             const int* __restrict__ lev_rows,
                                                             const int* __restrict__ ia, const int* __restrict__ ja,
                                                             const double* __restrict__ aa,
                                                             const double* __restrict__ rhs, double* x)
{
#pragma clang fp contract(off)  // the reference's host build: separate multiply and subtract
   for (int lv = 0; lv < nlev; lv++) {
      for (int e = lev_ptr[lv] + threadIdx.x; e < lev_ptr[lv + 1]; e += kTrsvThreads) {
         const int i = lev_rows[e];
         const int j2 = ia[i + 1] - 1;
         double s = rhs[i];
         for (int j = ia[i]; j < j2; j++) s -= aa[j] * x[ja[j]];
         x[i] = s / aa[j2];
      }
      __syncthreads();
   }
}

// x = L^{-T} rhs (fsai.c:701-728) through L^T stored as CSR (tia/tja/taa: column c of L, rows ascending,
// diagonal first): the reference subtracts L_ic x_i from x[c] for i descending, then divides by L_cc
__global__ __launch_bounds__(kTrsvThreads) void k_trsv_upper(const int* __restrict__ lev_ptr, int nlev,
                                                             const int* __restrict__ lev_rows,
                                                             const int* __restrict__ tia,
                                                             const int* __restrict__ tja,
                                                             const double* __restrict__ taa,
                                                             const double* __restrict__ rhs, double* x)
{
#pragma clang fp contract(off)
   for (int lv = 0; lv < nlev; lv++) {
      for (int e = lev_ptr[lv] + threadIdx.x; e < lev_ptr[lv + 1]; e += kTrsvThreads) {
         const int c = lev_rows[e];
         const int p0 = tia[c];
         double s = rhs[c];
         for (int p = tia[c + 1] - 1; p > p0; p--) s -= taa[p] * x[tja[p]];
         x[c] = s / taa[p0];
      }
      __syncthreads();
   }
}

// y = beta y + A x for a CSR A (matops.c:139-272 with alpha = 1, beta in {0, 1}): the row accumulates
// into y[i] itself (matops.c:247), in row order, unfused
__global__ __launch_bounds__(256) void k_csr_mv(const int* __restrict__ ia, const int* __restrict__ ja,
                                                const double* __restrict__ a, const double* __restrict__ x,
                                                double* __restrict__ y, int n, int beta_one)
{
   const int r0 = blockIdx.x * 256;
   csr_rows_staged<256, 2048>(ia, ja, a, x, y, r0, min(r0 + 256, n), beta_one != 0);  // csr.hpp: entries via LDS
}

// out[blk] = sum over the block's rows of num[diag_i] / den[diag_i] (or log(1 / den[diag_i]) when num is
// NULL), diag_i = ia[i+1] - 1; the host sums the blocks in order
__global__ __launch_bounds__(256) void k_diag_sum(const int* __restrict__ ia, int n, const double* __restrict__ num,
                                                  const double* __restrict__ den, double* __restrict__ out)
{
   __shared__ double s[4];
   const int i = blockIdx.x * 256 + threadIdx.x;
   double v = 0.0;
   if (i < n) {
      const int p = ia[i + 1] - 1;
      v = num ? num[p] / den[p] : log(1.0 / den[p]);
   }
   for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
   if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
   __syncthreads();
   if (threadIdx.x == 0) out[blockIdx.x] = (s[0] + s[1]) + (s[2] + s[3]);
}

__global__ void k_gather_vals(const double* __restrict__ src, const int* __restrict__ map, int count,
                              double* __restrict__ dst)
{
   const int p = blockIdx.x * blockDim.x + threadIdx.x;
   if (p < count) dst[p] = src[map[p]];
}

// the reference's precond_fsai, restated, with the device factors
struct PrecondFsaiAmd {
   int lfil = 50;  // fsai.c:12
   int kernel = 0;
   int n = 0, nnz = 0;
   bool grad = false;
   int *ia = nullptr, *ja = nullptr, *tia = nullptr, *tja = nullptr, *tmap = nullptr;
   double *aa = nullptr, *taa = nullptr, *da = nullptr, *tda = nullptr;  // da, tda: 3 nnz
   int *lev_ptr = nullptr, *lev_rows = nullptr, *rlev_ptr = nullptr, *rlev_rows = nullptr;
   int nlev = 0, nrlev = 0;
   double *work = nullptr, *part = nullptr;
   void release()
   {
      (void)hipStreamSynchronize(current_stream());
      for (int* p : {ia, ja, tia, tja, tmap, lev_ptr, lev_rows, rlev_ptr, rlev_rows}) (void)hipFree(p);
      for (double* p : {aa, taa, da, tda, work, part}) (void)hipFree(p);
      ia = ja = tia = tja = tmap = lev_ptr = lev_rows = rlev_ptr = rlev_rows = nullptr;
      aa = taa = da = tda = work = part = nullptr;
      n = nnz = nlev = nrlev = 0;
      grad = false;
   }
};

// level sets of the lower solve (a row after all its dependencies) and of the transposed solve
void level_sets(int n, const std::vector<int>& ia, const std::vector<int>& ja, std::vector<int>& ptr,
                std::vector<int>& rows, bool transposed)
{
   std::vector<int> lev(n, 0);
   int maxlev = 0;
   if (!transposed) {
      for (int i = 0; i < n; i++) {
         int l = 0;
         for (int p = ia[i]; p < ia[i + 1] - 1; p++) l = std::max(l, lev[ja[p]] + 1);
         lev[i] = l;
         maxlev = std::max(maxlev, l);
      }
   } else {
      for (int j = n - 1; j >= 0; j--)
         for (int p = ia[j]; p < ia[j + 1] - 1; p++) lev[ja[p]] = std::max(lev[ja[p]], lev[j] + 1);
      for (int i = 0; i < n; i++) maxlev = std::max(maxlev, lev[i]);
   }
   ptr.assign(maxlev + 2, 0);
   for (int i = 0; i < n; i++) ptr[lev[i] + 1]++;
   for (int l = 0; l <= maxlev; l++) ptr[l + 1] += ptr[l];
   rows.assign(n, 0);
   std::vector<int> pos(ptr.begin(), ptr.end() - 1);
   for (int i = 0; i < n; i++) rows[pos[lev[i]]++] = i;
}

// device factors from host CSR (ia, ja, aa [, da 3 nnz]): L, L^T (column entries in ascending row order,
// the order Nfft4GPCsrMv('T') accumulates in), the map between them, the level sets
int fsai_load(PrecondFsaiAmd* F, int n, const int* ia, const int* ja, const double* aa, const double* da)
{
   F->release();
   const int nnz = ia[n];
   std::vector<int> hia(ia, ia + n + 1), hja(ja, ja + nnz);
   std::vector<int> tcnt(n + 1, 0), tia(n + 1, 0), tja(nnz), tmap(nnz);
   for (int p = 0; p < nnz; p++) tcnt[ja[p] + 1]++;
   for (int c = 0; c < n; c++) tia[c + 1] = tia[c] + tcnt[c + 1];
   std::vector<int> pos(tia.begin(), tia.end() - 1);
   for (int i = 0; i < n; i++)
      for (int p = ia[i]; p < ia[i + 1]; p++) {
         const int q = pos[ja[p]]++;
         tja[q] = i;
         tmap[q] = p;
      }
   std::vector<int> lp, lr, rp, rr;
   level_sets(n, hia, hja, lp, lr, false);
   level_sets(n, hia, hja, rp, rr, true);
   F->n = n;
   F->nnz = nnz;
   F->nlev = (int)lp.size() - 1;
   F->nrlev = (int)rp.size() - 1;
   // reverse the transposed levels: the first processed holds the rows with no later dependents
   if (upload(&F->ia, hia.data(), hia.size()) || upload(&F->ja, hja.data(), hja.size()) ||
       upload(&F->tia, tia.data(), tia.size()) || upload(&F->tja, tja.data(), tja.size()) ||
       upload(&F->tmap, tmap.data(), tmap.size()) || upload(&F->lev_ptr, lp.data(), lp.size()) ||
       upload(&F->lev_rows, lr.data(), lr.size()) || upload(&F->rlev_ptr, rp.data(), rp.size()) ||
       upload(&F->rlev_rows, rr.data(), rr.size()) || upload(&F->aa, aa, (size_t)nnz) ||
       upload(&F->taa, (const double*)nullptr, (size_t)nnz) || upload(&F->work, (const double*)nullptr, 3 * (size_t)n) ||
       upload(&F->part, (const double*)nullptr, (size_t)(n + 255) / 256 + 1))
      return -1;
   hipStream_t s = current_stream();
   hipLaunchKernelGGL(k_gather_vals, dim3((nnz + 255) / 256), dim3(256), 0, s, F->aa, F->tmap, nnz, F->taa);
   if (da) {
      if (upload(&F->da, da, 3 * (size_t)nnz) || upload(&F->tda, (const double*)nullptr, 3 * (size_t)nnz)) return -1;
      for (int g = 0; g < 3; g++)
         hipLaunchKernelGGL(k_gather_vals, dim3((nnz + 255) / 256), dim3(256), 0, s, F->da + (size_t)g * nnz, F->tmap,
                            nnz, F->tda + (size_t)g * nnz);
      F->grad = true;
   }
   NFFT4GP_HIP_CHECK(hipGetLastError());
   return 0;
}

int inv_l(PrecondFsaiAmd* F, double* x, const double* rhs, hipStream_t s)
{
   hipLaunchKernelGGL(k_trsv_lower, dim3(1), dim3(kTrsvThreads), 0, s, F->lev_ptr, F->nlev, F->lev_rows, F->ia, F->ja,
                      F->aa, rhs, x);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   return 0;
}

int inv_lt(PrecondFsaiAmd* F, double* x, const double* rhs, hipStream_t s)
{
   hipLaunchKernelGGL(k_trsv_upper, dim3(1), dim3(kTrsvThreads), 0, s, F->rlev_ptr, F->nrlev, F->rlev_rows, F->tia,
                      F->tja, F->taa, rhs, x);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   return 0;
}

void csr_mv(const int* ia, const int* ja, const double* a, const double* x, double* y, int n, int beta_one,
            hipStream_t s)
{
   hipLaunchKernelGGL(k_csr_mv, dim3((n + 255) / 256), dim3(256), 0, s, ia, ja, a, x, y, n, beta_one);
}

// fsai.c:163-200 for gradient g on device vectors; y: n entries
int dvp_one(PrecondFsaiAmd* F, int g, const double* x, double* y, hipStream_t s)
{
   const int n = F->n;
   double* w1 = F->work;
   double* w2 = F->work + n;
   const double* dl = F->da + (size_t)g * F->nnz;
   const double* tdl = F->tda + (size_t)g * F->nnz;
   if (inv_lt(F, w1, x, s)) return -1;            // work = L^{-T} x
   csr_mv(F->tia, F->tja, tdl, w1, y, n, 0, s);   // y = dL^T work
   if (inv_lt(F, w2, y, s)) return -1;            // work2 = L^{-T} y
   if (inv_l(F, y, w1, s)) return -1;             // y = L^{-1} work
   csr_mv(F->ia, F->ja, dl, y, w2, n, 1, s);      // work2 += dL y
   csr_mv(F->tia, F->tja, F->taa, w2, y, n, 0, s);  // y = L^T work2
   NFFT4GP_HIP_CHECK(hipGetLastError());
   return 0;
}

double diag_sum(PrecondFsaiAmd* F, const double* num, hipStream_t s)
{
   const int nb = (F->n + 255) / 256;
   hipLaunchKernelGGL(k_diag_sum, dim3(nb), dim3(256), 0, s, F->ia, F->n, num, F->aa, F->part);
   std::vector<double> h(nb);
   if (hipMemcpyAsync(h.data(), F->part, sizeof(double) * nb, hipMemcpyDeviceToHost, s) != hipSuccess ||
       hipStreamSynchronize(s) != hipSuccess)
      return NAN;
   double v = 0.0;
   for (double t : h) v += t;
   return v;
}

}  // namespace

namespace nfft4gp_amd {

int additive_buffer_info(void* str, const double** xw, int* n, int* nw, int* dw, int* skip_last, int* kernel);

// The kernel a setup evaluates: this library's additive NFFT handle as fkernel_params gives the dense
// additive kernel of its gathered window buffer (uploaded to *owned), anything else the plain kernel of
// the points with _params / _noise_level of the nfft4gp_kernel.  The kernel type comes from fkernel
// when it is one of this library's setup functions, else from `kernel`.  Returns 1 (additive), 0
// (plain) or -1.
int kernel_spec_of(void* fkernel_params, func_kernel fkernel, int kernel, int n, KernelSpec& K, double** owned)
{
   *owned = nullptr;
   const nfft4gp_kernel* kp = (const nfft4gp_kernel*)fkernel_params;
   if (!kp) return -1;
   K.kernel = kernel ? 1 : 0;
   if (fkernel == &Nfft4GPNFFTAdditiveKernelGaussianKernel) K.kernel = 0;
   else if (fkernel == &Nfft4GPNFFTAdditiveKernelMatern12Kernel) K.kernel = 1;
   K.f = kp->_params[0];
   K.l = kp->_params[1];
   K.mu = kp->_noise_level;
   K.Xk = nullptr;
   const double* xw = nullptr;
   int nn = 0, nw = 0, dw = 0, skip = 0, pk = -1;
   if (additive_buffer_info(fkernel_params, &xw, &nn, &nw, &dw, &skip, &pk)) return 0;
   if (nn != n || nw <= 0 || dw <= 0 || skip >= dw) {
      fprintf(stderr, "nfft4gp_amd: the additive handle holds %d points, the setup got %d\n", nn, n);
      return -1;
   }
   if (fkernel != &Nfft4GPNFFTAdditiveKernelGaussianKernel && fkernel != &Nfft4GPNFFTAdditiveKernelMatern12Kernel &&
       pk >= 0)
      K.kernel = pk;
   const size_t D = (size_t)(nw - 1) * dw + (dw - skip);
   if (upload(owned, xw, D * (size_t)n)) return -1;
   K.Xk = *owned;
   K.ldk = n;
   K.nw = nw;
   K.dw = dw;
   K.last_dw = dw - skip;
   return 1;
}

// The FSAI of a kernel matrix (fsai.c:314-673) from device coordinates: KNN pattern, per-row values (and
// gradients), copied to host CSR.  dW (kw x n, optional): the Schur-complement kernel of the AFN setup.
int fsai_kernel_csr(const double* dX, int n, int ldim, int d, int lfil, const KernelSpec& Ks, const double* dW, int kw,
                    int require_grad, std::vector<int>& hia, std::vector<int>& hja, std::vector<double>& haa,
                    std::vector<double>& hda, hipStream_t s, const double* dGB, const double* dGC, void** keep)
{
   if (n <= 0 || ldim < n || d <= 0 || d > kMaxDims || lfil < 1 || lfil > kFsaiMaxK || (dW && kw <= 0)) {
      fprintf(stderr, "nfft4gp_amd: FSAI setup needs 1 <= lfil <= %d and at most %d features\n", kFsaiMaxK,
              kMaxDims);
      return -1;
   }
   if (require_grad && dW && !dGC) {
      fprintf(stderr, "nfft4gp_amd: FSAI setup: gradients of the Schur-complement kernel need its B / C panels\n");
      return -1;
   }
   // pattern row pointers (kernels.c:133-168): dense rows below lfil, lfil entries after
   hia.assign(n + 1, 0);
   for (int i = 0; i < n; i++) hia[i + 1] = hia[i] + ((n <= lfil || i < lfil) ? i + 1 : lfil);
   const int nnz = hia[n];
   hja.assign((size_t)nnz, 0);
   for (int i = 0; i < std::min(n, n <= lfil ? n : lfil); i++)
      for (int j = 0; j <= i; j++) hja[hia[i] + j] = j;
   double *daa = nullptr, *dda = nullptr;
   int *dia = nullptr, *dja = nullptr;
   auto cleanup = [&](int rc) {
      (void)hipStreamSynchronize(s);
      for (double* p : {daa, dda}) (void)hipFree(p);
      for (int* p : {dia, dja}) (void)hipFree(p);
      return rc;
   };
   if (upload(&dia, hia.data(), hia.size()) || upload(&dja, hja.data(), hja.size()) ||
       upload(&daa, (const double*)nullptr, (size_t)nnz) ||
       (require_grad && upload(&dda, (const double*)nullptr, 3 * (size_t)nnz)))
      return cleanup(-1);
   if (n > lfil) {
      if (knn_pattern(dX, n, ldim, d, lfil, dia, dja, s, -1) < 0) return cleanup(-1);
   }
   const KernelParams P = kernel_params_of(Ks, d);
   const double* Xk = Ks.Xk ? Ks.Xk : dX;
   const long long ldk = Ks.Xk ? Ks.ldk : ldim;
   auto rows_kernel = fsai_rows_kernel(lfil);
   hipLaunchKernelGGL(rows_kernel, dim3(n), dim3(64), 0, s, Xk, ldk, dia, dja, P, dW, kw, require_grad ? 1 : 0, nnz,
                      daa, dda, dGB, dGC, (const int*)nullptr);
   if (keep && !require_grad) {  // the caller builds the handle on the device
      if (hipGetLastError() != hipSuccess) return cleanup(-1);
      keep[0] = dia;
      keep[1] = dja;
      keep[2] = daa;
      dia = nullptr;
      dja = nullptr;
      daa = nullptr;
      hja.clear();
      haa.clear();
      hda.clear();
      return cleanup(0);
   }
   haa.assign((size_t)nnz, 0.0);
   hda.assign(require_grad ? 3 * (size_t)nnz : 0, 0.0);
   if (hipGetLastError() != hipSuccess ||
       hipMemcpyAsync(hja.data(), dja, sizeof(int) * nnz, hipMemcpyDeviceToHost, s) != hipSuccess ||
       hipMemcpyAsync(haa.data(), daa, sizeof(double) * nnz, hipMemcpyDeviceToHost, s) != hipSuccess ||
       (require_grad &&
        hipMemcpyAsync(hda.data(), dda, sizeof(double) * hda.size(), hipMemcpyDeviceToHost, s) != hipSuccess) ||
       hipStreamSynchronize(s) != hipSuccess)
      return cleanup(-1);
   return cleanup(0);
}

// A row shard's rows of the FSAI pattern (kernels.c:121-278): `rows` (ascending) of the n points; rows below
// lfil hold every earlier point, the others the lfil - 1 nearest earlier points and themselves (the
// screened scans over this rank's rows only).  hia: m + 1 pointers over the listed rows, hja: point indices.
int fsai_pattern_rows(const double* dX, int n, int ldim, int d, int lfil, const std::vector<int>& rows,
                      std::vector<int>& hia, std::vector<int>& hja, hipStream_t s)
{
   if (n <= 0 || ldim < n || d <= 0 || d > kMaxDims || lfil < 1 || lfil > kFsaiMaxK) return -1;
   const int m = (int)rows.size();
   hia.assign(m + 1, 0);
   std::vector<int> iav((size_t)n + 1, 0), knn_rows;
   for (int r = 0; r < m; r++) {
      const int i = rows[r];
      const int len = (n <= lfil || i < lfil) ? i + 1 : lfil;
      iav[i] = hia[r];
      hia[r + 1] = hia[r] + len;
      if (!(n <= lfil || i < lfil)) knn_rows.push_back(i);
   }
   hja.assign((size_t)hia[m], 0);
   for (int r = 0; r < m; r++)
      if (n <= lfil || rows[r] < lfil)
         for (int j = 0; j <= rows[r]; j++) hja[hia[r] + j] = j;
   if (knn_rows.empty()) return 0;
   int *dia = nullptr, *dja = nullptr, *drows = nullptr;
   auto cleanup = [&](int rc) {
      (void)hipStreamSynchronize(s);
      for (int* p : {dia, dja, drows}) (void)hipFree(p);
      return rc;
   };
   if (upload(&dia, iav.data(), iav.size()) || upload(&dja, hja.data(), hja.size()) ||
       upload(&drows, knn_rows.data(), knn_rows.size()))
      return cleanup(-1);
   const int nf = knn_pattern(dX, n, ldim, d, lfil, dia, dja, s, -1, drows, (int)knn_rows.size());
   if (nf < 0 || hipMemcpyAsync(hja.data(), dja, sizeof(int) * hja.size(), hipMemcpyDeviceToHost, s) != hipSuccess ||
       hipStreamSynchronize(s) != hipSuccess)
      return cleanup(-1);
   return cleanup(0);
}

// Values of `nrows` pattern rows (device ia over those rows, absolute offsets into ja / aa) of the kernel (or,
// with W, the Schur-complement kernel): k_fsai_rows, W's column of each entry from wcol (nullptr: the point).
int fsai_values_rows(const KernelSpec& Ks, const double* dX, long long ldim, int d, int lfil, const int* dia,
                     const int* dja, int nrows, const double* dW, int kw, const int* dwcol, double* daa, hipStream_t s)
{
   if (nrows <= 0) return 0;
   const KernelParams P = kernel_params_of(Ks, d);
   const double* Xk = Ks.Xk ? Ks.Xk : dX;
   const long long ldk = Ks.Xk ? Ks.ldk : ldim;
   auto rows_kernel = fsai_rows_kernel(lfil);
   hipLaunchKernelGGL(rows_kernel, dim3(nrows), dim3(64), 0, s, Xk, ldk, dia, dja, P, dW, kw, 0, 0, daa,
                      (double*)nullptr, (const double*)nullptr, (const double*)nullptr, dwcol);
   return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- the Schur FSAI's operators for the AFN gradients (afn_grad.hip) ----------------------------------
void* fsai_grad_create(int n, const int* ia, const int* ja, const double* aa, const double* da)
{
   PrecondFsaiAmd* F = new PrecondFsaiAmd();
   if (fsai_load(F, n, ia, ja, aa, da)) {
      F->release();
      delete F;
      return nullptr;
   }
   return F;
}

void fsai_grad_free(void* F)
{
   if (!F) return;
   ((PrecondFsaiAmd*)F)->release();
   delete (PrecondFsaiAmd*)F;
}

// y = G x (op 0), G^T x (1), G^{-1} x (2), G^{-T} x (3), dG_g x (4), dG_g^T x (5); x != y
int fsai_grad_op(void* vF, int op, int g, const double* x, double* y, hipStream_t s)
{
   PrecondFsaiAmd* F = (PrecondFsaiAmd*)vF;
   const int n = F->n;
   switch (op) {
      case 0: csr_mv(F->ia, F->ja, F->aa, x, y, n, 0, s); break;
      case 1: csr_mv(F->tia, F->tja, F->taa, x, y, n, 0, s); break;
      case 2: return inv_l(F, y, x, s);
      case 3: return inv_lt(F, y, x, s);
      case 4: csr_mv(F->ia, F->ja, F->da + (size_t)g * F->nnz, x, y, n, 0, s); break;
      case 5: csr_mv(F->tia, F->tja, F->tda + (size_t)g * F->nnz, x, y, n, 0, s); break;
      default: return -1;
   }
   NFFT4GP_HIP_CHECK(hipGetLastError());
   return 0;
}

// sum_i dG_g(i,i) / G(i,i) (g = 0..2), or sum_i log(1 / G(i,i)) (g < 0)
double fsai_grad_diag(void* vF, int g, hipStream_t s)
{
   PrecondFsaiAmd* F = (PrecondFsaiAmd*)vF;
   return diag_sum(F, g < 0 ? nullptr : F->da + (size_t)g * F->nnz, s);
}

}  // namespace nfft4gp_amd

extern "C" {

void* Nfft4GPAmdPrecondFsaiCreate(void) { return new PrecondFsaiAmd(); }

void Nfft4GPAmdPrecondFsaiSetLfil(void* str, int lfil)
{
   if (str) ((PrecondFsaiAmd*)str)->lfil = lfil;
}

void Nfft4GPAmdPrecondFsaiSetKernel(void* str, int kernel)
{
   if (str) ((PrecondFsaiAmd*)str)->kernel = kernel ? 1 : 0;
}

void Nfft4GPAmdPrecondFsaiReset(void* str)
{
   if (str) ((PrecondFsaiAmd*)str)->release();  // keeps lfil (fsai.c:60-98)
}

void Nfft4GPAmdPrecondFsaiFree(void* str)
{
   PrecondFsaiAmd* F = (PrecondFsaiAmd*)str;
   if (!F) return;
   F->release();
   delete F;
}

int Nfft4GPAmdPrecondFsaiSetupWithKernel(double* data, int n, int ldim, int d, func_kernel fkernel,
                                         void* fkernel_params, int require_grad, void* vfsai_mat)
{
   PrecondFsaiAmd* F = (PrecondFsaiAmd*)vfsai_mat;
   if (!F || !need_device("Nfft4GPAmdPrecondFsaiSetupWithKernel")) return -1;
   if (!fkernel_params || !data || n <= 0 || ldim < n || d <= 0) {
      fprintf(stderr, "nfft4gp_amd: Nfft4GPAmdPrecondFsaiSetupWithKernel needs data and kernel parameters\n");
      return -1;
   }
   KernelSpec K;
   double* dXk = nullptr;
   if (kernel_spec_of(fkernel_params, fkernel, F->kernel, n, K, &dXk) < 0) return -1;
   hipStream_t s = current_stream();
   double* dX = nullptr;
   if (upload(&dX, (const double*)nullptr, (size_t)ldim * d) ||
       hipMemcpy(dX, data, sizeof(double) * (size_t)ldim * d, hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(dX);
      (void)hipFree(dXk);
      return -1;
   }
   std::vector<int> hia, hja;
   std::vector<double> haa, hda;
   const int rc = fsai_kernel_csr(dX, n, ldim, d, F->lfil, K, nullptr, 0, require_grad, hia, hja, haa, hda, s);
   (void)hipStreamSynchronize(s);
   (void)hipFree(dX);
   (void)hipFree(dXk);
   if (rc) return -1;
   return fsai_load(F, n, hia.data(), hja.data(), haa.data(), require_grad ? hda.data() : nullptr);
}

int Nfft4GPAmdPrecondFsaiSetCsr(void* vfsai_mat, int n, const int* ia, const int* ja, const double* aa,
                                const double* da)
{
   PrecondFsaiAmd* F = (PrecondFsaiAmd*)vfsai_mat;
   if (!F || !ia || !ja || !aa || !need_device("Nfft4GPAmdPrecondFsaiSetCsr")) return -1;
   return fsai_load(F, n, ia, ja, aa, da);
}

int Nfft4GPAmdPrecondFsaiCsr(void* vfsai_mat, int* ia, int* ja, double* aa, double* da)
{
   PrecondFsaiAmd* F = (PrecondFsaiAmd*)vfsai_mat;
   if (!F || !F->ia) return -1;
   const int n = F->n, nnz = F->nnz;
   if (ia) NFFT4GP_HIP_CHECK(hipMemcpy(ia, F->ia, sizeof(int) * (n + 1), hipMemcpyDeviceToHost));
   if (ja) NFFT4GP_HIP_CHECK(hipMemcpy(ja, F->ja, sizeof(int) * nnz, hipMemcpyDeviceToHost));
   if (aa) NFFT4GP_HIP_CHECK(hipMemcpy(aa, F->aa, sizeof(double) * nnz, hipMemcpyDeviceToHost));
   if (da && F->da) NFFT4GP_HIP_CHECK(hipMemcpy(da, F->da, sizeof(double) * 3 * nnz, hipMemcpyDeviceToHost));
   return nnz;
}

int Nfft4GPAmdPrecondFsaiSolve(void* vfsai_mat, int n, double* x, double* rhs)
{
   PrecondFsaiAmd* F = (PrecondFsaiAmd*)vfsai_mat;
   if (!F || !F->ia || n != F->n) return -1;
   hipStream_t s = current_stream();
   Vec vx, vr;
   if (vx.open(x, n, false) || vr.open(rhs, n, true)) return -1;
   csr_mv(F->ia, F->ja, F->aa, vr.d, F->work, n, 0, s);    // work = L rhs
   csr_mv(F->tia, F->tja, F->taa, F->work, vx.d, n, 0, s);  // x = L^T work
   NFFT4GP_HIP_CHECK(hipGetLastError());
   vr.close(false);
   vx.close(true);
   return 0;
}

int Nfft4GPAmdPrecondFsaiInvL(void* vfsai_mat, int n, double* x, double* rhs)
{
   PrecondFsaiAmd* F = (PrecondFsaiAmd*)vfsai_mat;
   if (!F || !F->ia || n != F->n) return -1;
   Vec vx, vr;
   if (vx.open(x, n, false) || vr.open(rhs, n, true)) return -1;
   const int rc = inv_l(F, vx.d, vr.d, current_stream());
   vr.close(false);
   vx.close(rc == 0);
   return rc;
}

int Nfft4GPAmdPrecondFsaiInvLT(void* vfsai_mat, int n, double* x, double* rhs)
{
   PrecondFsaiAmd* F = (PrecondFsaiAmd*)vfsai_mat;
   if (!F || !F->ia || n != F->n) return -1;
   Vec vx, vr;
   if (vx.open(x, n, false) || vr.open(rhs, n, true)) return -1;
   const int rc = inv_lt(F, vx.d, vr.d, current_stream());
   vr.close(false);
   vx.close(rc == 0);
   return rc;
}

int Nfft4GPAmdPrecondFsaiDvp(void* vfsai_mat, int n, int* mask, double* x, double** yp)
{
   PrecondFsaiAmd* F = (PrecondFsaiAmd*)vfsai_mat;
   if (!F || !F->ia || n != F->n) return -1;
   if (!F->grad) {
      printf("Setup FSAI without gradient, trace not supported.\n");  // fsai.c:139-143
      return -1;
   }
   if (!yp) {
      printf("output pointer cannot be NULL\n");
      return -1;
   }
   if (!*yp) {
      if (is_device_ptr(x)) {
         if (hipMalloc((void**)yp, sizeof(double) * 3 * (size_t)n) != hipSuccess) return -1;
         NFFT4GP_HIP_CHECK(hipMemset(*yp, 0, sizeof(double) * 3 * (size_t)n));
      } else {
         *yp = (double*)calloc(3 * (size_t)n, sizeof(double));
      }
   }
   hipStream_t s = current_stream();
   Vec vx, vy;
   if (vx.open(x, n, true) || vy.open(*yp, 3 * (size_t)n, true)) return -1;
   int rc = 0;
   for (int g = 0; g < 3 && !rc; g++)
      if (!mask || mask[g]) rc = dvp_one(F, g, vx.d, vy.d + (size_t)g * n, s);
   vx.close(false);
   vy.close(rc == 0);
   return rc;
}

int Nfft4GPAmdPrecondFsaiTrace(void* vfsai_mat, double** tracesp)
{
   PrecondFsaiAmd* F = (PrecondFsaiAmd*)vfsai_mat;
   if (!F || !F->ia) return -1;
   if (!F->grad) {
      printf("Setup FSAI without gradient, trace not supported.\n");  // fsai.c:225-229
      return -1;
   }
   if (!tracesp) {
      printf("Trace pointer cannot be NULL\n");
      return -1;
   }
   double* traces = *tracesp ? *tracesp : (double*)calloc(3, sizeof(double));
   hipStream_t s = current_stream();
   // the reference adds to what the array holds, then doubles (fsai.c:256-265)
   for (int g = 0; g < 3; g++) traces[g] = 2.0 * (traces[g] + diag_sum(F, F->da + (size_t)g * F->nnz, s));
   *tracesp = traces;
   return 0;
}

double Nfft4GPAmdPrecondFsaiLogdet(void* vfsai_mat)
{
   PrecondFsaiAmd* F = (PrecondFsaiAmd*)vfsai_mat;
   if (!F || !F->ia) return NAN;
   return 2.0 * diag_sum(F, nullptr, current_stream());
}

}  // extern "C"
