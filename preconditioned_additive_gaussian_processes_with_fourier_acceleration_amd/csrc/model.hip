// model.hip -- a fitted GP as a table: the posterior mean at new points without the training data.
//
// After the spread and grid steps of a matvec with alpha = (K + mu I)^{-1} y the plan's d_H holds, per (window,
// cell), the 8 coefficients of the interpolation polynomial (internal.h: H[cell][d]); k_interp evaluates them at
// the training points' own offsets.  Evaluated at any other point of the handle's domain the same table gives
// (1/nw) sum_c K_c(x*, X) alpha: the windows' periodic grids do not know which points are training points.  A
// Model is that table (nw x 64 x kNC doubles) plus each window's feature, centre and scale.
//
// A new point's coordinate in window c is computed exactly as the first setup computes a training point's
// (nfft_api.cpp centre_and_scale + quantize): xs = (x - centre) * scale, then round-to-nearest of xs 2^32 mod
// 2^32; cell = the top 6 bits, s = the slot word without index bits (internal.h slot_word).  A training point
// therefore lands on its own cell and, up to the layout's sub-quantum index bits (<= 8 units of 2^-32 of a
// cell; 2048 in the 32-bit mode), its own offset.
//
// Domain: |xs| <= 1/4 + 2^-33 in every window.  The reference scales the training points of a window to radius
// 1/4 (nfft_interface.c:150-213) so that every pair of them is within the distance 1/2 up to which the
// regularised periodic kernel is the kernel; a new point within that radius has the same guarantee, one outside
// it does not (NaN, counted).  The half fixed-point unit of slack keeps inside the training point that defines
// the radius, whose (x - c) * (0.25 / r) may round one ulp above 1/4.
//
// The second half of the file is the predictive standard deviation: the operator's finite-rank form gives the
// posterior variance as a quadratic form in a point's trigonometric features (see "the predictive variance").
// The last part draws from the joint posterior: S is factored once and a set of sample paths is a matrix of weights
// on the same features, evaluated at any point set by k_model_paths (see "joint posterior sample paths").
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "internal.h"
#include "quad_walk.hpp"

namespace nfft4gp_amd {
namespace {

constexpr int kMpThreads = 256;
constexpr int kMpPts = 4;                  // points per thread (strided by the workgroup: coalesced columns)
constexpr int kMpGroup = 8;                // windows staged in LDS per pass (8 x 513 doubles = 32.8 KB)
constexpr int kMpWin = kNC * kNos + 1;     // [window][degree][cell], windows 513 doubles apart (k_interp_hl)

struct Model {
   int nw = 0, d = 0, kernel = 0;
   double f = 1.0, l = 1.0, mu = 0.0;
   std::vector<double> centre, scale;  // host copies
   std::vector<int> feature;
   double* d_H = nullptr;       // [nw][64][kNC]
   double* d_centre = nullptr;  // [nw]
   double* d_scale = nullptr;   // [nw]
   int* d_feature = nullptr;    // [nw]
   unsigned int* d_cnt = nullptr;  // per-workgroup counts of outside points (grown on demand)
   size_t cnt_cap = 0;
   double* d_S = nullptr;  // the variance matrix, mv_order(nw)^2, symmetric, windows kMvPad slots apart; or none
   int R = 0;              // 33 nw once a variance is held, else 0
   double fit_ms[3] = {0.0, 0.0, 0.0};  // the last fit's wall clock: features, Grams and their sum, system + LU
   // the sampler (see "joint posterior sample paths"): S+ = F F^T and the drawn paths' weights B = F xi
   double* d_Ft = nullptr;  // F^T, R x R_p column-major: column slot(j) is F's row j, the padded slots' columns zero
   double* d_Bt = nullptr;  // B^T, nsp x R_p column-major, nsp = ns rounded up to the sample tile; rows >= ns zero
   int ns = 0, nsp = 0;
   double defect = 0.0, lam_min = 0.0, lam_max = 0.0;  // sum |lambda < 0| / sum |lambda| and S's extreme eigenvalues
   double sampler_ms = 0.0;                            // the eigendecomposition's wall clock
};

// S has changed or goes: the factor of the old one and the paths drawn from it go with it
void model_drop_sampler(Model* M)
{
   if (M->d_Ft) (void)hipFree(M->d_Ft);
   if (M->d_Bt) (void)hipFree(M->d_Bt);
   M->d_Ft = M->d_Bt = nullptr;
   M->ns = M->nsp = 0;
}

void model_free(Model* M)
{
   if (!M) return;
   model_drop_sampler(M);
   if (M->d_S) (void)hipFree(M->d_S);
   if (M->d_H) (void)hipFree(M->d_H);
   if (M->d_centre) (void)hipFree(M->d_centre);
   if (M->d_scale) (void)hipFree(M->d_scale);
   if (M->d_feature) (void)hipFree(M->d_feature);
   if (M->d_cnt) (void)hipFree(M->d_cnt);
   delete M;
}

// One thread owns kMpPts points and walks the windows in order, group by group: the group's rows of the table are
// staged in LDS transposed to [window][degree][cell]; per (point, window) one coalesced 8-byte load of the
// point's coordinate, the cell / offset decode, 8 LDS reads and a Horner.  Each point's windows are added in
// the order c = 0 .. nw - 1 by its own thread: no atomics, the same bits however the points are batched.
// Measured at config C's shapes (n_new = 1e6, 32 windows; tools/model_probe.py, profiles/model_probe.json): 82.6 us,
// 3.2 TB/s of the 264 MB coordinate stream; the variant that gathered each 64-byte row from L2 instead of staging
// the table took 169.5 us (profiles/model_predict_ab.txt) and was removed.
__global__ __launch_bounds__(kMpThreads) void k_model_predict(const double* __restrict__ H,
                                                              const double* __restrict__ centre,
                                                              const double* __restrict__ scale,
                                                              const int* __restrict__ feature, int nw,
                                                              const double* __restrict__ X, long long ldim, int n_new,
                                                              double ff, double* __restrict__ mean,
                                                              unsigned int* __restrict__ cnt_out)
{
   __shared__ double s_H[kMpGroup * kMpWin];
   __shared__ unsigned int s_cnt[kMpThreads / kWave];
   const int tid = threadIdx.x;
   const long long base = (long long)blockIdx.x * (kMpThreads * kMpPts) + tid;
   double acc[kMpPts];
   bool outside[kMpPts];
#pragma unroll
   for (int p = 0; p < kMpPts; p++) {
      acc[p] = 0.0;
      outside[p] = false;
   }
   for (int c0 = 0; c0 < nw; c0 += kMpGroup) {
      const int ng = min(kMpGroup, nw - c0);
      if (c0) __syncthreads();  // every thread has left the previous group's rows
      {
         const double2* src = reinterpret_cast<const double2*>(H + (size_t)c0 * kNos * kNC);
         const int pairs = ng * kNos * kNC / 2;
         for (int i = tid; i < pairs; i += kMpThreads) {
            const double2 v = src[i];
            const int e = 2 * i;  // element of [window][cell][degree]
            double* row = s_H + (e / (kNos * kNC)) * kMpWin + ((e / kNC) & (kNos - 1));
            const int dg = e & (kNC - 1);
            row[dg * kNos] = v.x;
            row[(dg + 1) * kNos] = v.y;
         }
      }
      __syncthreads();
      for (int cl = 0; cl < ng; cl++) {
         const int c = c0 + cl;
         const double ctr = centre[c], sc = scale[c];
         const double* col = X + (size_t)feature[c] * (size_t)ldim;
         double xv[kMpPts];
#pragma unroll
         for (int p = 0; p < kMpPts; p++) {
            const long long i = base + (long long)p * kMpThreads;
            xv[p] = (i < n_new) ? col[i] : ctr;
         }
#pragma unroll
         for (int p = 0; p < kMpPts; p++) {
            const double xs = (xv[p] - ctr) * sc;         // subtract, then multiply: the setup's two roundings
            const bool in = fabs(xs) <= kMpLimit;         // false for NaN and infinities too
            outside[p] = outside[p] || !in;
            const double xq = in ? xs : 0.0;
            const uint32_t q = (uint32_t)(unsigned long long)llround(xq * 4294967296.0);  // quantize()
            const uint32_t cell = q >> 26;
            const double s = (double)(int)(((q & 0x3FFFFFFu) << 6) ^ 0x80000000u);  // slot_word, no index bits
            const double* hrow = s_H + cl * kMpWin + cell;
            double hc[kNC];
#pragma unroll
            for (int dg = 0; dg < kNC; dg++) hc[dg] = hrow[dg * kNos];
            double v = hc[kNC - 1];
#pragma unroll
            for (int dg = kNC - 2; dg >= 0; dg--) v = fma(v, s, hc[dg]);
            acc[p] += v;
         }
      }
   }
   unsigned int cnt = 0;
#pragma unroll
   for (int p = 0; p < kMpPts; p++) {
      const long long i = base + (long long)p * kMpThreads;
      const bool live = i < n_new;
      if (live) mean[i] = outside[p] ? __builtin_nan("") : ff * acc[p];
      cnt += (unsigned int)__popcll(__ballot(live && outside[p]));
   }
   if (cnt_out) {
      if ((tid & (kWave - 1)) == 0) s_cnt[tid / kWave] = cnt;
      __syncthreads();
      if (tid == 0) {
         unsigned int t = 0;
         for (int w = 0; w < kMpThreads / kWave; w++) t += s_cnt[w];
         cnt_out[blockIdx.x] = t;
      }
   }
}

template <class T>
int to_device(T** dptr, const T* h, size_t count)
{
   NFFT4GP_HIP_CHECK(hipMalloc((void**)dptr, sizeof(T) * std::max<size_t>(1, count)));
   NFFT4GP_HIP_CHECK(hipMemcpy(*dptr, h, sizeof(T) * count, hipMemcpyHostToDevice));
   return 0;
}

// the device side of a model whose host fields are filled; H: nw * 64 * kNC doubles on the host, or NULL to
// leave d_H allocated and unwritten
int model_upload(Model* M, const double* H)
{
   const size_t nh = (size_t)M->nw * kNos * kNC;
   if (H) {
      if (to_device(&M->d_H, H, nh)) return -1;
   } else {
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&M->d_H, sizeof(double) * nh));
   }
   if (to_device(&M->d_centre, M->centre.data(), (size_t)M->nw) ||
       to_device(&M->d_scale, M->scale.data(), (size_t)M->nw) ||
       to_device(&M->d_feature, M->feature.data(), (size_t)M->nw))
      return -1;
   return 0;
}

int model_predict(Model* M, const double* Xnew, int n_new, long long ldim, double* mean, long long* n_outside)
{
   hipStream_t s = current_stream();
   const bool xdev = is_device_ptr(Xnew), mdev = is_device_ptr(mean);
   double *xs = nullptr, *ms = nullptr;  // staging of host arrays
   const double* dX = Xnew;
   double* dmean = mean;
   int rc = 0;
   auto body = [&]() -> int {
      if (!xdev) {
         NFFT4GP_HIP_CHECK(hipMalloc((void**)&xs, sizeof(double) * (size_t)n_new * M->d));
         NFFT4GP_HIP_CHECK(hipMemcpy2DAsync(xs, sizeof(double) * (size_t)n_new, Xnew, sizeof(double) * (size_t)ldim,
                                            sizeof(double) * (size_t)n_new, (size_t)M->d, hipMemcpyHostToDevice, s));
         dX = xs;
         ldim = n_new;
      }
      if (!mdev) {
         NFFT4GP_HIP_CHECK(hipMalloc((void**)&ms, sizeof(double) * (size_t)n_new));
         dmean = ms;
      }
      const int per = kMpThreads * kMpPts;
      const size_t nblk = ((size_t)n_new + per - 1) / per;
      if (n_outside && nblk > M->cnt_cap) {
         if (M->d_cnt) (void)hipFree(M->d_cnt);
         M->d_cnt = nullptr;
         M->cnt_cap = 0;
         NFFT4GP_HIP_CHECK(hipMalloc((void**)&M->d_cnt, sizeof(unsigned int) * nblk));
         M->cnt_cap = nblk;
      }
      hipLaunchKernelGGL(k_model_predict, dim3((unsigned int)nblk), dim3(kMpThreads), 0, s, (const double*)M->d_H,
                         (const double*)M->d_centre, (const double*)M->d_scale, (const int*)M->d_feature, M->nw, dX,
                         ldim, n_new, M->f * M->f, dmean, n_outside ? M->d_cnt : (unsigned int*)nullptr);
      NFFT4GP_HIP_CHECK(hipGetLastError());
      if (!mdev)
         NFFT4GP_HIP_CHECK(hipMemcpyAsync(mean, ms, sizeof(double) * (size_t)n_new, hipMemcpyDeviceToHost, s));
      if (n_outside) {
         std::vector<unsigned int> h(nblk);
         NFFT4GP_HIP_CHECK(hipMemcpyAsync(h.data(), M->d_cnt, sizeof(unsigned int) * nblk, hipMemcpyDeviceToHost, s));
         NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
         long long t = 0;
         for (unsigned int v : h) t += v;
         *n_outside = t;
      } else if (!xdev || !mdev) {
         NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
      }
      return 0;
   };
   rc = body();
   if (xs || ms) (void)hipStreamSynchronize(s);  // (error paths) nothing in flight reads the staging buffers
   if (xs) (void)hipFree(xs);
   if (ms) (void)hipFree(ms);
   return rc;
}

// ---- the predictive variance ---------------------------------------------------------------------------------
// With 1-D windows the operator is a finite-rank kernel, A = f^2 (Z W Z^T + mu I): Z holds per window the 33
// features [cos 2 pi k xs, k = 0..16 | sin 2 pi k xs, k = 1..16] of the window's scaled coordinate and W is
// diagonal (feature_weights).  The posterior variance at a point with features phi is f^2 (mu + phi^T S phi) with
// S = mu (mu I + W G)^{-1} W, G = Z^T Z over the training points: no solve and no training data at serving time.
// W has negative entries (the regularised periodic kernel's b^ are not all positive), so mu I + W G is solved as
// the nonsymmetric matrix it is, by LU; S itself is symmetric (W - W G (mu I + W G)^{-1} W) and is stored as
// (S + S^T) / 2.  Internally a window takes kMvPad = 36 slots (33 features and 3 zeros: a whole number of MFMA k
// steps) and the windows are padded to a multiple of 4 (k_model_std's column tile), R_p = 36 * 4 ceil(nw / 4); the
// added slots have zero features and zero weight, so mu I + W G keeps mu on their diagonal and S is zero there.
// (the slot constants, mv_order, mv_angle and mv_rotate are internal.h's: feature_gp.hip shares them)

// per workgroup the number of rows with a coordinate outside some window's domain
__global__ __launch_bounds__(256) void k_model_outside(const double* __restrict__ centre,
                                                       const double* __restrict__ scale,
                                                       const int* __restrict__ feature, int nw,
                                                       const double* __restrict__ X, long long ldim, int n,
                                                       unsigned int* __restrict__ cnt_out)
{
   __shared__ unsigned int s_cnt[256 / kWave];
   const int tid = threadIdx.x;
   const long long i = (long long)blockIdx.x * 256 + tid;
   bool out = false;
   if (i < n)
      for (int c = 0; c < nw; c++) {
         const double xs = (X[(size_t)feature[c] * (size_t)ldim + i] - centre[c]) * scale[c];
         out = out || !(fabs(xs) <= kMpLimit);
      }
   const unsigned int cnt = (unsigned int)__popcll(__ballot(out));
   if ((tid & (kWave - 1)) == 0) s_cnt[tid / kWave] = cnt;
   __syncthreads();
   if (tid == 0) {
      unsigned int t = 0;
      for (int w = 0; w < 256 / kWave; w++) t += s_cnt[w];
      cnt_out[blockIdx.x] = t;
   }
}

// Z[(36 c + j) ldz + i] = feature j of window c at point i0 + i, i < cnt: a chunk of Z, column-major [feature][point];
// blockIdx.y runs over the padded windows, those >= nw are zero
__global__ __launch_bounds__(256) void k_model_features(const double* __restrict__ centre,
                                                        const double* __restrict__ scale,
                                                        const int* __restrict__ feature, int nw,
                                                        const double* __restrict__ X, long long ldim, long long i0,
                                                        int cnt, double* __restrict__ Z, long long ldz)
{
   const int i = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
   if (i >= cnt) return;
   double* z = Z + (size_t)c * kMvPad * ldz + i;
   if (c >= nw) {
      for (int j = 0; j < kMvPad; j++) z[j * ldz] = 0.0;
      return;
   }
   double c1, s1;
   (void)mv_angle(X[(size_t)feature[c] * (size_t)ldim + i0 + i], centre[c], scale[c], c1, s1);
   double ck = 1.0, sk = 0.0;
#pragma unroll
   for (int k = 0; k <= 16; k++) {
      z[k * ldz] = ck;
      if (k) z[(16 + k) * ldz] = sk;
      mv_rotate(ck, sk, c1, s1);
   }
   for (int j = kMvFeat; j < kMvPad; j++) z[j * ldz] = 0.0;
}

// Z^T y and y^T y without Z: part[block][slot] = the block's sum of feature(slot) y over its points, slot R_p the
// block's sum of y^2.  A thread owns kZyPts points (strided by the workgroup) and regenerates their features window
// by window as k_model_features does (the same bits); each of a window's 33 sums folds over the wave in a fixed
// butterfly, then over the 4 waves in wave order.  k_model_sum_parts adds the blocks in block order: no atomics, the
// same bits every time.
constexpr int kZyThreads = 256, kZyPts = 4;

__device__ inline double zy_wave_sum(double v)
{
#pragma unroll
   for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
   return v;
}

__global__ __launch_bounds__(kZyThreads) void k_model_zty(const double* __restrict__ centre,
                                                          const double* __restrict__ scale,
                                                          const int* __restrict__ feature, int nw,
                                                          const double* __restrict__ X, long long ldim, int n,
                                                          const double* __restrict__ y, int Rp,
                                                          double* __restrict__ part)
{
   __shared__ double s_w[kZyThreads / kWave][kMvPad];
   const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
   const long long base = (long long)blockIdx.x * (kZyThreads * kZyPts) + tid;
   double* out = part + (size_t)blockIdx.x * (Rp + 1);
   double yv[kZyPts];
   double yy = 0.0;
#pragma unroll
   for (int p = 0; p < kZyPts; p++) {
      const long long i = base + (long long)p * kZyThreads;
      yv[p] = (i < n) ? y[i] : 0.0;  // a point past the end adds exact zeros
      yy = fma(yv[p], yv[p], yy);
   }
   yy = zy_wave_sum(yy);
   if (lane == 0) s_w[wave][0] = yy;
   __syncthreads();
   if (tid == 0) out[Rp] = ((s_w[0][0] + s_w[1][0]) + s_w[2][0]) + s_w[3][0];
   for (int c = 0; c < Rp / kMvPad; c++) {
      __syncthreads();  // the previous window's sums have been read
      if (c >= nw) {    // a padded window (uniform over the workgroup)
         if (tid < kMvPad) out[c * kMvPad + tid] = 0.0;
         continue;
      }
      const double ctr = centre[c], sc = scale[c];
      const double* col = X + (size_t)feature[c] * (size_t)ldim;
      double c1[kZyPts], s1[kZyPts], ck[kZyPts], sk[kZyPts];
#pragma unroll
      for (int p = 0; p < kZyPts; p++) {
         const long long i = base + (long long)p * kZyThreads;
         (void)mv_angle((i < n) ? col[i] : ctr, ctr, sc, c1[p], s1[p]);
         ck[p] = 1.0;
         sk[p] = 0.0;
      }
#pragma unroll
      for (int k = 0; k <= 16; k++) {
         double vc = 0.0, vs = 0.0;
#pragma unroll
         for (int p = 0; p < kZyPts; p++) {
            vc = fma(yv[p], ck[p], vc);
            vs = fma(yv[p], sk[p], vs);
            mv_rotate(ck[p], sk[p], c1[p], s1[p]);
         }
         vc = zy_wave_sum(vc);
         if (lane == 0) s_w[wave][k] = vc;
         if (k) {
            vs = zy_wave_sum(vs);
            if (lane == 0) s_w[wave][16 + k] = vs;
         }
      }
      __syncthreads();
      if (tid < kMvPad)
         out[c * kMvPad + tid] = tid < kMvFeat ? ((s_w[0][tid] + s_w[1][tid]) + s_w[2][tid]) + s_w[3][tid] : 0.0;
   }
}

// out[slot] = sum over the blocks of part[block][slot], in block order
__global__ void k_model_sum_parts(const double* __restrict__ part, int nblk, int count, double* __restrict__ out)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= count) return;
   double v = 0.0;
   for (int b = 0; b < nblk; b++) v += part[(size_t)b * count + i];
   out[i] = v;
}

__global__ void k_model_add(double* __restrict__ G, const double* __restrict__ Gc, long long count)
{
   const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
   if (i < count) G[i] += Gc[i];
}

// A = mu I + W G and B = mu W (both R_p x R_p column-major): S = A^{-1} B
__global__ void k_model_system(const double* __restrict__ G, const double* __restrict__ w, int Rp, double mu,
                               double* __restrict__ A, double* __restrict__ B)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
   if (i >= Rp) return;
   const size_t e = i + (size_t)j * Rp;
   A[e] = w[i] * G[e] + (i == j ? mu : 0.0);
   B[e] = (i == j) ? mu * w[i] : 0.0;
}

__global__ void k_model_symmetrise(const double* __restrict__ B, int Rp, double* __restrict__ S)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
   if (i < Rp) S[i + (size_t)j * Rp] = 0.5 * (B[i + (size_t)j * Rp] + B[j + (size_t)i * Rp]);
}

// points per chunk of Z: the chunk stays <= 256 MB
int chunk_points(int n, int Rp)
{
   const long long cap = std::max<long long>(1024, (32LL << 20) / Rp / 16 * 16);
   return (int)std::min<long long>(n, cap);
}

// b^ (index k + 16) -> the 33 weights: [cos 0] = b^_0 / nw, [cos k] = [sin k] = 2 b^_k / nw (k = 1..15),
// [cos 16] = [sin 16] = b^_{-16} / nw (the band's one unpaired mode)
void weight_map(const double* bh, double mult, int nw, double* w33)
{
   w33[0] = mult * bh[16] / nw;
   for (int k = 1; k <= 15; k++) w33[k] = w33[16 + k] = mult * (2.0 * bh[16 + k]) / nw;
   w33[16] = w33[32] = mult * bh[0] / nw;
}

}  // namespace

// the 33 weights of one window, from the kernel's b^ at plan_setup's comp_sigma
void feature_weights(int kernel, double l, double scale, int nw, double* w33)
{
   double bh[kBand];
   const double sig = (kernel == 0) ? l * scale * std::sqrt(2.0) : l * scale;
   bhat_1d(kernel == 0 ? 0 : 2, sig, bh);
   weight_map(bh, 1.0, nw, w33);
}

// dW / dl: the same map of the derivative kernel's b^ times plan_setup's dscale (what the gradient matvec applies)
void feature_weights_grad(int kernel, double l, double scale, int nw, double* dw33)
{
   double bh[kBand];
   const double sig = (kernel == 0) ? l * scale * std::sqrt(2.0) : l * scale;
   bhat_1d(kernel == 0 ? 1 : 3, sig, bh);
   const double dscale = (kernel == 0) ? 2.0 * scale * std::sqrt(2.0) / sig : scale / sig;
   weight_map(bh, dscale, nw, dw33);
}

int sum_parts_dev(const double* part, int nblk, int count, double* out, hipStream_t s)
{
   hipLaunchKernelGGL(k_model_sum_parts, dim3((count + 255) / 256), dim3(256), 0, s, part, nblk, count, out);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   return 0;
}

int window_count_outside(const WindowMap& W, const double* dX, long long ld, int n, hipStream_t s, long long* outside)
{
   const size_t nblk = ((size_t)n + 255) / 256;
   unsigned int* d_cnt = nullptr;
   NFFT4GP_HIP_CHECK(hipMalloc((void**)&d_cnt, sizeof(unsigned int) * std::max<size_t>(1, nblk)));
   std::vector<unsigned int> h(nblk);
   hipLaunchKernelGGL(k_model_outside, dim3((unsigned int)nblk), dim3(256), 0, s, W.centre, W.scale, W.feature, W.nw,
                      dX, ld, n, d_cnt);
   const bool ok = hipGetLastError() == hipSuccess &&
                   hipMemcpyAsync(h.data(), d_cnt, sizeof(unsigned int) * nblk, hipMemcpyDeviceToHost, s) == hipSuccess &&
                   hipStreamSynchronize(s) == hipSuccess;
   (void)hipFree(d_cnt);
   if (!ok) return -1;
   long long t = 0;
   for (unsigned int v : h) t += v;
   *outside = t;
   return 0;
}

// Z in chunks -> their Grams (gram_tn: split sum in a fixed order) added in chunk order; Z^T y and y^T y by
// k_model_zty (b and yy must be contiguous: b + R_p == yy)
int window_moments(const WindowMap& W, const double* dX, long long ld, int n, const double* dy, double* G, double* b,
                   double* yy, double* ms2, hipStream_t s)
{
   const int Rp = mv_order(W.nw);
   const size_t rr = (size_t)Rp * Rp;
   double *Z = nullptr, *Gc = nullptr, *part = nullptr;
   auto body = [&]() -> int {
      if (dy) {
         if (yy != b + Rp) return -1;
         const int per = kZyThreads * kZyPts;
         const int nblk = (int)(((long long)n + per - 1) / per);
         NFFT4GP_HIP_CHECK(hipMalloc((void**)&part, sizeof(double) * (size_t)nblk * (Rp + 1)));
         hipLaunchKernelGGL(k_model_zty, dim3(nblk), dim3(kZyThreads), 0, s, W.centre, W.scale, W.feature, W.nw, dX, ld,
                            n, dy, Rp, part);
         if (sum_parts_dev(part, nblk, Rp + 1, b, s)) return -1;
         if (!G) {
            NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
            return 0;
         }
      }
      const int chunk = chunk_points(n, Rp);
      const long long ldz = ((long long)chunk + 15) / 16 * 16;
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&Z, sizeof(double) * (size_t)ldz * Rp));
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&Gc, sizeof(double) * rr));
      NFFT4GP_HIP_CHECK(hipMemsetAsync(G, 0, sizeof(double) * rr, s));
      NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
      double ms[2] = {0.0, 0.0};
      auto t0 = std::chrono::steady_clock::now();
      auto lap = [&](int which) {  // the stream is idle: gram_tn synchronises
         const auto t1 = std::chrono::steady_clock::now();
         ms[which] += std::chrono::duration<double, std::milli>(t1 - t0).count();
         t0 = t1;
      };
      for (long long i0 = 0; i0 < n; i0 += chunk) {
         const int cnt = (int)std::min<long long>(chunk, n - i0);
         hipLaunchKernelGGL(k_model_features, dim3((cnt + 255) / 256, Rp / kMvPad), dim3(256), 0, s, W.centre, W.scale,
                            W.feature, W.nw, dX, ld, i0, cnt, Z, ldz);
         NFFT4GP_HIP_CHECK(hipGetLastError());
         NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
         lap(0);
         if (gram_tn(Rp, Rp, cnt, Z, ldz, Z, ldz, Gc, 1, s)) return -1;
         lap(1);
         hipLaunchKernelGGL(k_model_add, dim3((unsigned int)((rr + 255) / 256)), dim3(256), 0, s, G,
                            (const double*)Gc, (long long)rr);
         NFFT4GP_HIP_CHECK(hipGetLastError());
      }
      NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
      lap(1);
      if (ms2) ms2[0] = ms[0], ms2[1] = ms[1];
      return 0;
   };
   const int rc = body();
   (void)hipStreamSynchronize(s);
   for (double* p : {Z, Gc, part})
      if (p) (void)hipFree(p);
   return rc;
}

namespace {

// X (n x d, ld ldim; host or device) as a device array: *dX, *ld; *owned is to be freed by the caller
int stage_points(const Model* M, const double* X, int n, long long ldim, hipStream_t s, const double** dX,
                 long long* ld, double** owned)
{
   *owned = nullptr;
   *dX = X;
   *ld = ldim;
   if (is_device_ptr(X)) return 0;
   NFFT4GP_HIP_CHECK(hipMalloc((void**)owned, sizeof(double) * (size_t)n * M->d));
   NFFT4GP_HIP_CHECK(hipMemcpy2DAsync(*owned, sizeof(double) * (size_t)n, X, sizeof(double) * (size_t)ldim,
                                      sizeof(double) * (size_t)n, (size_t)M->d, hipMemcpyHostToDevice, s));
   *dX = *owned;
   *ld = n;
   return 0;
}

int grow_counts(Model* M, size_t nblk)
{
   if (nblk <= M->cnt_cap) return 0;
   if (M->d_cnt) (void)hipFree(M->d_cnt);
   M->d_cnt = nullptr;
   M->cnt_cap = 0;
   NFFT4GP_HIP_CHECK(hipMalloc((void**)&M->d_cnt, sizeof(unsigned int) * nblk));
   M->cnt_cap = nblk;
   return 0;
}

int read_counts(Model* M, size_t nblk, hipStream_t s, long long* total)
{
   std::vector<unsigned int> h(nblk);
   NFFT4GP_HIP_CHECK(hipMemcpyAsync(h.data(), M->d_cnt, sizeof(unsigned int) * nblk, hipMemcpyDeviceToHost, s));
   NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
   long long t = 0;
   for (unsigned int v : h) t += v;
   *total = t;
   return 0;
}

// The fit: G = Z^T Z (window_moments) -> mu I + W G -> LU -> S.  Every step is deterministic, so two fits give the
// same bits.  Returns 0, -1, or -2 (rows outside).
int model_fit_variance(Model* M, const double* X, int n, long long ldim)
{
   hipStream_t s = current_stream();
   const int nw = M->nw, Rp = mv_order(nw);
   const size_t rr = (size_t)Rp * Rp;
   double *xown = nullptr, *G = nullptr, *Gc = nullptr, *A = nullptr, *S = nullptr, *d_w = nullptr;
   auto body = [&]() -> int {
      const double* dX;
      long long ld;
      if (stage_points(M, X, n, ldim, s, &dX, &ld, &xown)) return -1;
      const WindowMap W{nw, M->d, M->d_centre, M->d_scale, M->d_feature};
      long long outside = 0;
      if (window_count_outside(W, dX, ld, n, s, &outside)) return -1;
      if (outside) {
         fprintf(stderr, "nfft4gp_amd: Nfft4GPAmdModelFitVariance: %lld of %d rows lie outside the model's domain; "
                         "the model is unchanged.\n", outside, n);
         return -2;
      }
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&G, sizeof(double) * rr));
      double ms[3] = {0.0, 0.0, 0.0};
      if (window_moments(W, dX, ld, n, nullptr, G, nullptr, nullptr, ms, s)) return -1;
      const auto t0 = std::chrono::steady_clock::now();
      std::vector<double> w((size_t)Rp, 0.0);
      for (int c = 0; c < nw; c++) feature_weights(M->kernel, M->l, M->scale[c], nw, w.data() + (size_t)c * kMvPad);
      if (to_device(&d_w, w.data(), w.size())) return -1;
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&Gc, sizeof(double) * rr));
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&A, sizeof(double) * rr));
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&S, sizeof(double) * rr));
      const dim3 g2((Rp + 255) / 256, Rp);
      hipLaunchKernelGGL(k_model_system, g2, dim3(256), 0, s, (const double*)G, (const double*)d_w, Rp, M->mu, A, Gc);
      NFFT4GP_HIP_CHECK(hipGetLastError());
      if (const int info = lu_solve_dev(A, Rp, Gc, Rp, s)) {
         fprintf(stderr, "nfft4gp_amd: Nfft4GPAmdModelFitVariance: the LU of mu I + W G failed (%d)%s.\n", info,
                 M->mu == 0.0 ? "; mu is 0" : "");
         return -1;
      }
      hipLaunchKernelGGL(k_model_symmetrise, g2, dim3(256), 0, s, (const double*)Gc, Rp, S);
      NFFT4GP_HIP_CHECK(hipGetLastError());
      NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
      ms[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      for (int i = 0; i < 3; i++) M->fit_ms[i] = ms[i];
      std::swap(M->d_S, S);  // the previous matrix, if any, is freed below
      M->R = kMvFeat * nw;
      model_drop_sampler(M);
      return 0;
   };
   const int rc = body();
   (void)hipStreamSynchronize(s);
   for (double* p : {xown, G, Gc, A, S, d_w})
      if (p) (void)hipFree(p);
   return rc;
}

// ---- serving: std = sqrt| f^2 (mu + phi^T S phi) | ---------------------------------------------------------------
// k_model_std: one workgroup owns 128 points; phi^T S phi is quad_walk.hpp's walk of S on v_mfma_f64_16x16x4_f64
// (column tiles of 4 windows, k steps of one window, features generated into LDS, the symmetric half-walk, double
// buffering; a point's bits depend on neither its place in the batch nor the batch size).
// Measured at n_new = 1e6, 32 windows (tools/model_std_probe.py; profiles/model_std_ab.txt): 28.9 ms, 49 % of the
// fp64 matrix peak counted at n_new R^2 flops; without the symmetry 50.2 ms; the composed route (a feature kernel,
// gemm_f64 and a row dot, in chunks) 72.3 ms with the same values to 2e-15.  Both were removed.
__global__ __launch_bounds__(kMsThreads) void k_model_std(const double* __restrict__ S, int Rp,
                                                          const double* __restrict__ centre,
                                                          const double* __restrict__ scale,
                                                          const int* __restrict__ feature, int nw,
                                                          const double* __restrict__ X, long long ldim, int n_new,
                                                          double ff, double noise, double* __restrict__ out,
                                                          unsigned int* __restrict__ cnt_out)
{
   extern __shared__ double m_smem[];
   __shared__ unsigned int s_cnt[kMsThreads / kWave];
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
   const int p = tid & (kMsPts - 1), part = tid >> 7;
   const long long ip = (long long)blockIdx.x * kMsPts + p;
   const bool live = ip < n_new;
   quad_zero_pad(m_smem);
   const QuadPoints Q{centre, scale, feature, nw, X, ldim, ip, live};
   const double psum = quad_walk<0>(S, Rp, Q, m_smem, false, nullptr, 0, nullptr);
   __syncthreads();
   double* s_q = m_smem + kMvPad * kMsLdA;  // [point]
   quad_fold(psum, s_q);
   __syncthreads();
   bool outside = false;
   if (part == 0 && live) {
      for (int c = 0; c < nw; c++) {
         const double xs = (X[(size_t)feature[c] * (size_t)ldim + ip] - centre[c]) * scale[c];
         outside = outside || !(fabs(xs) <= kMpLimit);
      }
      out[ip] = outside ? __builtin_nan("") : sqrt(fabs(ff * (noise + s_q[p])));
   }
   if (cnt_out) {
      const unsigned int cnt = (unsigned int)__popcll(__ballot(outside));
      if (lane == 0) s_cnt[wave] = cnt;
      __syncthreads();
      if (tid == 0) {
         unsigned int tsum = 0;
         for (int w = 0; w < kMsThreads / kWave; w++) tsum += s_cnt[w];
         cnt_out[blockIdx.x] = tsum;
      }
   }
}

int model_predict_std(Model* M, const double* Xnew, int n_new, long long ldim, double* std_out, int with_noise,
                      long long* n_outside)
{
   hipStream_t s = current_stream();
   const int nw = M->nw, Rp = mv_order(nw);
   const bool odev = is_device_ptr(std_out);
   double *xown = nullptr, *oown = nullptr;
   const double ff = M->f * M->f, noise = with_noise ? M->mu : 0.0;
   auto body = [&]() -> int {
      const double* dX;
      long long ld;
      if (stage_points(M, Xnew, n_new, ldim, s, &dX, &ld, &xown)) return -1;
      double* dout = std_out;
      if (!odev) {
         NFFT4GP_HIP_CHECK(hipMalloc((void**)&oown, sizeof(double) * (size_t)n_new));
         dout = oown;
      }
      static const bool attr = []() {
         (void)hipFuncSetAttribute((const void*)k_model_std, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMsLds);
         (void)hipGetLastError();
         return true;
      }();
      (void)attr;
      const size_t nblk = ((size_t)n_new + kMsPts - 1) / kMsPts;
      if (n_outside && grow_counts(M, nblk)) return -1;
      hipLaunchKernelGGL(k_model_std, dim3((unsigned int)nblk), dim3(kMsThreads), kMsLds, s, (const double*)M->d_S, Rp,
                         (const double*)M->d_centre, (const double*)M->d_scale, (const int*)M->d_feature, nw, dX, ld,
                         n_new, ff, noise, dout, n_outside ? M->d_cnt : (unsigned int*)nullptr);
      NFFT4GP_HIP_CHECK(hipGetLastError());
      if (!odev)
         NFFT4GP_HIP_CHECK(hipMemcpyAsync(std_out, oown, sizeof(double) * (size_t)n_new, hipMemcpyDeviceToHost, s));
      if (n_outside) {
         if (read_counts(M, nblk, s, n_outside)) return -1;
      } else if (xown || oown) {
         NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
      }
      return 0;
   };
   const int rc = body();
   if (xown || oown) (void)hipStreamSynchronize(s);
   for (double* p : {xown, oown})
      if (p) (void)hipFree(p);
   return rc;
}

// ---- the windows one by one: effect[i][c] = f^2 Horner(H_c), effect_std[i][c] = sqrt| f^2 phi_c^T S_cc phi_c | ------
// f = sum_c g_c is a sum of independent terms a priori; a posteriori g_c(x_c) has mean k_c^T alpha, the value
// k_model_predict adds for window c, and variance f^2 phi_c^T W_c phi_c - k_c^T A^{-1} k_c = f^2 phi_c^T S_cc phi_c,
// S_cc the window's 33 x 33 diagonal block of S (no noise term).  The constant b^_0 / nw sits in every window and only
// the windows' sum of it is identified by the data, so a window's raw std carries the constant's uncertainty.
//
// k_model_effects: k_model_predict's walk (the group's tables staged in LDS, one coalesced coordinate load per
// (point, window), the same decode and Horner) over the windows [w0, w0 + wn), storing each window's ff * v in its
// own column instead of adding them.  With kStd the point's thread also generates the window's 33 features
// (mv_angle / mv_rotate: k_model_std's and fit_variance's bits) and forms phi^T S_cc phi over the upper triangle, row
// by row, the diagonal once and the off-diagonal sum doubled: 561 FMAs and 33 closing steps per (point, window).  S_cc
// is the same for every lane: the group's blocks are staged in LDS next to its tables (two windows per pass with kStd)
// and read by broadcast, each read shared by the thread's two points.  A (point, window) pair outside the window's
// domain is NaN in both columns; the count is of points with any such pair in the range.  No atomics; a point's
// values depend on neither its place in the batch nor n_new.
// Measured at n_new = 1e6, 32 windows (tools/model_effects_probe.py, profiles/model_effects_probe.json): effects alone
// 108.7 us (4.7 TB/s of its 512 MB; k_model_predict 83.5 us in the same run), with std 1.34 ms, 36 % of the fp64 vector
// peak: the quadratic form's arithmetic and LDS reads, not the streams, set the time.  The form that fetched S_cc by
// scalar loads from S's own rows (no LDS for S, eight windows per pass) took 1.92 ms against 1.39 ms with the same
// bits (profiles/model_effects_ab.txt) and was removed; 3 or 4 points per thread and 4 windows per pass were no faster.
constexpr int kMePts = 2;                  // points per thread with kStd: 2 x 33 features live in registers
constexpr int kMeBlk = kMvFeat * kMvFeat;  // a window's block of S as staged in LDS
constexpr int kMeGroup = 2;                // windows per pass with kStd: 2 x (4.1 + 8.7) KB

// quad[p] += phi_p^T B phi_p for a symmetric 33 x 33 block B in LDS (rows of 33, every lane reads the same entry: a
// broadcast), over its upper triangle row by row; each entry read serves the thread's kPts points
template <int kPts>
__device__ inline void effects_quad(const double* blk, const double (&phi)[kPts][kMvFeat], double (&quad)[kPts])
{
#pragma unroll
   for (int j = 0; j < kMvFeat; j++) {
      const double* row = blk + j * kMvFeat;
      double t[kPts];
#pragma unroll
      for (int p = 0; p < kPts; p++) t[p] = 0.0;
#pragma unroll
      for (int k = j + 1; k < kMvFeat; k++) {
         const double sjk = row[k];
#pragma unroll
         for (int p = 0; p < kPts; p++) t[p] = fma(sjk, phi[p][k], t[p]);
         // at most 8 entries of the block in flight: 164 VGPRs and 3 waves per SIMD; without it 172 and 2, 1.52 ms
         // against 1.32 ms (profiles/model_effects_ab.txt)
         if ((k - j) % 8 == 0) __builtin_amdgcn_sched_barrier(0);
      }
      const double sjj = row[j];
#pragma unroll
      for (int p = 0; p < kPts; p++) quad[p] = fma(phi[p][j], fma(sjj, phi[p][j], 2.0 * t[p]), quad[p]);
   }
}

template <bool kStd>
__global__ __launch_bounds__(kMpThreads) void k_model_effects(
   const double* __restrict__ H, const double* __restrict__ S, int Rp, const double* __restrict__ centre,
   const double* __restrict__ scale, const int* __restrict__ feature, int w0, int wn, const double* __restrict__ X,
   long long ldim, int n_new, double ff, double* __restrict__ effects, double* __restrict__ effect_std, long long lde,
   long long lds, unsigned int* __restrict__ cnt_out)
{
   constexpr int kPts = kStd ? kMePts : kMpPts;
   constexpr int kGroup = kStd ? kMeGroup : kMpGroup;
   __shared__ double s_H[kGroup * kMpWin];
   __shared__ double s_S[kStd ? kGroup * kMeBlk : 1];
   __shared__ unsigned int s_cnt[kMpThreads / kWave];
   const int tid = threadIdx.x;
   const long long base = (long long)blockIdx.x * (kMpThreads * kPts) + tid;
   bool outside[kPts];
#pragma unroll
   for (int p = 0; p < kPts; p++) outside[p] = false;
   for (int c0 = w0; c0 < w0 + wn; c0 += kGroup) {
      const int ng = min(kGroup, w0 + wn - c0);
      if (c0 != w0) __syncthreads();  // every thread has left the previous group's rows
      {
         const double2* src = reinterpret_cast<const double2*>(H + (size_t)c0 * kNos * kNC);
         const int pairs = ng * kNos * kNC / 2;
         for (int i = tid; i < pairs; i += kMpThreads) {
            const double2 v = src[i];
            const int e = 2 * i;  // element of [window][cell][degree]
            double* row = s_H + (e / (kNos * kNC)) * kMpWin + ((e / kNC) & (kNos - 1));
            const int dg = e & (kNC - 1);
            row[dg * kNos] = v.x;
            row[(dg + 1) * kNos] = v.y;
         }
      }
      if constexpr (kStd)
         for (int i = tid; i < ng * kMeBlk; i += kMpThreads) {
            const int cl = i / kMeBlk, e = i - cl * kMeBlk, j = e / kMvFeat, k = e - j * kMvFeat;
            s_S[i] = S[((size_t)(c0 + cl) * kMvPad + j) * Rp + (size_t)(c0 + cl) * kMvPad + k];
         }
      __syncthreads();
      for (int cl = 0; cl < ng; cl++) {
         const int c = c0 + cl;
         const double ctr = centre[c], sc = scale[c];
         const double* col = X + (size_t)feature[c] * (size_t)ldim;
         double xv[kPts];
         bool in[kPts];
#pragma unroll
         for (int p = 0; p < kPts; p++) {
            const long long i = base + (long long)p * kMpThreads;
            xv[p] = (i < n_new) ? col[i] : ctr;
         }
#pragma unroll
         for (int p = 0; p < kPts; p++) {
            const long long i = base + (long long)p * kMpThreads;
            const double xs = (xv[p] - ctr) * sc;         // subtract, then multiply: the setup's two roundings
            in[p] = fabs(xs) <= kMpLimit;                 // false for NaN and infinities too
            outside[p] = outside[p] || !in[p];
            const double xq = in[p] ? xs : 0.0;
            const uint32_t q = (uint32_t)(unsigned long long)llround(xq * 4294967296.0);  // quantize()
            const uint32_t cell = q >> 26;
            const double s = (double)(int)(((q & 0x3FFFFFFu) << 6) ^ 0x80000000u);  // slot_word, no index bits
            const double* hrow = s_H + cl * kMpWin + cell;
            double hc[kNC];
#pragma unroll
            for (int dg = 0; dg < kNC; dg++) hc[dg] = hrow[dg * kNos];
            double v = hc[kNC - 1];
#pragma unroll
            for (int dg = kNC - 2; dg >= 0; dg--) v = fma(v, s, hc[dg]);
            if (effects && i < n_new) effects[(size_t)(c - w0) * (size_t)lde + i] = in[p] ? ff * v : __builtin_nan("");
         }
         if constexpr (kStd) {
            double phi[kPts][kMvFeat], quad[kPts];
#pragma unroll
            for (int p = 0; p < kPts; p++) {
               double c1, s1;
               (void)mv_angle(xv[p], ctr, sc, c1, s1);
               double ck = 1.0, sk = 0.0;
#pragma unroll
               for (int k = 0; k <= 16; k++) {
                  phi[p][k] = ck;
                  if (k) phi[p][16 + k] = sk;
                  mv_rotate(ck, sk, c1, s1);
               }
               quad[p] = 0.0;
            }
            effects_quad<kPts>(s_S + cl * kMeBlk, phi, quad);
#pragma unroll
            for (int p = 0; p < kPts; p++) {  // (all of them before the first store)
               // the points' forms stay side by side, sharing each entry of the block: without this use the compiler
               // sinks each point's form into its own guarded store and keeps the whole block live across both
               asm volatile("" : "+v"(quad[p]));
            }
#pragma unroll
            for (int p = 0; p < kPts; p++) {
               const long long i = base + (long long)p * kMpThreads;
               if (i < n_new) effect_std[(size_t)(c - w0) * (size_t)lds + i] = in[p] ? sqrt(fabs(ff * quad[p])) : __builtin_nan("");
            }
         }
      }
   }
   if (cnt_out) {
      unsigned int cnt = 0;
#pragma unroll
      for (int p = 0; p < kPts; p++) {
         const long long i = base + (long long)p * kMpThreads;
         cnt += (unsigned int)__popcll(__ballot(i < n_new && outside[p]));
      }
      if ((tid & (kWave - 1)) == 0) s_cnt[tid / kWave] = cnt;
      __syncthreads();
      if (tid == 0) {
         unsigned int t = 0;
         for (int w = 0; w < kMpThreads / kWave; w++) t += s_cnt[w];
         cnt_out[blockIdx.x] = t;
      }
   }
}

int model_predict_effects(Model* M, const double* Xnew, int n_new, long long ldim, int w0, int wn, double* effects,
                          double* effect_std, long long ldo, long long* n_outside)
{
   hipStream_t s = current_stream();
   const size_t col = sizeof(double) * (size_t)n_new;
   double *xown = nullptr, *eown = nullptr, *sown = nullptr;
   auto body = [&]() -> int {
      const double* dX = Xnew;
      long long ld = ldim;
      if (!is_device_ptr(Xnew)) {  // only the columns the windows in range read
         NFFT4GP_HIP_CHECK(hipMalloc((void**)&xown, col * (size_t)M->d));
         for (int c = w0; c < w0 + wn; c++) {
            const size_t ft = (size_t)M->feature[c];
            NFFT4GP_HIP_CHECK(hipMemcpyAsync(xown + ft * (size_t)n_new, Xnew + ft * (size_t)ldim, col,
                                             hipMemcpyHostToDevice, s));
         }
         dX = xown;
         ld = n_new;
      }
      double *de = effects, *ds = effect_std;
      long long lde = ldo, lds = ldo;
      const bool ehost = effects && !is_device_ptr(effects), shost = effect_std && !is_device_ptr(effect_std);
      if (ehost) {
         NFFT4GP_HIP_CHECK(hipMalloc((void**)&eown, col * (size_t)wn));
         de = eown;
         lde = n_new;
      }
      if (shost) {
         NFFT4GP_HIP_CHECK(hipMalloc((void**)&sown, col * (size_t)wn));
         ds = sown;
         lds = n_new;
      }
      const int per = kMpThreads * (effect_std ? kMePts : kMpPts);
      const size_t nblk = ((size_t)n_new + per - 1) / per;
      if (n_outside && grow_counts(M, nblk)) return -1;
      unsigned int* cnt = n_outside ? M->d_cnt : (unsigned int*)nullptr;
      const dim3 grid((unsigned int)nblk), block(kMpThreads);
      auto* kern = effect_std ? k_model_effects<true> : k_model_effects<false>;
      hipLaunchKernelGGL(kern, grid, block, 0, s, (const double*)M->d_H, (const double*)M->d_S, mv_order(M->nw),
                         (const double*)M->d_centre, (const double*)M->d_scale, (const int*)M->d_feature, w0, wn, dX, ld,
                         n_new, M->f * M->f, de, ds, lde, lds, cnt);
      NFFT4GP_HIP_CHECK(hipGetLastError());
      if (ehost)
         NFFT4GP_HIP_CHECK(hipMemcpy2DAsync(effects, sizeof(double) * (size_t)ldo, eown, col, col, (size_t)wn,
                                            hipMemcpyDeviceToHost, s));
      if (shost)
         NFFT4GP_HIP_CHECK(hipMemcpy2DAsync(effect_std, sizeof(double) * (size_t)ldo, sown, col, col, (size_t)wn,
                                            hipMemcpyDeviceToHost, s));
      if (n_outside) {
         if (read_counts(M, nblk, s, n_outside)) return -1;
      } else if (xown || eown || sown) {
         NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
      }
      return 0;
   };
   const int rc = body();
   if (xown || eown || sown) (void)hipStreamSynchronize(s);
   for (double* p : {xown, eown, sown})
      if (p) (void)hipFree(p);
   return rc;
}

// ---- joint posterior sample paths ------------------------------------------------------------------------------------
// The posterior over functions is finite-rank: f(x) = mean(x) + f phi(x)^T theta, theta ~ N(0, S).  S is not always
// positive semidefinite (W has negative entries), so it is factored by a symmetric eigendecomposition and the negative
// part is dropped: S+ = V max(Lambda, 0) V^T = F F^T, F = V diag(sqrt max(lambda, 0)); defect = sum |lambda < 0| /
// sum |lambda| says how much went.  A set of paths is B = F xi for standard normal xi (R x ns, the caller's), kept in
// the model: the same B evaluated at any point set is the same ns functions.

// C[i + j R] = S[slot(i) R_p + slot(j)]: S without its padding (symmetric, so either triangle order)
__global__ void k_model_compact(const double* __restrict__ S, int Rp, int R, double* __restrict__ C)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
   if (i >= R) return;
   const int ip = i / kMvFeat * kMvPad + i % kMvFeat, jp = j / kMvFeat * kMvPad + j % kMvFeat;
   C[i + (size_t)j * R] = S[(size_t)ip * Rp + jp];
}

// Ft[k + jp R] = V[j + k R] sq[k] at the slot jp of feature j, zero at the padded slots (jp = blockIdx.y over R_p)
__global__ void k_model_factor(const double* __restrict__ V, const double* __restrict__ sq, int R, int nw,
                               double* __restrict__ Ft)
{
   const int k = blockIdx.x * blockDim.x + threadIdx.x, jp = blockIdx.y;
   if (k >= R) return;
   const int c = jp / kMvPad, r = jp % kMvPad;
   Ft[k + (size_t)jp * R] = (c < nw && r < kMvFeat) ? V[(c * kMvFeat + r) + (size_t)k * R] * sq[k] : 0.0;
}

// 0; -1
int model_fit_sampler(Model* M)
{
   hipStream_t s = current_stream();
   const int nw = M->nw, Rp = mv_order(nw), R = kMvFeat * nw;
   double *V = nullptr, *Ft = nullptr, *d_sq = nullptr;
   auto body = [&]() -> int {
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&V, sizeof(double) * (size_t)R * R));
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&Ft, sizeof(double) * (size_t)R * Rp));
      hipLaunchKernelGGL(k_model_compact, dim3((R + 255) / 256, R), dim3(256), 0, s, (const double*)M->d_S, Rp, R, V);
      NFFT4GP_HIP_CHECK(hipGetLastError());
      NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
      const auto t0 = std::chrono::steady_clock::now();
      std::vector<double> w;
      if (sym_eig_dev(V, R, w, s)) {
         fprintf(stderr, "nfft4gp_amd: Nfft4GPAmdModelFitSampler: the eigendecomposition of S failed.\n");
         return -1;
      }
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      double neg = 0.0, all = 0.0;
      std::vector<double> sq((size_t)R);
      for (int k = 0; k < R; k++) {  // ascending, a fixed order
         if (!std::isfinite(w[k])) return -1;
         if (w[k] < 0.0) neg += -w[k];
         all += std::fabs(w[k]);
         sq[k] = w[k] > 0.0 ? std::sqrt(w[k]) : 0.0;
      }
      if (to_device(&d_sq, sq.data(), sq.size())) return -1;
      hipLaunchKernelGGL(k_model_factor, dim3((R + 255) / 256, Rp), dim3(256), 0, s, (const double*)V,
                         (const double*)d_sq, R, nw, Ft);
      NFFT4GP_HIP_CHECK(hipGetLastError());
      NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
      model_drop_sampler(M);  // a refit starts again: the paths of the previous factor go
      std::swap(M->d_Ft, Ft);
      M->defect = all > 0.0 ? neg / all : 0.0;
      M->lam_min = w[0];
      M->lam_max = w[R - 1];
      M->sampler_ms = ms;
      return 0;
   };
   const int rc = body();
   (void)hipStreamSynchronize(s);
   for (double* p : {V, Ft, d_sq})
      if (p) (void)hipFree(p);
   return rc;
}

// The sample tile: the columns a workgroup of k_model_paths holds at once.  128 against 64, measured at n_new = 1e6 and
// 32 windows with the same bits (profiles/model_paths_ab.txt): 3.55 / 4.98 / 7.14 / 13.9 ms against 5.85 / 12.4 / 24.5 /
// 48.7 ms at ns = 16 / 64 / 128 / 256 (the narrower tile regenerates the features twice as often, and its instance
// took all 256 VGPRs and spilled); the 64-column instance was removed.
constexpr int kMqBlocks = 8, kMqCols = 16 * kMqBlocks;

// B^T = xi^T F^T (ns x R_p, leading dimension nsp = ns rounded up to the sample tile, the rows past ns zero) on
// gemm_f64: entry (s, slot) sums over k in gemm_f64's fixed order, whatever s and ns are.  0; -1
int model_draw_paths(Model* M, const double* xi, int ns, long long ldxi)
{
   hipStream_t s = current_stream();
   const int Rp = mv_order(M->nw), R = M->R;
   const int nsp = (ns + kMqCols - 1) / kMqCols * kMqCols;
   double *xown = nullptr, *Bt = nullptr;
   auto body = [&]() -> int {
      const double* dxi = xi;
      if (!is_device_ptr(xi)) {
         NFFT4GP_HIP_CHECK(hipMalloc((void**)&xown, sizeof(double) * (size_t)R * ns));
         NFFT4GP_HIP_CHECK(hipMemcpy2DAsync(xown, sizeof(double) * (size_t)R, xi, sizeof(double) * (size_t)ldxi,
                                            sizeof(double) * (size_t)R, (size_t)ns, hipMemcpyHostToDevice, s));
         dxi = xown;
         ldxi = R;
      }
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&Bt, sizeof(double) * (size_t)nsp * Rp));
      NFFT4GP_HIP_CHECK(hipMemsetAsync(Bt, 0, sizeof(double) * (size_t)nsp * Rp, s));
      if (gemm_f64(true, ns, Rp, R, dxi, ldxi, M->d_Ft, R, Bt, nsp, s)) return -1;
      NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
      std::swap(M->d_Bt, Bt);  // the previous paths are freed below
      M->ns = ns;
      M->nsp = nsp;
      return 0;
   };
   const int rc = body();
   (void)hipStreamSynchronize(s);
   for (double* p : {xown, Bt})
      if (p) (void)hipFree(p);
   return rc;
}

// k_model_paths: out[s ldo + i] = mean[i] + f sum_j phi_j(x_i) B[j, s] over the windows [w0, w0 + wn).
// quad_walk.hpp's organisation with B's rows in S's place: a workgroup owns 128 points and walks the samples in tiles
// of 16 NB columns; per tile, k steps of one window (36 slots): the features generated into LDS by quad_gen (mv_angle /
// mv_rotate: k_model_std's bits), 8 waves of 16 points x 16 NB columns on v_mfma_f64_16x16x4_f64 with the operands
// swapped as in k_gemm_f64 (a lane holds the columns lane / 16 + 4 reg of 16 consecutive points, so a store writes
// whole 128-byte segments of out's columns), and the next window's rows of B^T (global loads issued before the step's
// MFMAs) and features double-buffered behind them; one barrier per step.  Each window's 36 products start from a zero
// accumulator and the windows' sums are added in window order: the term of window c is the same bits alone (wn = 1)
// and inside the sum.  The 16-column blocks past ns are skipped (uniform over the workgroup).  Every further sample
// tile regenerates the features: one sincospi and 16 rotations per (point, window) against 36 x 16 NB FMAs.
// A (point, sample) value depends on neither the point's place in the batch, nor n_new, nor ns, nor the sample's
// column: the sums run over (window, slot) in a fixed order.  mean is NaN where the point is outside a window in
// range (k_model_predict / k_model_effects wrote it), and NaN + finite is NaN in every path; the features of such a
// point are those of the angle 0 (mv_angle).  No atomics.
// Measured at n_new = 1e6, 32 windows, with the mean's pass and the scratch allocation (tools/model_paths_probe.py,
// profiles/model_paths_probe.json): 3.56 / 3.57 / 5.01 / 13.97 ms at ns = 1 / 16 / 64 / 256 (54 % of the fp64 matrix
// peak at 256, counted at 2 n_new R_p ns flops; below 64 paths the feature generation sets the time) against 8.83 /
// 8.90 / 9.12 / 15.17 ms for the composed route (k_model_features, gemm_f64 and an add of the mean, in chunks), the two
// routes' values within 4.4e-15.
template <int NB>
__global__ __launch_bounds__(kMsThreads) void k_model_paths(const double* __restrict__ Bt, long long ldb, int ns,
                                                            const double* __restrict__ centre,
                                                            const double* __restrict__ scale,
                                                            const int* __restrict__ feature, int nw, int w0, int wn,
                                                            const double* __restrict__ X, long long ldim, int n_new,
                                                            double f, const double* __restrict__ mean,
                                                            double* __restrict__ out, long long ldo)
{
   constexpr int kCols = 16 * NB, kPairs = kCols / 2, kGroups = kMsThreads / kPairs;
   constexpr int kU = (kMvPad + kGroups - 1) / kGroups, kLdB = kCols + 1;
   static_assert(kLdB <= kMsLdB, "the rows of B^T take the place of quad_walk's rows of S");
   extern __shared__ double m_smem[];
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
   const int wm = wave * 16, lr = lane & 15, lg = lane >> 4;
   const int p = tid & (kMsPts - 1), part = tid >> 7;
   const int fcol = 2 * (tid % kPairs), frow = tid / kPairs;
   const long long ip = (long long)blockIdx.x * kMsPts + p;
   const QuadPoints Q{centre, scale, feature, nw, X, ldim, ip, ip < n_new};
   const long long io = (long long)blockIdx.x * kMsPts + wm + lr;  // the point of the lane's accumulators
   const bool olive = io < n_new;
   const double mu = olive ? mean[io] : 0.0;
   quad_zero_pad(m_smem);
   auto xload = [&](int c) { return Q.live ? X[(size_t)feature[c] * (size_t)ldim + ip] : centre[c]; };
   auto gen = [&](int c, double x, double* As) { quad_gen<0>(Q, c, x, p, part, As, nullptr, 0, nullptr); };
   double2 bv[kU];
   for (int t0 = 0; t0 < ns; t0 += kCols) {
      const int nb = min(NB, (ns - t0 + 15) / 16);  // the tile's blocks with a sample in them
      auto fetch = [&](int c) {  // slots 36 c .. 36 c + 35 of the tile's columns (ldb is a whole number of tiles)
         const double* Bc = Bt + (size_t)(c * kMvPad + frow) * ldb + t0 + fcol;
#pragma unroll
         for (int u = 0; u < kU; u++)
            if (frow + u * kGroups < kMvPad) bv[u] = *reinterpret_cast<const double2*>(Bc + (size_t)u * kGroups * ldb);
      };
      auto store = [&](double* Bs) {
#pragma unroll
         for (int u = 0; u < kU; u++)
            if (frow + u * kGroups < kMvPad) {
               Bs[(frow + u * kGroups) * kLdB + fcol] = bv[u].x;
               Bs[(frow + u * kGroups) * kLdB + fcol + 1] = bv[u].y;
            }
      };
      d4 sum[NB];
#pragma unroll
      for (int j = 0; j < NB; j++) sum[j] = d4{0.0, 0.0, 0.0, 0.0};
      __syncthreads();  // the previous tile's last step has left both buffers
      fetch(w0);
      gen(w0, xload(w0), m_smem);
      store(m_smem + kMvPad * kMsLdA);
      __syncthreads();
      int cur = 0;
      for (int c = w0; c < w0 + wn; c++) {
         const bool more = c + 1 < w0 + wn;
         double xn = 0.0;
         if (more) {
            fetch(c + 1);  // in flight during this step's MFMAs
            xn = xload(c + 1);
         }
         const double* As = m_smem + cur * kMsBuf;
         const double* Bs = As + kMvPad * kMsLdA;
         d4 acc[NB];
#pragma unroll
         for (int j = 0; j < NB; j++) acc[j] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 3
         for (int k4 = 0; k4 < kMvPad / 4; k4++) {
            const int kk = 4 * k4 + lg;
            const double a = As[kk * kMsLdA + wm + lr];
#pragma unroll
            for (int j = 0; j < NB; j++)
               if (j < nb) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(Bs[kk * kLdB + 16 * j + lr], a, acc[j], 0, 0, 0);
         }
#pragma unroll
         for (int j = 0; j < NB; j++) sum[j] += acc[j];
         if (more) {  // the other buffer: nobody reads it during this step
            gen(c + 1, xn, m_smem + (cur ^ 1) * kMsBuf);
            store(m_smem + (cur ^ 1) * kMsBuf + kMvPad * kMsLdA);
         }
         __syncthreads();
         cur ^= 1;
      }
      // sum[j][rg] = (Phi B)[point wm + lr][sample t0 + 16 j + lg + 4 rg]
#pragma unroll
      for (int j = 0; j < NB; j++)
#pragma unroll
         for (int rg = 0; rg < 4; rg++) {
            const int sc = t0 + 16 * j + lg + 4 * rg;
            if (olive && sc < ns) out[(size_t)sc * (size_t)ldo + io] = fma(f, sum[j][rg], mu);
         }
   }
}

template <int NB>
int launch_paths(const Model* M, int w0, int wn, const double* dX, long long ld, int n_new, const double* mean,
                 double* out, long long ldo, hipStream_t s)
{
   static const bool attr = []() {
      (void)hipFuncSetAttribute((const void*)k_model_paths<NB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMsLds);
      (void)hipGetLastError();
      return true;
   }();
   (void)attr;
   const size_t nblk = ((size_t)n_new + kMsPts - 1) / kMsPts;
   hipLaunchKernelGGL(k_model_paths<NB>, dim3((unsigned int)nblk), dim3(kMsThreads), kMsLds, s, (const double*)M->d_Bt,
                      (long long)M->nsp, M->ns, (const double*)M->d_centre, (const double*)M->d_scale,
                      (const int*)M->d_feature, M->nw, w0, wn, dX, ld, n_new, M->f, mean, out, ldo);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   return 0;
}

// The drawn paths at the rows of Xnew.  The mean (all windows: k_model_predict; one window: k_model_effects) goes to a
// scratch vector that k_model_paths' epilogue adds, with the outside count.  A host `out` is produced in chunks of
// points through a staging buffer of at most 64 MB; the bits do not depend on the chunking.
int model_eval_paths(Model* M, const double* Xnew, int n_new, long long ldim, int window, double* out, long long ldo,
                     long long* n_outside)
{
   hipStream_t s = current_stream();
   const int ns = M->ns;
   const bool odev = is_device_ptr(out);
   const int w0 = window < 0 ? 0 : window, wn = window < 0 ? M->nw : 1;
   double *xown = nullptr, *oown = nullptr, *mean = nullptr;
   auto body = [&]() -> int {
      const double* dX;
      long long ld;
      if (stage_points(M, Xnew, n_new, ldim, s, &dX, &ld, &xown)) return -1;
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&mean, sizeof(double) * (size_t)n_new));
      long long outside = 0;
      long long* pout = n_outside ? &outside : nullptr;
      if (window < 0) {
         if (model_predict(M, dX, n_new, ld, mean, pout)) return -1;
      } else if (model_predict_effects(M, dX, n_new, ld, w0, 1, mean, nullptr, n_new, pout)) {
         return -1;
      }
      int chunk = n_new;
      if (!odev) {
         const long long cap = std::max<long long>(kMsPts, (8LL << 20) / ns / kMsPts * kMsPts);
         chunk = (int)std::min<long long>(n_new, cap);
         NFFT4GP_HIP_CHECK(hipMalloc((void**)&oown, sizeof(double) * (size_t)chunk * ns));
      }
      for (long long i0 = 0; i0 < n_new; i0 += chunk) {
         const int cnt = (int)std::min<long long>(chunk, n_new - i0);
         if (launch_paths<kMqBlocks>(M, w0, wn, dX + i0, ld, cnt, mean + i0, odev ? out + i0 : oown,
                                     odev ? ldo : (long long)cnt, s))
            return -1;
         if (!odev) {  // (the next chunk's launch follows the copy on the stream)
            NFFT4GP_HIP_CHECK(hipMemcpy2DAsync(out + i0, sizeof(double) * (size_t)ldo, oown,
                                               sizeof(double) * (size_t)cnt, sizeof(double) * (size_t)cnt, (size_t)ns,
                                               hipMemcpyDeviceToHost, s));
            NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
         }
      }
      if (xown || !odev) NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
      if (n_outside) *n_outside = outside;
      return 0;
   };
   const int rc = body();
   (void)hipStreamSynchronize(s);  // the scratch mean is read by the launch in flight
   for (double* p : {xown, oown, mean})
      if (p) (void)hipFree(p);
   return rc;
}

// ---- the composed route, for tools/model_paths_probe.py's comparison only: a chunk of Z by k_model_features, Z B on
// gemm_f64, and the mean added by a third kernel ------------------------------------------------------------------------
__global__ void k_model_paths_transpose(const double* __restrict__ Bt, long long ldb, int ns, int Rp,
                                        double* __restrict__ B)
{
   const int j = blockIdx.x * blockDim.x + threadIdx.x, sc = blockIdx.y;
   if (j < Rp && sc < ns) B[j + (size_t)sc * Rp] = Bt[sc + (size_t)j * ldb];
}

__global__ void k_model_paths_finish(double* __restrict__ out, long long ldo, int cnt, const double* __restrict__ mean,
                                     double f)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i < cnt) {
      double* o = out + (size_t)blockIdx.y * (size_t)ldo + i;
      *o = fma(f, *o, mean[i]);
   }
}

int model_eval_paths_composed(Model* M, const double* dX, int n_new, long long ld, double* out, long long ldo)
{
   hipStream_t s = current_stream();
   const int ns = M->ns, Rp = mv_order(M->nw);
   double *Z = nullptr, *B = nullptr, *mean = nullptr;
   auto body = [&]() -> int {
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&mean, sizeof(double) * (size_t)n_new));
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&B, sizeof(double) * (size_t)Rp * ns));
      const int chunk = chunk_points(n_new, Rp);
      const long long ldz = ((long long)chunk + 15) / 16 * 16;
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&Z, sizeof(double) * (size_t)ldz * Rp));
      if (model_predict(M, dX, n_new, ld, mean, nullptr)) return -1;
      hipLaunchKernelGGL(k_model_paths_transpose, dim3((Rp + 255) / 256, ns), dim3(256), 0, s, (const double*)M->d_Bt,
                         (long long)M->nsp, ns, Rp, B);
      NFFT4GP_HIP_CHECK(hipGetLastError());
      for (long long i0 = 0; i0 < n_new; i0 += chunk) {
         const int cnt = (int)std::min<long long>(chunk, n_new - i0);
         hipLaunchKernelGGL(k_model_features, dim3((cnt + 255) / 256, Rp / kMvPad), dim3(256), 0, s,
                            (const double*)M->d_centre, (const double*)M->d_scale, (const int*)M->d_feature, M->nw, dX,
                            ld, i0, cnt, Z, ldz);
         NFFT4GP_HIP_CHECK(hipGetLastError());
         if (gemm_f64(false, cnt, ns, Rp, Z, ldz, B, Rp, out + i0, ldo, s)) return -1;
         hipLaunchKernelGGL(k_model_paths_finish, dim3((cnt + 255) / 256, ns), dim3(256), 0, s, out + i0, ldo, cnt,
                            (const double*)(mean + i0), M->f);
         NFFT4GP_HIP_CHECK(hipGetLastError());
      }
      return 0;
   };
   const int rc = body();
   (void)hipStreamSynchronize(s);
   for (double* p : {Z, B, mean})
      if (p) (void)hipFree(p);
   return rc;
}

}  // namespace
}  // namespace nfft4gp_amd

using namespace nfft4gp_amd;

extern "C" {

void* Nfft4GPAmdModelCreate(void* additive_handle, const double* alpha, int n)
{
   if (!device_ok()) {
      fprintf(stderr, "nfft4gp_amd: Nfft4GPAmdModelCreate: no HIP device visible.\n");
      return NULL;
   }
   AdditivePlan* Pp = additive_plan_of(additive_handle);
   if (!Pp || !alpha) {
      fprintf(stderr, "nfft4gp_amd: Nfft4GPAmdModelCreate needs an additive handle of this library (a distributed "
                      "operator has no table of its own) and alpha.\n");
      return NULL;
   }
   AdditivePlan& P = *Pp;
   const char* why = nullptr;
   if (!P.points_ready || !P.d_w || !P.d_H)
      why = "no Gaussian / Matern-1/2 setup call has been made on the handle";
   else if (P.row_begin != 0 || P.row_end != P.n_global)
      why = "the handle is a row shard";
   else if (P.diag != 1.0 || P.weight != 1.0 / (double)P.nw)
      why = "the handle is a component shard";
   else if (P.md.on || (int)P.comp_feature.size() != P.nw || (int)P.comp_centre.size() != P.nw)
      why = "every window must have exactly one feature";
   else if (n != P.n)
      why = "n is not the handle's number of points";
   if (!why)
      for (int c = 0; c < P.nw; c++)
         if (P.comp_dims[c] != 1 || P.comp_feature[c] < 0 || (P.d > 0 && P.comp_feature[c] >= P.d))
            why = "every window must have exactly one feature";
   if (why) {
      fprintf(stderr, "nfft4gp_amd: Nfft4GPAmdModelCreate: %s.\n", why);
      return NULL;
   }
   Model* M = new Model();
   M->nw = P.nw;
   M->d = P.d;
   M->kernel = P.kernel;
   M->f = P.f;
   M->l = P.l;
   M->mu = P.mu;
   M->centre = P.comp_centre;
   M->scale = P.comp_scale;
   M->feature = P.comp_feature;
   hipStream_t s = current_stream();
   double* d_a = nullptr;
   auto body = [&]() -> int {
      if (model_upload(M, nullptr)) return -1;
      const double* da = alpha;
      if (!is_device_ptr(alpha)) {
         NFFT4GP_HIP_CHECK(hipMalloc((void**)&d_a, sizeof(double) * (size_t)std::max(1, n)));
         NFFT4GP_HIP_CHECK(hipMemcpyAsync(d_a, alpha, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
         da = d_a;
      }
      // the matvec's own first two steps: d_H = the table for alpha (the interpolation step is the model's)
      if (launch_spread_grid(P, da, 0, s)) return -1;
      NFFT4GP_HIP_CHECK(hipMemcpyAsync(M->d_H, P.d_H, sizeof(double) * (size_t)P.nw * kNos * kNC,
                                       hipMemcpyDeviceToDevice, s));
      NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
      return 0;
   };
   const int rc = body();
   if (d_a) {
      (void)hipStreamSynchronize(s);
      (void)hipFree(d_a);
   }
   if (rc) {
      model_free(M);
      return NULL;
   }
   return M;
}

void* Nfft4GPAmdModelFromCoefficients(int nw, int d, int kernel, const double* hyper3, const double* H,
                                      const double* centre, const double* scale, const int* feature)
{
   if (!device_ok()) {
      fprintf(stderr, "nfft4gp_amd: Nfft4GPAmdModelFromCoefficients: no HIP device visible.\n");
      return NULL;
   }
   bool ok = nw >= 1 && d >= 1 && (kernel == 0 || kernel == 1) && hyper3 && H && centre && scale && feature;
   for (int c = 0; ok && c < nw; c++) ok = feature[c] >= 0 && feature[c] < d;
   if (!ok) {
      fprintf(stderr, "nfft4gp_amd: Nfft4GPAmdModelFromCoefficients: invalid arguments (nw >= 1, kernel 0 / 1, "
                      "features in [0, d)).\n");
      return NULL;
   }
   Model* M = new Model();
   M->nw = nw;
   M->d = d;
   M->kernel = kernel;
   M->f = hyper3[0];
   M->l = hyper3[1];
   M->mu = hyper3[2];
   M->centre.assign(centre, centre + nw);
   M->scale.assign(scale, scale + nw);
   M->feature.assign(feature, feature + nw);
   if (model_upload(M, H)) {
      model_free(M);
      return NULL;
   }
   return M;
}

int Nfft4GPAmdModelPredict(void* model, const double* Xnew, int n_new, int ldim, int d, double* mean,
                           long long* n_outside)
{
   Model* M = (Model*)model;
   if (!M || d != M->d || n_new < 0 || ldim < n_new) return -1;
   if (n_outside) *n_outside = 0;
   if (n_new == 0) return 0;
   if (!Xnew || !mean) return -1;
   return model_predict(M, Xnew, n_new, (long long)ldim, mean, n_outside);
}

int Nfft4GPAmdModelInfo(void* model, int* nw, int* d, int* kernel, double* hyper3)
{
   Model* M = (Model*)model;
   if (!M) return -1;
   if (nw) *nw = M->nw;
   if (d) *d = M->d;
   if (kernel) *kernel = M->kernel;
   if (hyper3) {
      hyper3[0] = M->f;
      hyper3[1] = M->l;
      hyper3[2] = M->mu;
   }
   return 0;
}

int Nfft4GPAmdModelCoefficients(void* model, double* H, double* centre, double* scale, int* feature)
{
   Model* M = (Model*)model;
   if (!M) return -1;
   if (H) NFFT4GP_HIP_CHECK(hipMemcpy(H, M->d_H, sizeof(double) * (size_t)M->nw * kNos * kNC, hipMemcpyDeviceToHost));
   for (int c = 0; c < M->nw; c++) {
      if (centre) centre[c] = M->centre[c];
      if (scale) scale[c] = M->scale[c];
      if (feature) feature[c] = M->feature[c];
   }
   return 0;
}

int Nfft4GPAmdModelFeatureWeights(int kernel, double l, double scale, int nw, double* w33)
{
   if ((kernel != 0 && kernel != 1) || !(l > 0.0) || !(scale > 0.0) || nw < 1 || !w33) return -1;
   feature_weights(kernel, l, scale, nw, w33);
   return 0;
}

static bool variance_fits(const Model* M, const char* who)
{
   if (M->nw <= kMvMaxNw) return true;
   fprintf(stderr, "nfft4gp_amd: %s: the variance matrix of %d windows would take %.0f MB; the limit is %d windows "
                   "(170 MB).\n", who, M->nw, 8e-6 * kMvPad * kMvPad * (double)M->nw * M->nw, kMvMaxNw);
   return false;
}

int Nfft4GPAmdModelFitVariance(void* model, const double* X, int n, int ldim, int d)
{
   Model* M = (Model*)model;
   if (!M || !X || d != M->d || n < 1 || ldim < n) return -1;
   if (!variance_fits(M, "Nfft4GPAmdModelFitVariance")) return -1;
   return model_fit_variance(M, X, n, (long long)ldim);
}

int Nfft4GPAmdModelPredictStd(void* model, const double* Xnew, int n_new, int ldim, int d, double* std_out,
                              int with_noise, long long* n_outside)
{
   Model* M = (Model*)model;
   if (!M || d != M->d || n_new < 0 || ldim < n_new) return -1;
   if (!M->d_S) return -3;
   if (n_outside) *n_outside = 0;
   if (n_new == 0) return 0;
   if (!Xnew || !std_out) return -1;
   return model_predict_std(M, Xnew, n_new, (long long)ldim, std_out, with_noise, n_outside);
}

int Nfft4GPAmdModelPredictEffects(void* model, const double* Xnew, int n_new, int ldim, int d, int w0, int wn,
                                  double* effects, double* effect_std, int ldo, long long* n_outside)
{
   Model* M = (Model*)model;
   if (!M || d != M->d || n_new < 0 || ldim < n_new || ldo < n_new) return -1;
   if (w0 < 0 || wn < 1 || (long long)w0 + wn > M->nw || (n_new > 0 && !Xnew)) return -1;
   if (effect_std && !M->d_S) return -3;
   if (n_outside) *n_outside = 0;
   if (n_new == 0) return 0;
   return model_predict_effects(M, Xnew, n_new, (long long)ldim, w0, wn, effects, effect_std, (long long)ldo,
                                n_outside);
}

int Nfft4GPAmdModelVarianceInfo(void* model, int* R)
{
   Model* M = (Model*)model;
   if (!M) return -1;
   if (R) *R = M->R;
   return 0;
}

int Nfft4GPAmdModelFitTimes(void* model, double* ms3)
{
   Model* M = (Model*)model;
   if (!M || !ms3) return -1;
   for (int i = 0; i < 3; i++) ms3[i] = M->fit_ms[i];
   return 0;
}

int Nfft4GPAmdModelVariance(void* model, double* S)
{
   Model* M = (Model*)model;
   if (!M || !S) return -1;
   if (!M->d_S) return -3;
   const int Rp = mv_order(M->nw), R = M->R;
   std::vector<double> h((size_t)Rp * Rp);
   NFFT4GP_HIP_CHECK(hipMemcpy(h.data(), M->d_S, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
   for (int i = 0; i < R; i++)
      for (int j = 0; j < R; j++)
         S[(size_t)i * R + j] = h[(size_t)(i / kMvFeat * kMvPad + i % kMvFeat) * Rp + j / kMvFeat * kMvPad + j % kMvFeat];
   return 0;
}

int Nfft4GPAmdModelSetVariance(void* model, const double* S, int R)
{
   Model* M = (Model*)model;
   if (!M || !S || R != kMvFeat * M->nw) return -1;
   if (!variance_fits(M, "Nfft4GPAmdModelSetVariance")) return -1;
   const int Rp = mv_order(M->nw);
   std::vector<double> h((size_t)Rp * Rp, 0.0);
   for (int i = 0; i < R; i++)
      for (int j = 0; j < R; j++)
         h[(size_t)(i / kMvFeat * kMvPad + i % kMvFeat) * Rp + j / kMvFeat * kMvPad + j % kMvFeat] = S[(size_t)i * R + j];
   double* dS = nullptr;
   if (to_device(&dS, h.data(), h.size())) {
      if (dS) (void)hipFree(dS);
      return -1;
   }
   if (M->d_S) (void)hipFree(M->d_S);
   M->d_S = dS;
   M->R = R;
   model_drop_sampler(M);
   return 0;
}

int Nfft4GPAmdModelFitSampler(void* model, double* info3)
{
   Model* M = (Model*)model;
   if (!M) return -1;
   if (!M->d_S) return -3;
   if (model_fit_sampler(M)) return -1;
   if (info3) {
      info3[0] = M->defect;
      info3[1] = M->lam_min;
      info3[2] = M->lam_max;
   }
   return 0;
}

int Nfft4GPAmdModelSamplerFitTime(void* model, double* ms)
{
   Model* M = (Model*)model;
   if (!M || !ms) return -1;
   if (!M->d_Ft) return -4;
   *ms = M->sampler_ms;
   return 0;
}

int Nfft4GPAmdModelSamplerFactor(void* model, double* F)
{
   Model* M = (Model*)model;
   if (!M || !F) return -1;
   if (!M->d_S) return -3;
   if (!M->d_Ft) return -4;
   const int Rp = mv_order(M->nw), R = M->R;
   std::vector<double> h((size_t)R * Rp);
   NFFT4GP_HIP_CHECK(hipMemcpy(h.data(), M->d_Ft, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
   for (int i = 0; i < R; i++) {
      const double* row = h.data() + (size_t)(i / kMvFeat * kMvPad + i % kMvFeat) * R;
      for (int k = 0; k < R; k++) F[(size_t)i * R + k] = row[k];
   }
   return 0;
}

int Nfft4GPAmdModelDrawPaths(void* model, const double* xi, int ns, int ldxi)
{
   Model* M = (Model*)model;
   if (!M) return -1;
   if (!M->d_S) return -3;
   if (!M->d_Ft) return -4;
   if (!xi || ns < 1 || ldxi < M->R) return -1;
   return model_draw_paths(M, xi, ns, (long long)ldxi);
}

int Nfft4GPAmdModelPathsInfo(void* model, int* ns)
{
   Model* M = (Model*)model;
   if (!M) return -1;
   if (ns) *ns = M->d_Bt ? M->ns : 0;
   return 0;
}

int Nfft4GPAmdModelPathWeights(void* model, double* B)
{
   Model* M = (Model*)model;
   if (!M || !B) return -1;
   if (!M->d_Bt) return -4;
   const int Rp = mv_order(M->nw), R = M->R, ns = M->ns, nsp = M->nsp;
   std::vector<double> h((size_t)nsp * Rp);
   NFFT4GP_HIP_CHECK(hipMemcpy(h.data(), M->d_Bt, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
   for (int sc = 0; sc < ns; sc++)
      for (int i = 0; i < R; i++)
         B[i + (size_t)sc * R] = h[sc + (size_t)(i / kMvFeat * kMvPad + i % kMvFeat) * nsp];
   return 0;
}

int Nfft4GPAmdModelEvalPaths(void* model, const double* Xnew, int n_new, int ldim, int d, int window, double* out,
                             int ldo, long long* n_outside)
{
   Model* M = (Model*)model;
   if (!M || d != M->d || n_new < 0 || ldim < n_new || ldo < n_new || window < -1 || window >= M->nw) return -1;
   if (n_new > 0 && (!Xnew || !out)) return -1;
   if (!M->d_Bt) return -4;
   if (n_outside) *n_outside = 0;
   if (n_new == 0) return 0;
   return model_eval_paths(M, Xnew, n_new, (long long)ldim, window, out, (long long)ldo, n_outside);
}

int Nfft4GPAmdDebugModelPaths(void* model, const double* Xnew, int n_new, int ldim, int route, double* out, int ldo)
{
   Model* M = (Model*)model;
   if (!M || !Xnew || !out || n_new < 1 || ldim < n_new || ldo < n_new || route != 0) return -1;
   if (!M->d_Bt) return -4;
   if (!is_device_ptr(Xnew) || !is_device_ptr(out)) return -1;
   return model_eval_paths_composed(M, Xnew, n_new, (long long)ldim, out, (long long)ldo);
}

void Nfft4GPAmdModelFree(void* model) { model_free((Model*)model); }

}  // extern "C"
