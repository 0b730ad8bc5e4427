// window_moments.hip -- the moments of the operator's finite-rank form with 1-D windows (internal.h's section; DESIGN
// 3.16, 3.17): G = Z^T Z, Z^T y and y^T y over a point set, the windows' weights W, and the count of rows outside the
// domain.  The variance fit of the model (model_variance.hip) and the feature-space GP (feature_gp.hip) both start from
// these.  The host helpers that every driver of this family uses (stage, BlockCounts) are defined here too.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <vector>

#include "window_points.hpp"

namespace nfft4gp_amd {
namespace {

// per workgroup the number of rows with a coordinate outside some window's domain
__global__ __launch_bounds__(256) void k_model_outside(const double* __restrict__ centre,
                                                       const double* __restrict__ scale,
                                                       const int* __restrict__ feature, int nw,
                                                       const double* __restrict__ X, long long ldim, int n,
                                                       unsigned int* __restrict__ cnt_out)
{
   const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
   const bool out[1] = {i < n && row_outside(centre, scale, feature, nw, X, ldim, i)};
   block_count_outside<256>(out, cnt_out);
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
   (void)mv_features(X[(size_t)feature[c] * (size_t)ldim + i0 + i], centre[c], scale[c],
                     [&](int j, double v) { z[j * ldz] = v; });
   for (int j = kMvFeat; j < kMvPad; j++) z[j * ldz] = 0.0;
}

// Z^T y and y^T y without Z: part[block][slot] = the block's sum of feature(slot) y over its points, slot R_p the
// block's sum of y^2.  A thread owns kZyPts points (strided by the workgroup) and regenerates their features window
// by window as k_model_features does (the same bits); each of a window's 33 sums folds over the wave in a fixed
// butterfly, then over the 4 waves in wave order.  k_model_sum_parts adds the blocks in block order: no atomics, the
// same bits every time.
constexpr int kZyThreads = 256, kZyPts = 4;

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
   BlockCounts counts;
   if (counts.grow(nblk)) return -1;
   hipLaunchKernelGGL(k_model_outside, dim3((unsigned int)nblk), dim3(256), 0, s, W.centre, W.scale, W.feature, W.nw,
                      dX, ld, n, counts.d);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   return counts.read(nblk, s, outside);
}

int stage(Scratch& sc, const double* src, size_t rows, size_t cols, size_t ld, const double** dev, long long* dld)
{
   *dev = src;
   *dld = (long long)ld;
   if (is_device_ptr(src)) return 0;
   double* packed;
   if (sc.alloc(&packed, std::max<size_t>(1, rows * cols))) return -1;
   NFFT4GP_HIP_CHECK(hipMemcpy2DAsync(packed, sizeof(double) * rows, src, sizeof(double) * ld, sizeof(double) * rows,
                                      cols, hipMemcpyHostToDevice, sc.s));
   *dev = packed;
   *dld = (long long)rows;
   return 0;
}

int BlockCounts::grow(size_t nblk)
{
   if (nblk <= cap) return 0;
   if (d) (void)hipFree(d);
   d = nullptr;
   cap = 0;
   NFFT4GP_HIP_CHECK(hipMalloc((void**)&d, sizeof(unsigned int) * nblk));
   cap = nblk;
   return 0;
}

int BlockCounts::read(size_t nblk, hipStream_t s, long long* total)
{
   std::vector<unsigned int> h(nblk);
   NFFT4GP_HIP_CHECK(hipMemcpyAsync(h.data(), d, sizeof(unsigned int) * nblk, hipMemcpyDeviceToHost, s));
   NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
   long long t = 0;
   for (unsigned int v : h) t += v;
   *total = t;
   return 0;
}

// Z in chunks -> their Grams (gram_tn: split sum in a fixed order) added in chunk order; Z^T y and y^T y by
// k_model_zty (b and yy must be contiguous: b + R_p == yy)
int window_moments(const WindowMap& W, const double* dX, long long ld, int n, const double* dy, double* G, double* b,
                   double* yy, double* ms2, hipStream_t s)
{
   const int Rp = mv_order(W.nw);
   const size_t rr = (size_t)Rp * Rp;
   Scratch sc(s);
   double *Z, *Gc, *part;
   if (dy) {
      if (yy != b + Rp) return -1;
      const int per = kZyThreads * kZyPts;
      const int nblk = (int)(((long long)n + per - 1) / per);
      if (sc.alloc(&part, (size_t)nblk * (Rp + 1))) return -1;
      hipLaunchKernelGGL(k_model_zty, dim3(nblk), dim3(kZyThreads), 0, s, W.centre, W.scale, W.feature, W.nw, dX, ld, n,
                         dy, Rp, part);
      if (sum_parts_dev(part, nblk, Rp + 1, b, s)) return -1;
      if (!G) return sc.finish();
   }
   const int chunk = chunk_points(n, Rp);
   const long long ldz = ((long long)chunk + 15) / 16 * 16;
   if (sc.alloc(&Z, (size_t)ldz * Rp) || sc.alloc(&Gc, rr)) return -1;
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
      hipLaunchKernelGGL(k_model_add, dim3((unsigned int)((rr + 255) / 256)), dim3(256), 0, s, G, (const double*)Gc,
                         (long long)rr);
      NFFT4GP_HIP_CHECK(hipGetLastError());
   }
   NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
   lap(1);
   if (ms2) ms2[0] = ms[0], ms2[1] = ms[1];
   return 0;
}

}  // namespace nfft4gp_amd

using namespace nfft4gp_amd;

extern "C" {

int Nfft4GPAmdModelFeatureWeights(int kernel, double l, double scale, int nw, double* w33)
{
   if ((kernel != 0 && kernel != 1) || !(l > 0.0) || !(scale > 0.0) || nw < 1 || !w33) return -1;
   feature_weights(kernel, l, scale, nw, w33);
   return 0;
}

int Nfft4GPAmdModelFeatureWeightsGrad(int kernel, double l, double scale, int nw, double* dw33)
{
   if ((kernel != 0 && kernel != 1) || !(l > 0.0) || !(scale > 0.0) || nw < 1 || !dw33) return -1;
   feature_weights_grad(kernel, l, scale, nw, dw33);
   return 0;
}

}  // extern "C"
