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
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "internal.h"

namespace nfft4gp_amd {
namespace {

constexpr int kMpThreads = 256;
constexpr int kMpPts = 4;                  // points per thread (strided by the workgroup: coalesced columns)
constexpr int kMpGroup = 8;                // windows staged in LDS per pass (8 x 513 doubles = 32.8 KB)
constexpr int kMpWin = kNC * kNos + 1;     // [window][degree][cell], windows 513 doubles apart (k_interp_hl)
constexpr double kMpLimit = 0.25 + 1.0 / 8589934592.0;  // 1/4 + 2^-33

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
};

void model_free(Model* M)
{
   if (!M) return;
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

void Nfft4GPAmdModelFree(void* model) { model_free((Model*)model); }

}  // extern "C"
