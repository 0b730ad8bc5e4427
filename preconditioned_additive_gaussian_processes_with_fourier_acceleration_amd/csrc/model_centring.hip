// model_centring.hip -- the fitted model's effects centred on a reference sample, and its intercept.
//
// Every window's term carries 1/nw of the constant and the data identify only the constant's sum, so a window's raw
// std is mostly the uncertainty of a constant (model.hip, the effects' section).  Over a reference sample X_ref of n
// rows -- the training points -- the model keeps
//   m     = Z^T 1 / n, the features' means (33 nw; the constant slot of every window is n / n = 1 exactly),
//   e_c   = (1/n) sum_i e_ic and sd_c = sqrt((1/n) sum_i (e_ic - e_c)^2), e_ic = ff Horner(H_c) the value
//           k_model_effects stores for (point i, window c),
// after which k_model_effects<., true> serves e_c(x) - e_c and sqrt|f^2 (phi_c - m_c)^T S_cc (phi_c - m_c)|, and the
// intercept is b = sum_c e_c with std sqrt|f^2 m^T S m|.  The centring belongs to the table and the sample, not to S: a
// new variance keeps it.  m comes from window_moments (Z^T y with y = 1: k_model_zty's bits); the effects' moments are
// k_model_effect_moments' two passes.  No atomics anywhere: two fits give the same bits.
#include <cmath>
#include <cstdio>
#include <vector>

#include "model.hpp"
#include "window_points.hpp"

namespace nfft4gp_amd {

void model_drop_centring(Model* M)
{
   if (M->d_fmean) (void)hipFree(M->d_fmean);
   if (M->d_emean) (void)hipFree(M->d_emean);
   M->d_fmean = M->d_emean = nullptr;
   M->emean.clear();
   M->esd.clear();
   M->n_ref = 0;
}

namespace {

constexpr int kCmPts = 4;    // points per thread, as k_model_predict
constexpr int kCmGroup = 8;  // windows staged in LDS per pass, as k_model_predict
constexpr int kCmWaves = kMpThreads / kWave;

__global__ void k_centring_fill(double* __restrict__ v, int n, double a)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i < n) v[i] = a;
}

// m[i] = b[i] / n (a division: the constant slots are n / n = 1 exactly)
__global__ void k_centring_divide(const double* __restrict__ b, int count, double n, double* __restrict__ m)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i < count) m[i] = b[i] / n;
}

// The reference sample's pass over the table: part[block][c] = the workgroup's sum over its points of e_ic (emean
// NULL: the first pass) or of (e_ic - emean[c])^2 (the second), e_ic = ff * v rounded as k_model_effects stores it.
// k_model_predict's walk: the group's tables staged in LDS, one coalesced coordinate load per (point, window), the same
// table_stage and table_eval.  Per window a thread adds its kCmPts points in order, the wave folds in zy_wave_sum's
// butterfly, the waves are added in wave order and k_model_sum_parts adds the workgroups in block order.  Two passes
// and not sum e^2 - n e_c^2: each window carries the constant, so |e_c| can be far above the spread and the one-pass
// form cancels.  A point past the end adds an exact zero; rows outside the domain have been refused by the caller.
// Measured (tools/model_centring_probe.py, profiles/model_centring_probe.json): the whole fit -- the outside count,
// Z^T 1, both passes and their host round trips -- over n = 1e6 device points at 32 windows takes 2.25 ms.
template <bool kSpread>
__global__ __launch_bounds__(kMpThreads) void k_model_effect_moments(
   const double* __restrict__ H, const double* __restrict__ centre, const double* __restrict__ scale,
   const int* __restrict__ feature, int nw, const double* __restrict__ X, long long ldim, int n, double ff,
   const double* __restrict__ emean, double* __restrict__ part)
{
   __shared__ double s_H[kCmGroup * kMpWin];
   __shared__ double s_w[kCmWaves][kCmGroup];
   const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
   const long long base = (long long)blockIdx.x * (kMpThreads * kCmPts) + tid;
   double* out = part + (size_t)blockIdx.x * nw;
   for (int c0 = 0; c0 < nw; c0 += kCmGroup) {
      const int ng = min(kCmGroup, nw - c0);
      if (c0) __syncthreads();  // every thread has left the previous group's rows and its sums have been read
      table_stage(H + (size_t)c0 * kNos * kNC, ng, s_H);
      __syncthreads();
      for (int cl = 0; cl < ng; cl++) {
         const int c = c0 + cl;
         const double ctr = centre[c], sc = scale[c];
         const double* col = X + (size_t)feature[c] * (size_t)ldim;
         double em = 0.0;
         if constexpr (kSpread) em = emean[c];
         double xv[kCmPts];
#pragma unroll
         for (int p = 0; p < kCmPts; p++) {
            const long long i = base + (long long)p * kMpThreads;
            xv[p] = (i < n) ? col[i] : ctr;
         }
         double acc = 0.0;
#pragma unroll
         for (int p = 0; p < kCmPts; p++) {
            const bool live = base + (long long)p * kMpThreads < n;
            bool in;
            double e = ff * table_eval(s_H + cl * kMpWin, (xv[p] - ctr) * sc, in);
            asm volatile("" : "+v"(e));  // the stored effect: the product rounded, not contracted into what follows
            if constexpr (kSpread) {
               const double dv = e - em;
               acc = live ? fma(dv, dv, acc) : acc;
            } else {
               acc += live ? e : 0.0;
            }
         }
         acc = zy_wave_sum(acc);
         if (lane == 0) s_w[wave][cl] = acc;
      }
      __syncthreads();
      if (tid < ng) {
         double v = s_w[0][tid];
#pragma unroll
         for (int w = 1; w < kCmWaves; w++) v += s_w[w][tid];
         out[c0 + tid] = v;
      }
   }
}

// part[block] = the workgroup's sum over its rows i of m_i (S m)_i, S the padded symmetric matrix (column-major, so a
// wave reads a column's consecutive rows) and m in its slot layout: row i's dot product runs over the columns in
// order, the rows fold as in k_model_effect_moments.  m^T S m once per call: R_p^2 multiply-adds.
__global__ __launch_bounds__(kMpThreads) void k_model_intercept_parts(const double* __restrict__ S, int Rp,
                                                                      const double* __restrict__ m,
                                                                      double* __restrict__ part)
{
   __shared__ double s_w[kCmWaves];
   const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
   const int i = blockIdx.x * kMpThreads + tid;
   double t = 0.0;
   if (i < Rp) {
      for (int j = 0; j < Rp; j++) t = fma(S[(size_t)j * Rp + i], m[j], t);
      t *= m[i];
   }
   t = zy_wave_sum(t);
   if (lane == 0) s_w[wave] = t;
   __syncthreads();
   if (tid == 0) {
      double v = s_w[0];
#pragma unroll
      for (int w = 1; w < kCmWaves; w++) v += s_w[w];
      part[blockIdx.x] = v;
   }
}

// The fit: the outside count -> m = Z^T 1 / n (window_moments) -> the effects' means -> their spreads.  The model takes
// the new centring only when every step has succeeded.  Returns 0, -1, or -2 (rows outside).
int model_fit_centring(Model* M, const double* X, int n, long long ldim)
{
   hipStream_t s = current_stream();
   const int nw = M->nw, Rp = mv_order(nw);
   Scratch sc(s);
   const double* dX;
   long long ld;
   if (stage(sc, X, (size_t)n, (size_t)M->d, (size_t)ldim, &dX, &ld)) return -1;
   const WindowMap W = window_map(M);
   long long outside = 0;
   if (window_count_outside(W, dX, ld, n, s, &outside)) return -1;
   if (outside) {
      fprintf(stderr, "nfft4gp_amd: Nfft4GPAmdModelFitCentring: %lld of %d rows lie outside the model's domain; "
                      "the model is unchanged.\n", outside, n);
      return -2;
   }
   double *ones, *b, *fm, *em, *part, *sums;
   if (sc.alloc(&ones, (size_t)n) || sc.alloc(&b, (size_t)Rp + 1) || sc.alloc(&fm, (size_t)Rp) ||
       sc.alloc(&em, (size_t)nw))
      return -1;
   hipLaunchKernelGGL(k_centring_fill, dim3((n + 255) / 256), dim3(256), 0, s, ones, n, 1.0);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   if (window_moments(W, dX, ld, n, ones, nullptr, b, b + Rp, nullptr, s)) return -1;
   hipLaunchKernelGGL(k_centring_divide, dim3((Rp + 255) / 256), dim3(256), 0, s, (const double*)b, Rp, (double)n, fm);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   const int per = kMpThreads * kCmPts;
   const int nblk = (int)(((long long)n + per - 1) / per);
   if (sc.alloc(&part, (size_t)nblk * nw) || sc.alloc(&sums, (size_t)nw)) return -1;
   const double ff = M->f * M->f;
   std::vector<double> emean((size_t)nw), esd((size_t)nw);
   for (int pass = 0; pass < 2; pass++) {
      auto* kern = pass ? k_model_effect_moments<true> : k_model_effect_moments<false>;
      hipLaunchKernelGGL(kern, dim3(nblk), dim3(kMpThreads), 0, s, (const double*)M->d_H, W.centre, W.scale, W.feature,
                         nw, dX, ld, n, ff, (const double*)em, part);
      NFFT4GP_HIP_CHECK(hipGetLastError());
      if (sum_parts_dev(part, nblk, nw, sums, s)) return -1;
      std::vector<double>& h = pass ? esd : emean;
      NFFT4GP_HIP_CHECK(hipMemcpyAsync(h.data(), sums, sizeof(double) * nw, hipMemcpyDeviceToHost, s));
      NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
      for (int c = 0; c < nw; c++) h[c] = pass ? std::sqrt(h[c] / (double)n) : h[c] / (double)n;
      if (!pass) NFFT4GP_HIP_CHECK(hipMemcpy(em, h.data(), sizeof(double) * nw, hipMemcpyHostToDevice));
   }
   sc.trade(&M->d_fmean, fm);  // the previous centring, if any, goes with the call
   sc.trade(&M->d_emean, em);
   M->emean.swap(emean);
   M->esd.swap(esd);
   M->n_ref = n;
   return 0;
}

// *q = m^T S m
int model_intercept_form(Model* M, double* q)
{
   hipStream_t s = current_stream();
   const int Rp = mv_order(M->nw), nblk = (Rp + kMpThreads - 1) / kMpThreads;
   Scratch sc(s);
   double* part;
   if (sc.alloc(&part, (size_t)nblk + 1)) return -1;
   hipLaunchKernelGGL(k_model_intercept_parts, dim3(nblk), dim3(kMpThreads), 0, s, (const double*)M->d_S, Rp,
                      (const double*)M->d_fmean, part);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   if (sum_parts_dev(part, nblk, 1, part + nblk, s)) return -1;
   NFFT4GP_HIP_CHECK(hipMemcpyAsync(q, part + nblk, sizeof(double), hipMemcpyDeviceToHost, s));
   return sc.finish();
}

}  // namespace
}  // namespace nfft4gp_amd

using namespace nfft4gp_amd;

extern "C" {

int Nfft4GPAmdModelFitCentring(void* model, const double* X, int n, int ldim, int d)
{
   Model* M = (Model*)model;
   if (!M || !X || d != M->d || n < 1 || ldim < n) return -1;
   return model_fit_centring(M, X, n, (long long)ldim);
}

int Nfft4GPAmdModelCentring(void* model, int* n_ref, double* feature_mean, double* effect_mean, double* effect_sd)
{
   Model* M = (Model*)model;
   if (!M) return -1;
   if (!M->n_ref) return -5;
   if (feature_mean) {
      std::vector<double> h((size_t)mv_order(M->nw));
      NFFT4GP_HIP_CHECK(hipMemcpy(h.data(), M->d_fmean, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
      for (int i = 0; i < kMvFeat * M->nw; i++) feature_mean[i] = h[(size_t)mv_slot(i)];
   }
   if (n_ref) *n_ref = M->n_ref;
   for (int c = 0; c < M->nw; c++) {
      if (effect_mean) effect_mean[c] = M->emean[c];
      if (effect_sd) effect_sd[c] = M->esd[c];
   }
   return 0;
}

int Nfft4GPAmdModelSetCentring(void* model, int n_ref, const double* feature_mean, const double* effect_mean,
                               const double* effect_sd, int nw)
{
   Model* M = (Model*)model;
   if (!M || n_ref < 1 || !feature_mean || !effect_mean || !effect_sd || nw != M->nw) return -1;
   for (int c = 0; c < nw; c++)
      if (feature_mean[(size_t)kMvFeat * c] != 1.0) return -1;  // the constant's mean is exact, or it is no mean
   std::vector<double> h((size_t)mv_order(nw), 0.0);
   for (int i = 0; i < kMvFeat * nw; i++) h[(size_t)mv_slot(i)] = feature_mean[i];
   double *fm = nullptr, *em = nullptr;
   if (to_device(&fm, h.data(), h.size()) || to_device(&em, effect_mean, (size_t)nw)) {
      if (fm) (void)hipFree(fm);
      if (em) (void)hipFree(em);
      return -1;
   }
   model_drop_centring(M);
   M->d_fmean = fm;
   M->d_emean = em;
   M->emean.assign(effect_mean, effect_mean + nw);
   M->esd.assign(effect_sd, effect_sd + nw);
   M->n_ref = n_ref;
   return 0;
}

int Nfft4GPAmdModelPredictEffectsCentred(void* model, const double* Xnew, int n_new, int ldim, int d, int w0, int wn,
                                         double* effects, double* effect_std, int ldo, long long* n_outside)
{
   Model* M = (Model*)model;
   if (!M || d != M->d || n_new < 0 || ldim < n_new || ldo < n_new) return -1;
   if (w0 < 0 || wn < 1 || (long long)w0 + wn > M->nw || (n_new > 0 && !Xnew)) return -1;
   if (!M->n_ref) return -5;
   if (effect_std && !M->d_S) return -3;
   if (n_outside) *n_outside = 0;
   if (n_new == 0) return 0;
   return model_predict_effects(M, Xnew, n_new, (long long)ldim, w0, wn, effects, effect_std, (long long)ldo,
                                n_outside, true);
}

int Nfft4GPAmdModelIntercept(void* model, double* value, double* std_out)
{
   Model* M = (Model*)model;
   if (!M) return -1;
   if (!M->n_ref) return -5;
   if (std_out && !M->d_S) return -3;
   double q = 0.0;
   if (std_out && model_intercept_form(M, &q)) return -1;
   if (value) {
      double b = 0.0;
      for (int c = 0; c < M->nw; c++) b += M->emean[c];
      *value = b;
   }
   if (std_out) *std_out = std::sqrt(std::fabs(M->f * M->f * q));
   return 0;
}

}  // extern "C"
