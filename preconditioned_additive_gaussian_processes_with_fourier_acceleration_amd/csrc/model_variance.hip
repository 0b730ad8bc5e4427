// model_variance.hip -- the fitted model's predictive standard deviation without the training data.
//
// With 1-D windows the operator is a finite-rank kernel, A = f^2 (Z W Z^T + mu I): Z holds per window the 33
// features [cos 2 pi k xs, k = 0..16 | sin 2 pi k xs, k = 1..16] of the window's scaled coordinate and W is
// diagonal (feature_weights).  The posterior variance at a point with features phi is f^2 (mu + phi^T S phi) with
// S = mu (mu I + W G)^{-1} W, G = Z^T Z over the training points: no solve and no training data at serving time.
// W has negative entries (the regularised periodic kernel's b^ are not all positive), so mu I + W G is solved as
// the nonsymmetric matrix it is, by LU; S itself is symmetric (W - W G (mu I + W G)^{-1} W) and is stored as
// (S + S^T) / 2.  Internally a window takes kMvPad = 36 slots (33 features and 3 zeros: a whole number of MFMA k
// steps) and the windows are padded to a multiple of 4 (k_model_std's column tile), R_p = 36 * 4 ceil(nw / 4); the
// added slots have zero features and zero weight, so mu I + W G keeps mu on their diagonal and S is zero there.
// (the slot constants, mv_order and mv_slot are internal.h's, mv_angle and mv_rotate window_points.hpp's:
// feature_gp.hip shares them)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <vector>

#include "model.hpp"
#include "quad_walk.hpp"

namespace nfft4gp_amd {
namespace {

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

// The fit: G = Z^T Z (window_moments) -> mu I + W G -> LU -> S.  Every step is deterministic, so two fits give the
// same bits.  Returns 0, -1, or -2 (rows outside).
int model_fit_variance(Model* M, const double* X, int n, long long ldim)
{
   hipStream_t s = current_stream();
   const int nw = M->nw, Rp = mv_order(nw);
   const size_t rr = (size_t)Rp * Rp;
   Scratch sc(s);
   const double* dX;
   long long ld;
   if (stage(sc, X, (size_t)n, (size_t)M->d, (size_t)ldim, &dX, &ld)) return -1;
   const WindowMap W = window_map(M);
   long long outside = 0;
   if (window_count_outside(W, dX, ld, n, s, &outside)) return -1;
   if (outside) {
      fprintf(stderr, "nfft4gp_amd: Nfft4GPAmdModelFitVariance: %lld of %d rows lie outside the model's domain; "
                      "the model is unchanged.\n", outside, n);
      return -2;
   }
   double *G, *Gc, *A, *S, *d_w;
   if (sc.alloc(&G, rr)) return -1;
   double ms[3] = {0.0, 0.0, 0.0};
   if (window_moments(W, dX, ld, n, nullptr, G, nullptr, nullptr, ms, s)) return -1;
   const auto t0 = std::chrono::steady_clock::now();
   std::vector<double> w((size_t)Rp, 0.0);
   for (int c = 0; c < nw; c++) feature_weights(M->kernel, M->l, M->scale[c], nw, w.data() + (size_t)c * kMvPad);
   if (sc.alloc(&d_w, w.size())) return -1;
   NFFT4GP_HIP_CHECK(hipMemcpy(d_w, w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice));
   if (sc.alloc(&Gc, rr) || sc.alloc(&A, rr) || sc.alloc(&S, rr)) return -1;
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
   sc.trade(&M->d_S, S);  // the previous matrix, if any, goes with the call
   M->R = kMvFeat * nw;
   model_drop_sampler(M);
   return 0;
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
   const int tid = threadIdx.x;
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
   bool outside[1] = {false};
   if (part == 0 && live) {
      outside[0] = row_outside(centre, scale, feature, nw, X, ldim, ip);
      out[ip] = outside[0] ? __builtin_nan("") : sqrt(fabs(ff * (noise + s_q[p])));
   }
   block_count_outside<kMsThreads>(outside, cnt_out);
}

int model_predict_std(Model* M, const double* Xnew, int n_new, long long ldim, double* std_out, int with_noise,
                      long long* n_outside)
{
   hipStream_t s = current_stream();
   Scratch sc(s);
   const int nw = M->nw, Rp = mv_order(nw);
   const double ff = M->f * M->f, noise = with_noise ? M->mu : 0.0;
   const double* dX;
   long long ld;
   if (stage(sc, Xnew, (size_t)n_new, (size_t)M->d, (size_t)ldim, &dX, &ld)) return -1;
   const bool odev = is_device_ptr(std_out);
   double* dout = std_out;
   if (!odev && sc.alloc(&dout, (size_t)n_new)) return -1;
   static const bool attr = []() {
      (void)hipFuncSetAttribute((const void*)k_model_std, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMsLds);
      (void)hipGetLastError();
      return true;
   }();
   (void)attr;
   const size_t nblk = ((size_t)n_new + kMsPts - 1) / kMsPts;
   if (n_outside && M->counts.grow(nblk)) return -1;
   hipLaunchKernelGGL(k_model_std, dim3((unsigned int)nblk), dim3(kMsThreads), kMsLds, s, (const double*)M->d_S, Rp,
                      (const double*)M->d_centre, (const double*)M->d_scale, (const int*)M->d_feature, nw, dX, ld, n_new,
                      ff, noise, dout, n_outside ? M->counts.d : (unsigned int*)nullptr);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   if (!odev)
      NFFT4GP_HIP_CHECK(hipMemcpyAsync(std_out, dout, sizeof(double) * (size_t)n_new, hipMemcpyDeviceToHost, s));
   if (n_outside && M->counts.read(nblk, s, n_outside)) return -1;
   return sc.finish();
}

}  // namespace
}  // namespace nfft4gp_amd

using namespace nfft4gp_amd;

extern "C" {

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
         S[(size_t)i * R + j] = h[(size_t)mv_slot(i) * Rp + mv_slot(j)];
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
         h[(size_t)mv_slot(i) * Rp + mv_slot(j)] = S[(size_t)i * R + j];
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

}  // extern "C"
